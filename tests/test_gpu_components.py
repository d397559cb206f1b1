"""gpu: gsat_level_components (csrc/components.hip) through the C ABI and through dp_gsat_amd.level_components / largest_component_mask /
component_labels / explanation_connectivity / explanation_subgraph(connected=True), against tests/components_oracle.py.  Every
comparison is integer and exact.  The shapes are the smallest at which a branch can go wrong: the wave / workgroup boundary, the cap,
long diameters, nested levels, every edge form, the tie rule, padded and ragged batches, accumulation, refusals, capture."""
import os

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests import components_oracle as co
from tests import padded_oracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("per_graph", "acc", "node_comp", "edge_big")


def _limits():
    from dp_gsat_amd import explain
    return explain.components_wave_nodes(), explain.components_lds_cap()


# ---- case builders (numpy) ---------------------------------------------------------------------------------------------------------------
def _random_graph(rng, n, S, density=1.2):
    """n nodes, about density * n random slots: self-loops, duplicates and one-directional edges occur, some nodes stay isolated."""
    m = int(density * n) if n else 0
    e = np.stack([rng.randint(0, n, size=m), rng.randint(0, n, size=m)], axis=1) if m else np.zeros((0, 2), np.int64)
    return n, e, rng.randint(0, S + 1, size=m)


def _path(ids, S, rng=None):
    """A path through the nodes in the order ``ids``; one-directional slots, levels random (or all 0)."""
    ids = np.asarray(ids)
    e = np.stack([ids[1:], ids[:-1]], axis=1)
    return len(ids), e, (rng.randint(0, S, size=len(e)) if rng is not None else np.zeros(len(e), np.int64))


def _batch(graphs, rng=None):
    """(edge_index int64[2, E], batch int64[N], level uint8[E]) of graphs given as (n, local edges [m, 2], levels [m]); with ``rng`` the
    edge slots are shuffled over the whole batch, so that edge_order is not the identity."""
    sizes = [g[0] for g in graphs]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ei = np.concatenate([np.asarray(g[1], np.int64).reshape(-1, 2) + starts[i] for i, g in enumerate(graphs)]).T
    level = np.concatenate([np.asarray(g[2], np.int64).reshape(-1) for g in graphs]).astype(np.uint8)
    if rng is not None:
        perm = rng.permutation(ei.shape[1])
        ei, level = ei[:, perm], level[perm]
    return np.ascontiguousarray(ei), np.repeat(np.arange(len(graphs)), sizes).astype(np.int64), level


def _abi(dev, ei, N, seg, G, level, S, bound, valid=None, acc=None, outputs=KEYS):
    """One gsat_level_components call on caller-made segments; the outputs start from the oracle's sentinels."""
    from dp_gsat_amd._lib import call, ptr, stream
    E = ei.shape[1]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)
    t_ei, t_lv = up(ei, np.int64), up(level, np.uint8)
    t_np, t_ep, t_eo = (up(a, np.int32) for a in seg)
    t_valid = up(valid, np.int32) if valid is not None else None
    out = {"per_graph": torch.full((G, S, 5), -7, dtype=torch.int32, device=dev),
           "acc": torch.zeros((S, 8), dtype=torch.int64, device=dev) if acc is None else up(acc, np.int64),
           "node_comp": torch.full((N,), -7, dtype=torch.int32, device=dev), "edge_big": torch.full((E,), 9, dtype=torch.uint8, device=dev)}
    some = lambda t: ptr(t) if t is not None and t.numel() else None
    call("gsat_level_components", some(t_ei), E, N, ptr(t_np), ptr(t_ep), some(t_eo), G, some(t_lv), S, bound, some(t_valid),
         *(some(out[k]) if k in outputs else None for k in KEYS), stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_abi(dev, graphs, S, bound=None, rng=None, valid=None, what=""):
    ei, batch, level = _batch(graphs, rng)
    G, N = len(graphs), len(batch)
    seg = co.segments(ei, batch, G)
    if bound is None:
        bound = max(g[0] for g in graphs)
    got = _abi(dev, ei, N, seg, G, level, S, bound, valid)
    want = co.level_components(ei, N, *seg, G, level, S, bound, valid)
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero((got[k] != want[k]).reshape(-1))[:8])
    return ei, batch, level, seg, got


# ---- 1. sizes at the wave and workgroup boundary, 2. diameter -----------------------------------------------------------------------------
def test_sizes_at_the_wave_and_workgroup_boundary(dev):
    W, cap = _limits()
    assert W == 64 and cap >= 4096
    rng = np.random.RandomState(1)
    S = 3
    mid = lambda: _random_graph(rng, 64, S)
    # waves of one workgroup finish at different rounds: tiny graphs, 64-node graphs and workgroup-tier graphs side by side
    graphs = [(1, np.zeros((0, 2)), []), (2, [(1, 0)], [1]), mid(), _random_graph(rng, W, S, 2.5),
              _random_graph(rng, W + 1, S), mid(), mid(), _path(rng.permutation(cap), S, rng),
              mid(), _random_graph(rng, W + 1, S, 6.0), (0, np.zeros((0, 2)), []), mid()]
    _, _, _, _, got = _check_abi(dev, graphs, S, rng=rng, what="boundary")
    assert got["per_graph"][0].tolist() == [[0] * 5] * S and got["per_graph"][1].tolist() == [[0] * 5, [1, 1, 1, 2, 2], [1, 1, 1, 2, 2]]
    assert got["per_graph"][7, S - 1].tolist() == [1, cap - 1, cap - 1, cap, cap] and got["acc"][0, 7] == 0
    # more slots than the LDS keeps (4 per node of the bound; 256 per wave): the rest is read from global memory
    dense = [_random_graph(rng, 10, S, 40.0), _random_graph(rng, W + 6, S, 9.0), _random_graph(rng, 3, S, 100.0)]
    _check_abi(dev, dense, S, rng=rng, what="dense")


def test_long_diameters_converge_in_the_one_launch(dev):
    W, _ = _limits()
    rng = np.random.RandomState(2)
    graphs = []
    for n in (W, W + 1):
        graphs.append(_path(np.arange(n), 1))                          # the minimum at one end, ids decreasing towards it
        graphs.append(_path(np.arange(n)[::-1], 1))
        graphs.append(_path(rng.permutation(n), 1))
        cyc = _path(np.arange(n), 1)
        graphs.append((n, np.concatenate([cyc[1], [[0, n - 1]]]), np.zeros(n, np.int64)))       # a cycle
        graphs.append((n, np.stack([np.full(n - 1, n - 1), np.arange(n - 1)], axis=1), np.zeros(n - 1, np.int64)))   # a star, centre last
    graphs.append(_path(np.arange(1000), 1))
    _, _, _, _, got = _check_abi(dev, graphs, 1, what="diameter")
    assert (got["per_graph"][:, 0, 0] == 1).all() and (got["node_comp"] == np.repeat(co.segments(*_batch(graphs)[:2], len(graphs))[0][:-1],
                                                                                      [g[0] for g in graphs])).all()


# ---- 3. nested levels, 4. edge forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 16])
def test_nested_levels_equal_independent_single_level_runs(dev, S):
    W, _ = _limits()
    rng = np.random.RandomState(30 + S)
    last = S - 1
    tri = [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (2, 3)]
    graphs = [(7, tri, [0, 0, 0, 0, 0, 0, last]),                     # two components that merge only at the last level
              (4, [(0, 1), (2, 3)], [0, S]),                             # a slot of no level: every level after 0 adds nothing
              (5, [(0, 1), (1, 2), (3, 3)], [last, last, last]),         # nothing kept before the last level; a self-loop
              (6, [(0, 1), (2, 3), (4, 5)], [S, S, S]),                  # every edge in no level
              (3, [(0, 2), (0, 2), (2, 0), (1, 1)], [0, last, 0, 0]),    # duplicates
              _random_graph(rng, 40, S), _random_graph(rng, W + 30, S), _random_graph(rng, 9, S, 3.0), _random_graph(rng, 200, S, 0.7)]
    ei, batch, level, seg, got = _check_abi(dev, graphs, S, rng=rng, what=f"S={S}")
    G, N = len(graphs), len(batch)
    for s in range(S):                                                   # row s of the one launch = a one-level run of its kept set
        one = co.level_components(ei, N, *seg, G, (level > s).astype(np.uint8), 1, max(g[0] for g in graphs))
        assert np.array_equal(got["per_graph"][:, s], one["per_graph"][:, 0]), s
    assert got["per_graph"][3].tolist() == [[0] * 5] * S and got["per_graph"][0, last].tolist() == [1, 7, 7, 6, 6]
    if S > 1:
        assert got["per_graph"][0, 0].tolist() == [2, 6, 3, 6, 3] and got["per_graph"][2, 0].tolist() == [0] * 5
        assert got["per_graph"][1, 0].tolist() == got["per_graph"][1, last].tolist() == [1, 1, 1, 2, 2]


def test_tie_rule_and_untouched_nodes(dev):
    tri = [(0, 1), (1, 2), (2, 0)]
    graphs = [(8, [(5, 6), (6, 7), (7, 5)] + tri, [0] * 6),            # equal kept slots: the component of node 0 wins, 3 and 4 untouched
              (5, [(3, 4), (3, 4), (0, 1)], [0, 0, 0]),                  # two slots against one: the later component wins
              (4, [(2, 2), (0, 1)], [0, 0])]                             # a self-loop ties with an edge: the smaller label wins
    _, _, _, _, got = _check_abi(dev, graphs, 1, what="ties")
    assert got["edge_big"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1]
    assert got["node_comp"].tolist() == [0, 0, 0, -1, -1, 5, 5, 5, 8, 8, -1, 11, 11, 13, 13, 15, -1]


# ---- 6. padded and ragged batches, guards -------------------------------------------------------------------------------------------------
def test_slots_behind_the_valid_count_are_never_read(dev):
    rng = np.random.RandomState(6)
    S = 2
    graphs = [_random_graph(rng, 20, S), _random_graph(rng, 70, S), _random_graph(rng, 12, S, 2.0)]
    ei, batch, level = _batch(graphs)                                    # identity order: the last slots are the last graph's
    G, N, E = 3, len(batch), ei.shape[1]
    seg = co.segments(ei, batch, G)
    ei[:, E - 5:] = 10 ** 9                                              # guard slots: reading one would skip the graph
    level[E - 5:] = 0                                                    # ... or count it at every level
    for word in ([N, E - 5, 3, 0], [N, E - 5, 2, 0], [N, E - 5, 9, 0], [N, 0, 3, 0], [N, E - 5, 3, 1], [N, E - 5, -2, 0]):
        got = _abi(dev, ei, N, seg, G, level, S, 70, word)
        want = co.level_components(ei, N, *seg, G, level, S, 70, word)
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (word, k)
        assert got["acc"][0, 7] == 0 and got["acc"][0, 0] == (0 if word[3] else min(max(word[2], 0), 3))
    assert (got["per_graph"] == -7).all()                                # not looked at: not written


@pytest.mark.parametrize("ragged", [False, True])
def test_padded_batches_count_their_real_graphs_only(dev, ragged):
    import dp_gsat_amd as G
    graphs = po.mutag_graphs(count=12)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    ids = [3, 7, 0, 9, 5] + ([-1, -1] if ragged else [])
    cap = ds.capacity_for(len(ids))
    b = ds.collate_padded(torch.tensor(ids, device=dev), (cap[0] + 3, cap[1] + 6), ragged=ragged)
    Gp, E, S = int(b.num_graphs), int(b.edge_index.shape[1]), 3
    valid = b.valid.tolist()
    assert valid[2] == 5 and valid[1] < E
    rng = np.random.RandomState(8)
    level = rng.randint(0, S + 1, size=E).astype(np.uint8)
    level[valid[1]:] = 0xFF if ragged else 0                             # filler behind valid[1]
    bound = int(ds.node_counts.max())
    kw = dict(num_graphs=Gp, max_seg_nodes=bound, ranked_graphs=Gp - 1, valid=b.valid, per_graph=True, labels=True)
    got = G.level_components(b.edge_index, b.batch, torch.from_numpy(level).to(dev), S, **kw)
    want = co.batch_components(b.edge_index.cpu().numpy(), b.batch.cpu().numpy(), Gp, level, S, bound, Gp - 1, valid)
    assert np.array_equal(got.out.cpu().numpy(), want["acc"]) and int(got.out[0, 0]) == 5 and int(got.out[0, 7]) == 0
    assert np.array_equal(got.per_graph.cpu().numpy(), want["per_graph"]) and tuple(got.per_graph.shape) == (Gp - 1, S, 5)
    assert np.array_equal(got.node_comp.cpu().numpy(), want["node_comp"]) and (got.node_comp[valid[0]:] == -1).all()
    assert np.array_equal(got.edge_big.cpu().numpy(), want["edge_big"].astype(bool)) and not got.edge_big[valid[1]:].any()
    # the same graphs unpadded give the same counts
    ub = ds.collate(torch.tensor(ids[:5], device=dev))
    plain = G.level_components(ub.edge_index, ub.batch, torch.from_numpy(level[:valid[1]]).to(dev), S, num_graphs=5)
    assert torch.equal(plain, got.out)
    spoiled = b.valid.clone()
    spoiled[3] = 1
    assert not G.level_components(b.edge_index, b.batch, torch.from_numpy(level).to(dev), S, **dict(kw, valid=spoiled)).out.any()
    G.clear_cache()


# ---- 7. accumulation, 8. refusals -----------------------------------------------------------------------------------------------------------
def test_accumulation_reset_and_repeatability(dev):
    import dp_gsat_amd as G
    rng = np.random.RandomState(7)
    S = 4
    ei, batch, level = _batch([_random_graph(rng, n, S) for n in (30, 64, 65, 100, 5, 64, 300)], rng)
    level2 = rng.randint(0, S + 1, size=len(level)).astype(np.uint8)
    t = lambda a: torch.from_numpy(a).to(dev)
    d_ei, d_b = t(ei), t(batch)
    a = G.level_components(d_ei, d_b, t(level), S, num_graphs=7)
    b = G.level_components(d_ei, d_b, t(level2), S, num_graphs=7)
    assert a.dtype == torch.int64 and tuple(a.shape) == (S, 8)
    assert np.array_equal(a.cpu().numpy(), co.batch_components(ei, batch, 7, level, S)["acc"])
    both = G.level_components(d_ei, d_b, t(level), S, num_graphs=7)
    assert G.level_components(d_ei, d_b, t(level2), S, num_graphs=7, out=both) is both and torch.equal(both, a + b)
    G.level_components_reset(both)
    assert not both.any()
    again = G.level_components(d_ei, d_b, t(level), S, num_graphs=7, per_graph=True, labels=True)
    once = G.level_components(d_ei, d_b, t(level), S, num_graphs=7, per_graph=True, labels=True)
    assert all(torch.equal(x, y) for x, y in zip(again, once)) and torch.equal(again.out, a)          # bitwise repeatable
    G.clear_cache()


def test_refusals_and_a_wrong_bound_skips_that_graph_alone(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import GsatHipError
    W, cap = _limits()
    rng = np.random.RandomState(9)
    S = 2
    graphs = [_random_graph(rng, 30, S), _random_graph(rng, 10, S), _random_graph(rng, W + 1, S), _random_graph(rng, 8, S)]
    for bound, skipped in ((10, [0, 2]), (W, [2]), (W + 1, [])):
        _, _, _, _, got = _check_abi(dev, graphs, S, bound=bound, what=f"bound {bound}")
        assert got["acc"][0, 7] == len(skipped) and got["acc"][0, 0] == 4 - len(skipped)
        for g in range(4):
            assert (got["per_graph"][g] == -1).all() == (g in skipped)
    # an edge that leaves its graph, and a slot that names no edge: the graph is skipped before anything is indexed with its ids
    ei, batch, level = _batch(graphs)
    seg = co.segments(ei, batch, 4)
    bad = ei.copy()
    bad[1, 0] = int(seg[0][1]) + 3                                       # graph 0's first edge ends in graph 1
    order = seg[2].copy()
    order[seg[1][3]] = ei.shape[1] + 5                                   # graph 3's first slot names no edge
    got = _abi(dev, bad, len(batch), (seg[0], seg[1], order), 4, level, S, W + 1)
    want = co.level_components(bad, len(batch), seg[0], seg[1], order, 4, level, S, W + 1)
    assert all(np.array_equal(got[k], want[k]) for k in KEYS) and got["acc"][0].tolist()[0::7] == [2, 2]
    for bound in (-1, cap + 1):
        with pytest.raises(GsatHipError, match="max_seg_nodes"):
            _abi(dev, ei, len(batch), seg, 4, level, S, bound)
    t = lambda a: torch.from_numpy(a).to(dev)
    d_ei, d_b, d_lv = t(ei), t(batch), t(level)
    with pytest.raises(ValueError, match="components_lds_cap"):
        G.level_components(d_ei, d_b, d_lv, S, num_graphs=4, max_seg_nodes=cap + 1)
    with pytest.raises(ValueError, match="ranked_graphs"):
        G.level_components(d_ei, d_b, d_lv, S, num_graphs=4, ranked_graphs=5)
    with pytest.raises(ValueError, match="valid"):
        G.level_components(d_ei, d_b, d_lv, S, num_graphs=4, valid=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(GsatHipError):
        G.level_components(d_ei.cpu(), d_b, d_lv, S, num_graphs=4)
    G.set_sync_free(True)
    try:
        with pytest.raises(ValueError, match="max_seg_nodes"):
            G.level_components(d_ei, d_b, d_lv, S, num_graphs=4)
        ok = G.level_components(d_ei, d_b, d_lv, S, num_graphs=4, max_seg_nodes=W + 1)
    finally:
        G.set_sync_free(False)
    assert np.array_equal(ok.cpu().numpy(), co.batch_components(ei, batch, 4, level, S)["acc"])
    G.clear_cache()


# ---- 9. capture ---------------------------------------------------------------------------------------------------------------------------
def test_capture_of_levels_and_components_replays_on_new_attention(dev):
    import dp_gsat_amd as G
    from tests import train_log as tl
    from tests.util import assert_no_memset_nodes
    import tempfile
    rng = np.random.RandomState(11)
    graphs = [_random_graph(rng, n, 1) for n in (30, 64, 65, 100, 5, 64, 130)]
    ei, batch, _ = _batch(graphs, rng)
    E, Gn, ratios = ei.shape[1], len(graphs), [0.2, 0.5, 0.9]
    d_ei, d_b = torch.from_numpy(ei).to(dev), torch.from_numpy(batch).to(dev)
    att = [torch.from_numpy(rng.rand(E).astype(np.float32)).to(dev) for _ in range(2)]
    static = att[0].clone()
    out = torch.zeros(3, 8, dtype=torch.int64, device=dev)
    bounds = dict(max_seg_edges=max(len(g[2]) for g in graphs), ranked_graphs=Gn)

    def body():
        level = G.explanation_levels(static, d_ei, d_b, ratios=ratios, num_graphs=Gn, **bounds)
        G.level_components(d_ei, d_b, level, 3, num_graphs=Gn, max_seg_nodes=130, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    graph = tl.kept_debug_graph()
    assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
    with torch.cuda.graph(graph):
        body()
    path = os.path.join(tempfile.mkdtemp(), "graph.dot")
    graph.debug_dump(path)
    dot = open(path, errors="replace").read()
    assert assert_no_memset_nodes(dot, "gsat_level_components") and "memcpy" not in dot.lower()
    assert sum("k_level_components" in n for n in tl.kernel_nodes(dot)) == 1
    G.level_components_reset(out)
    static.copy_(att[1])
    graph.replay()
    torch.cuda.synchronize()
    eager = G.level_components(d_ei, d_b, G.explanation_levels(att[1], d_ei, d_b, ratios=ratios, num_graphs=Gn), 3, num_graphs=Gn)
    assert torch.equal(out, eager)
    want = co.batch_components(ei, batch, Gn, co.levels_of(att[1].cpu().numpy(), ei, batch, Gn, ratios=ratios), 3)
    assert np.array_equal(out.cpu().numpy(), want["acc"])
    G.clear_cache()


# ---- 10. masks, labels, connected subgraphs; 11. real topology ---------------------------------------------------------------------------
def test_largest_component_mask_labels_and_connected_subgraph(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    b = synth.mutag_batch(os.path.join(ROOT, "tests", "golden", "mutag128.npz"), 24).to(dev)
    ei, batch, Gn = b.edge_index.cpu().numpy(), b.batch.cpu().numpy(), int(b.num_graphs)
    E = ei.shape[1]
    att = torch.from_numpy(np.random.RandomState(12).rand(E).astype(np.float32)).to(dev)
    mask = G.topk_edge_mask(att, b.edge_index, b.batch, ratio=0.4, num_graphs=Gn)
    want = co.batch_components(ei, batch, Gn, (~mask.cpu().numpy()).astype(np.uint8), 1)
    big = G.largest_component_mask(b.edge_index, b.batch, mask, num_graphs=Gn)
    assert big.dtype == torch.bool and np.array_equal(big.cpu().numpy(), want["edge_big"].astype(bool))
    assert 0 < int(big.sum()) < int(mask.sum()) and not (big & ~mask).any()
    lab = G.component_labels(b.edge_index, b.batch, mask, num_graphs=Gn)
    assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), want["node_comp"])
    plain = G.explanation_subgraph(att, b, ratio=0.4)
    off = G.explanation_subgraph(att, b, ratio=0.4, connected=False)
    for name in ("x", "edge_index", "batch", "edge_id", "edge_att"):
        assert torch.equal(getattr(plain, name), getattr(off, name)), name
    assert torch.equal(plain.edge_id, torch.nonzero(mask).view(-1))
    on = G.explanation_subgraph(att, b, ratio=0.4, connected=True)
    assert torch.equal(on.edge_id, torch.nonzero(big).view(-1)) and torch.equal(on.edge_att.view(-1), att[big])
    sub = G.edge_subgraph(b, big)
    assert torch.equal(on.edge_index, sub.edge_index) and torch.equal(on.batch, sub.batch)
    # every graph of the connected extraction is one component
    one = G.level_components(on.edge_index, on.batch, torch.zeros(int(on.edge_index.shape[1]), dtype=torch.uint8, device=dev), 1,
                             num_graphs=int(on.num_graphs), per_graph=True)
    assert (one.per_graph[:, 0, 0] <= 1).all() and int(one.out[0, 6]) == int((one.per_graph[:, 0, 0] == 1).sum()) > 0
    G.clear_cache()


def test_explanation_connectivity_on_mutag(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    b = synth.mutag_batch(os.path.join(ROOT, "tests", "golden", "mutag128.npz")).to(dev)
    ei, batch, Gn = b.edge_index.cpu().numpy(), b.batch.cpu().numpy(), int(b.num_graphs)
    assert Gn == 128
    ratios = [0.2, 0.5, 1.0]
    att = torch.from_numpy(np.random.RandomState(13).rand(ei.shape[1]).astype(np.float32)).to(dev)
    got = G.explanation_connectivity(b, att, ratios=ratios)
    level = co.levels_of(att.cpu().numpy(), ei, batch, Gn, ratios=ratios)
    assert np.array_equal(G.explanation_levels(att, b.edge_index, b.batch, ratios=ratios, num_graphs=Gn).cpu().numpy(), level)
    oracle = co.batch_components(ei, batch, Gn, level, 3)
    want = dict(co.scores(oracle["acc"]), levels=ratios)
    assert got == want and got["n"] == 128
    # at ratio 1.0 every edge is kept: the components of each whole graph's non-isolated part
    N = len(batch)
    _, lab = connected_components(coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N)), directed=False)
    touched = np.zeros(N, bool)
    touched[ei.reshape(-1)] = True
    whole = [len(np.unique(lab[(batch == g) & touched])) for g in range(Gn)]
    assert oracle["per_graph"][:, 2, 0].tolist() == whole and got["components"][2] == sum(whole) / 128
    by_k = G.explanation_connectivity(b, att, ks=[3, 1000])
    assert by_k["components"][1] == got["components"][2] and by_k["levels"] == [3, 1000]
    G.clear_cache()
