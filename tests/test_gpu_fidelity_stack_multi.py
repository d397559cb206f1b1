"""gpu: the multi-ranking stack (gsat_fidelity_stack_multi, dp_gsat_amd.explanation_stack_multi) bit for bit against
``explanation_stack`` (R = 1), tests/fidelity_multi_oracle.py and the unchanged ``edge_subgraph_padded`` variant by variant -- edge counts
around the workgroup's 1024 edge slots, padded / ragged / plain inputs, overflow and bad ids, guard words, capture, repeatability --
and ``gsat_fidelity_stack`` itself against outputs recorded from the commit before this entry existed
(tests/golden/fidelity_stack_parent.npz)."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import fidelity_multi_cases as fc
from tests import fidelity_multi_oracle as fmo
from tests import train_log as tl
from tests.test_gpu_padded_subgraph import _as_padded
from tests.test_gpu_subgraph import _batch
from tests.util import assert_no_memset_nodes

pytestmark = pytest.mark.gpu
GUARD = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fidelity_stack_parent.npz")
OUT = ("edge_index", "edge_id", "batch", "valid")


def _case(E, R, ks, kind="plain", seed=0):
    """(host batch, uint8[R, E_full] levels): a plain Batch, a PaddedBatch with slack, or a ragged one with three trailing empty graph
    slots.  Level entries behind the real edges are garbage the kernels must not load."""
    levels, ei, batch, counts = fc.ranking_levels(E, R, ks, seed)
    G = len(counts)
    if kind == "plain":
        return _batch(ei, batch, G), levels
    if kind == "ragged":
        b = _as_padded(_batch(ei, batch, G + 3), (len(batch) + 4, E + 6), graphs=G)
        b.ragged = True
    else:
        b = _as_padded(_batch(ei, batch, G), (len(batch) + 9, E + 13), overflow=int(kind == "overflowed"))
    slack = b.num_edges - E
    junk = np.random.RandomState(E).randint(0, 256, size=(R, slack)).astype(np.uint8)
    return b, np.concatenate([levels, junk], axis=1)


def _sync_free(fn, *a, **kw):
    import dp_gsat_amd as G
    G.set_sync_free(True)               # nothing read back: an overflow is a result here, not an exception
    try:
        return fn(*a, **kw)
    finally:
        G.set_sync_free(False)


def _oracle(b, stack, levels):
    valid_in = b.valid.tolist() if hasattr(b, "valid") else None
    real = b.num_graphs - (1 if valid_in is not None else 0)
    off = stack.segment_offsets
    caps = [off[v + 1] - off[v] for v in range(stack.variants)]
    return fmo.stack_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), real, levels, len(stack.levels), caps, stack.node_capacity,
                            valid_in, stack.graphs_per_variant)


def _check(dev, b, d, stack, levels, R, S, what):
    """The stack against the oracle, and every variant against ``edge_subgraph_padded`` at its mask and capacity, bit for bit."""
    import dp_gsat_amd as G
    V, N_cap, Gp, off = stack.variants, stack.node_capacity, stack.graphs_per_variant, stack.segment_offsets
    assert stack.rankings == R and V == 1 + 2 * R * S and tuple(stack.edge_level.shape) == (R, b.num_edges), what
    assert stack.num_graphs == V * Gp and stack.x.shape[0] == V * N_cap == stack.batch.shape[0] and stack.valid.shape == (V, 4), what
    o = _oracle(b, stack, levels)
    for name in ("edge_index", "edge_id", "batch"):
        assert np.array_equal(getattr(stack, name).cpu().numpy(), o[name]), (what, name)
    assert np.array_equal(stack.valid.cpu().numpy().astype(np.int64), o["valid"]) and list(off) == o["offsets"], what
    lv = torch.from_numpy(np.minimum(levels, S)).to(dev)
    masks = [(0, torch.ones(b.num_edges, dtype=torch.bool, device=dev))]
    masks += [(fmo.variant_index(R, S, r, s, True), lv[r] <= s) for r in range(R) for s in range(S)]
    masks += [(fmo.variant_index(R, S, r, s, False), lv[r] > s) for r in range(R) for s in range(S)]
    assert sorted(v for v, _ in masks) == list(range(V))
    for v, mask in masks:
        sub = _sync_free(G.edge_subgraph_padded, d, mask, (N_cap, off[v + 1] - off[v]), drop_isolated=False)
        seg, rows = slice(off[v], off[v + 1]), slice(v * N_cap, (v + 1) * N_cap)
        assert torch.equal(stack.edge_index[:, seg], sub.edge_index + v * N_cap), (what, v, "edge_index")
        assert torch.equal(stack.edge_id[seg], sub.edge_id), (what, v, "edge_id")
        assert torch.equal(stack.valid[v], sub.valid), (what, v, stack.valid[v].tolist(), sub.valid.tolist())
        assert torch.equal(stack.batch[rows], sub.batch + v * Gp), (what, v, "batch")
        assert torch.equal(stack.edge_attr[seg], sub.edge_attr), (what, v, "edge_attr")
    return o


@pytest.mark.parametrize("E", fc.EDGE_COUNTS)
def test_one_ranking_is_byte_equal_to_explanation_stack(dev, E):
    import dp_gsat_amd as G
    G.clear_cache()
    ks = list(fc.KS[:3])
    b, levels = _case(E, 1, ks)
    d = b.to(dev)
    lv = torch.from_numpy(levels).to(dev)
    one = _sync_free(G.explanation_stack, d, None, ks=ks, edge_level=lv[0].contiguous())
    multi = _sync_free(G.explanation_stack_multi, d, None, ks=ks, edge_levels=lv)
    assert one.rankings == multi.rankings == 1 and one.variants == multi.variants == 7 and one.segment_offsets == multi.segment_offsets
    for name in OUT + ("x", "edge_attr"):
        assert torch.equal(getattr(one, name), getattr(multi, name)), (E, name)
    assert torch.equal(multi.edge_level, lv) and torch.equal(one.edge_level, lv[0])
    _check(dev, b, d, multi, levels, 1, 3, f"R=1 E={E}")
    G.clear_cache()


@pytest.mark.parametrize("name,E,ks,padded", [("plain_1025", 1025, (3, 40, 200), False), ("padded_2049", 2049, (3, 300), True)])
def test_gsat_fidelity_stack_still_writes_what_the_parent_commit_wrote(dev, name, E, ks, padded):
    """The recorded arrays are the outputs of ``explanation_stack`` (gsat_fidelity_stack) built from the commit before
    gsat_fidelity_stack_multi existed, on these very inputs."""
    import dp_gsat_amd as G
    G.clear_cache()
    gold = np.load(GOLDEN)
    b, levels = _case(E, 1, list(ks), "padded" if padded else "plain")
    if padded:
        levels[:, E:] = 0                                  # the recording had zeros behind the real edges; they are never loaded
    stack = _sync_free(G.explanation_stack, b.to(dev), None, ks=list(ks), edge_level=torch.from_numpy(levels[0].copy()).to(dev))
    for f in OUT:
        got, want = getattr(stack, f).cpu().numpy(), gold[f"{name}.{f}"]
        assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), (name, f)
    G.clear_cache()


@pytest.mark.parametrize("E", fc.EDGE_COUNTS)
@pytest.mark.parametrize("R,S", [(2, 1), (2, 5), (3, 1), (3, 5), (2, 8)])
def test_every_variant_equals_the_oracle_and_the_padded_extraction(dev, E, R, S):
    import dp_gsat_amd as G
    G.clear_cache()
    ks = list(fc.KS[:S]) if S <= len(fc.KS) else [3, 10, 40, 90, 200, 260, 300, 400]
    b, levels = _case(E, R, ks)
    d = b.to(dev)
    what = f"E={E} R={R} S={S}"
    stack = _sync_free(G.explanation_stack_multi, d, None, ks=ks, edge_levels=torch.from_numpy(levels).to(dev))
    o = _check(dev, b, d, stack, levels, R, S, what)
    assert not o["valid"][:, 3].any() and int(o["valid"][0, 1]) == E and int(o["valid"][:, 1].sum()) == (1 + R * S) * E, what
    off = stack.segment_offsets
    seg = lambda v: stack.edge_id[off[v]:off[v + 1]]
    if R == 3:                                             # rankings 0 and 2 are the same ranking: identical variants
        for s in range(S):
            for keep in (True, False):
                assert torch.equal(seg(fmo.variant_index(R, S, 0, s, keep)), seg(fmo.variant_index(R, S, 2, s, keep))), (what, s, keep)
    if E > 1000:                                           # a ranking and its reverse share no edge of a large graph at the smallest level
        a, c = seg(1), seg(1 + S)
        counts = fc.graph_edge_counts(E)
        big = torch.from_numpy(np.repeat(np.asarray(counts) >= 2 * ks[0], counts)).to(dev)
        a, c = a[a >= 0], c[c >= 0]
        assert not set(a[big[a]].tolist()) & set(c[big[c]].tolist()), what
    again = _sync_free(G.explanation_stack_multi, d, None, ks=ks, edge_levels=torch.from_numpy(levels).to(dev))
    for name in OUT + ("x", "edge_attr", "edge_level"):
        assert torch.equal(getattr(stack, name), getattr(again, name)), (what, name)          # bitwise repeatable
    G.clear_cache()


@pytest.mark.parametrize("kind", ["padded", "ragged", "plain", "overflowed"])
@pytest.mark.parametrize("E", [1025, 2049])
def test_input_forms_and_levels_from_attentions(dev, kind, E):
    """Padded, ragged (trailing empty slots), plain and overflowed inputs; the levels come from attentions here, so ranking r of the stack
    is ``explanation_levels`` of attention r."""
    import dp_gsat_amd as G
    G.clear_cache()
    R, ks = 2, [3, 40, 200]
    b, _ = _case(E, R, ks, kind)
    d = b.to(dev)
    gen = torch.Generator().manual_seed(E)
    atts = [torch.rand(b.num_edges, generator=gen).to(dev) for _ in range(R)]
    atts[1][::5] = 0.5                                     # ties: the tie rule is the ranking's, unchanged
    bound = max(fc.graph_edge_counts(E))
    stack = _sync_free(G.explanation_stack_multi, d, atts, ks=ks, max_seg_edges=bound)
    real = b.num_graphs - (1 if hasattr(b, "valid") else 0)
    for r in range(R):
        want = _sync_free(G.explanation_levels, atts[r], d.edge_index, d.batch, ks=ks, num_graphs=b.num_graphs, max_seg_edges=bound,
                          ranked_graphs=real)
        assert torch.equal(stack.edge_level[r], want), (kind, E, r)
    _check(dev, b, d, stack, stack.edge_level.cpu().numpy(), R, 3, f"{kind} E={E}")
    if kind == "overflowed":
        assert (stack.valid.cpu() == torch.tensor([0, 0, 0, 1], dtype=torch.int32)).all() and (stack.edge_id == -1).all()
        with pytest.raises(ValueError, match="does not fit"):
            stack.check()
    else:
        assert not int(stack.valid[:, 3].any()) and int(stack.valid[0, 1]) == E
        stack.check()
    G.clear_cache()


def _raw_call(dev, d, level, R, S, Gp, N_cap, offsets, real, bufs=None):
    """gsat_fidelity_stack_multi itself, into buffers with GUARD sentinel elements on both sides of every output."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.graph_index import call_size
    V, E_stack = 2 * R * S + 1, offsets[-1]
    E, N = int(d.edge_index.shape[1]), int(d.x.shape[0])
    if bufs is None:
        bufs = dict(ei=torch.full((2 * E_stack + 2 * GUARD,), -77, dtype=torch.int64, device=dev),
                    eid=torch.full((E_stack + 2 * GUARD,), -77, dtype=torch.int64, device=dev),
                    batch=torch.full((V * N_cap + 2 * GUARD,), -77, dtype=torch.int64, device=dev),
                    valid=torch.full((4 * V + 2 * GUARD,), -77, dtype=torch.int32, device=dev))
        ws_bytes = call_size("gsat_fidelity_stack_multi_workspace_bytes", E, R, S)
        assert ws_bytes > 0
        bufs["ws"] = torch.full((ws_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    inner = {k: t[GUARD:t.numel() - GUARD] for k, t in bufs.items()}
    valid_in = getattr(d, "valid", None)
    call("gsat_fidelity_stack_multi", ptr(d.edge_index), E, N, ptr(d.batch), real, ptr(valid_in) if valid_in is not None else None,
         ptr(level), R, S, Gp, N_cap, (ctypes.c_int64 * (V + 1))(*offsets), ptr(inner["ei"]), ptr(inner["eid"]), ptr(inner["batch"]),
         ptr(inner["valid"]), ptr(inner["ws"]), inner["ws"].numel(), stream())
    return bufs, inner


def _guards_intact(bufs, what):
    for name, t in bufs.items():
        sentinel = 0xA5 if name == "ws" else -77
        assert (t[:GUARD] == sentinel).all() and (t[-GUARD:] == sentinel).all(), (what, name)


def _equals_oracle(inner, o, what):
    assert np.array_equal(inner["ei"].view(2, -1).cpu().numpy(), o["edge_index"]) and np.array_equal(inner["eid"].cpu().numpy(), o["edge_id"]), what
    assert np.array_equal(inner["batch"].cpu().numpy(), o["batch"]), what
    assert np.array_equal(inner["valid"].view(-1, 4).cpu().numpy().astype(np.int64), o["valid"]), what


def test_overflow_of_one_variant_alone_a_bad_id_spoils_all_and_guards_stay(dev):
    import dp_gsat_amd as G
    G.clear_cache()
    E, R, S, ks = 2049, 2, 3, [3, 40, 200]
    b, levels = _case(E, R, ks)
    d = b.to(dev)
    lv = torch.from_numpy(levels).to(dev)
    N, real, Gp, N_cap = b.num_nodes, b.num_graphs, b.num_graphs + 1, b.num_nodes + 2
    kept = [E] + [int((levels[r] <= s).sum()) for r in range(R) for s in range(S)] + [int((levels[r] > s).sum()) for r in range(R) for s in range(S)]
    tight = fmo.variant_index(R, S, 1, 1, False)          # ranking 1, level 1, the drop variant: one slot short
    caps = [k + 2 for k in kept]
    caps[tight] = kept[tight] - 1
    off = np.concatenate([[0], np.cumsum(caps)]).tolist()
    bufs, inner = _raw_call(dev, d, lv, R, S, Gp, N_cap, off, real)
    torch.cuda.synchronize()
    _guards_intact(bufs, "one tight segment")
    o = fmo.stack_oracle(b.edge_index.numpy(), N, b.batch.numpy(), real, levels, S, caps, N_cap, None, Gp)
    _equals_oracle(inner, o, "one tight segment")
    flags = inner["valid"].view(-1, 4)[:, 3].tolist()
    assert flags == [int(v == tight) for v in range(1 + 2 * R * S)]
    assert (inner["eid"][off[tight]:off[tight + 1]] == -1).all()
    # a node id out of range, in the second workgroup: every variant is all padding
    bad = _batch(b.edge_index.numpy().copy(), b.batch.numpy(), b.num_graphs)
    bad.edge_index[1, 1500] = N + 1
    bufs, inner = _raw_call(dev, bad.to(dev), lv, R, S, Gp, N_cap, off, real)
    torch.cuda.synchronize()
    _guards_intact(bufs, "bad id")
    _equals_oracle(inner, fmo.stack_oracle(bad.edge_index.numpy(), N, b.batch.numpy(), real, levels, S, caps, N_cap, None, Gp), "bad id")
    assert (inner["valid"].view(-1, 4).cpu() == torch.tensor([0, 0, 0, 1], dtype=torch.int32)).all() and (inner["eid"] == -1).all()
    # an overflowed padded input
    p, plv = _case(E, R, ks, "overflowed")
    dp = p.to(dev)
    caps_p = fmo.segment_capacities(p.num_edges, p.num_graphs - 1, R, ks=ks)
    off_p = np.concatenate([[0], np.cumsum(caps_p)]).tolist()
    bufs, inner = _raw_call(dev, dp, torch.from_numpy(plv).to(dev), R, S, p.num_graphs, p.num_nodes, off_p, p.num_graphs - 1)
    torch.cuda.synchronize()
    _guards_intact(bufs, "overflowed input")
    _equals_oracle(inner, fmo.stack_oracle(p.edge_index.numpy(), p.num_nodes, p.batch.numpy(), p.num_graphs - 1, plv, S, caps_p, p.num_nodes,
                                           p.valid.tolist(), p.num_graphs), "overflowed input")
    assert (inner["valid"].view(-1, 4).cpu() == torch.tensor([0, 0, 0, 1], dtype=torch.int32)).all()
    G.clear_cache()


def test_the_capture_holds_four_kernel_nodes_and_replays_on_new_levels(dev):
    import dp_gsat_amd as G
    G.clear_cache()
    E, R, S, ks = 2049, 2, 5, list(fc.KS)
    b, levels = _case(E, R, ks, "ragged")
    _, other = _case(E, R, ks, "ragged", seed=1)          # the same graphs ranked differently
    levels2 = np.ascontiguousarray(other[::-1])
    assert not np.array_equal(levels, levels2)
    d = b.to(dev)
    real, Gp, N_cap = b.num_graphs - 1, b.num_graphs, b.num_nodes
    caps = fmo.segment_capacities(b.num_edges, real, R, ks=ks)
    off = np.concatenate([[0], np.cumsum(caps)]).tolist()
    static = torch.from_numpy(levels).to(dev)
    want = [fmo.stack_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), real, l, S, caps, N_cap, b.valid.tolist(), Gp)
            for l in (levels, levels2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bufs, inner = _raw_call(dev, d, static, R, S, Gp, N_cap, off, real)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _guards_intact(bufs, "eager")
    _equals_oracle(inner, want[0], "eager")
    first = {k: inner[k].clone() for k in ("ei", "eid", "batch", "valid")}
    graph = tl.kept_debug_graph()
    assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
    with torch.cuda.graph(graph):
        _raw_call(dev, d, static, R, S, Gp, N_cap, off, real, bufs)
    path = os.path.join(tempfile.mkdtemp(), "graph.dot")
    graph.debug_dump(path)
    dot = open(path, errors="replace").read()
    assert assert_no_memset_nodes(dot, "gsat_fidelity_stack_multi") and "memcpy" not in dot.lower()
    nodes = tl.kernel_nodes(dot)
    assert nodes is not None, dot[:2000]
    assert len(nodes) == 4 and [n for k in ("k_stkm_hist", "k_stkm_scan", "k_stkm_scatter", "k_stk_fill") for n in nodes if k in n] == nodes, nodes
    for which, l in ((1, levels2), (0, levels)):
        static.copy_(torch.from_numpy(l))
        for name in ("ei", "eid", "batch", "valid"):
            inner[name].fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        _guards_intact(bufs, f"replay {which}")
        _equals_oracle(inner, want[which], f"replay {which}")
    for k, t in first.items():
        assert torch.equal(inner[k], t), k                                             # the second run of the same levels: bitwise equal
    G.clear_cache()


def test_seventeen_flat_levels_are_refused(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import GsatHipError
    b, levels = _case(61, 1, [3])
    d = b.to(dev)
    lv = torch.from_numpy(levels).to(dev)
    ok = _sync_free(G.explanation_stack_multi, d, None, ks=[3], edge_levels=[lv[0]] * 16)            # R S = 16: the limit
    assert ok.variants == 33 and ok.rankings == 16
    with pytest.raises(ValueError, match="at most 16"):
        G.explanation_stack_multi(d, None, ks=[3], edge_levels=[lv[0]] * 17)
    with pytest.raises(ValueError, match="at most 16"):
        G.explanation_stack_multi(d, None, ks=list(range(1, 10)), edge_levels=[lv[0]] * 2)
    off = list(range(0, 36 * 61, 61))
    with pytest.raises(GsatHipError, match="rankings \\* levels <= 16"):
        _raw_call(dev, d, lv, 17, 1, b.num_graphs + 1, b.num_nodes + 2, off, b.num_graphs,
                  bufs={k: torch.zeros(8192 + 2 * GUARD, dtype=t, device=dev) for k, t in
                        (("ei", torch.int64), ("eid", torch.int64), ("batch", torch.int64), ("valid", torch.int32), ("ws", torch.uint8))})
    G.clear_cache()
