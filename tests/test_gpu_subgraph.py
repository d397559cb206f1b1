"""gpu: dp_gsat_amd.subgraph against the CPU oracle of tests/subgraph_oracle.py -- index outputs bit-exact in both modes at the sizes
the kernels branch on, the row gather, explanation subgraphs, model identity / parity, fidelity, capture, repeatability."""
import re

import numpy as np
import pytest
import torch

from oracle import modules as om
from tests import explain_oracle as xo
from tests import subgraph_oracle as so
from tests.graphs import random_batch, shuffle_edges
from tests.util import TOL, assert_no_memset_nodes, capture_with_dump, close

pytestmark = pytest.mark.gpu


def _block():
    from dp_gsat_amd import subgraph as S
    return S.subgraph_block_items()


def _sized(N, E, seed, undirected=True):
    """random_batch graphs of 2..40 nodes cut / padded with isolated nodes to exactly N nodes, edges trimmed to exactly E."""
    from dp_gsat_amd.synth import Batch
    ei, batch, n = random_batch(seed, max(N // 8, 1) + 2, 2, 40, undirected=undirected)
    ei, batch = ei.numpy(), batch.numpy()
    if n >= N:
        batch = batch[:N]
        ei = ei[:, (ei[0] < N) & (ei[1] < N)]
    else:
        batch = np.concatenate([batch, np.full(N - n, batch.max() + 1, dtype=np.int64)])      # isolated nodes, one more graph
    assert ei.shape[1] >= E, (N, E, ei.shape)
    ei = np.ascontiguousarray(ei[:, :E])
    return _batch(ei, batch)


def _batch(ei, batch, num_graphs=None):
    """A Batch with recognisable attributes of every kind the extraction gathers."""
    from dp_gsat_amd.synth import Batch
    N, E = len(batch), ei.shape[1]
    G = int(batch.max()) + 1 if num_graphs is None else num_graphs
    return Batch(x=torch.arange(N * 3, dtype=torch.float32).view(N, 3), edge_index=torch.from_numpy(np.ascontiguousarray(ei)),
                 batch=torch.from_numpy(batch), edge_attr=torch.arange(E, dtype=torch.float32).view(E, 1) * 0.5,
                 edge_label=torch.arange(E, dtype=torch.int64) % 3, node_label=torch.arange(N, dtype=torch.int64) % 5,
                 y=torch.zeros(G, 1), num_graphs=G)


def _compare(sub, o, b, what):
    assert np.array_equal(sub.counts[:2].cpu().numpy(), np.array(o["counts"])) and sub.counts[2:].tolist() == [0, 0], what
    for name, got in (("node_id", sub.node_id), ("edge_id", sub.edge_id), ("edge_index", sub.edge_index), ("batch", sub.batch),
                      ("node_ptr", sub.node_ptr), ("edge_mask", sub.edge_mask.view(torch.uint8))):
        g = got.cpu().numpy()
        assert g.dtype == o[name].dtype and g.shape == o[name].shape and np.array_equal(g, o[name]), (what, name)
    nid, eid = torch.from_numpy(o["node_id"]), torch.from_numpy(o["edge_id"])
    for name, index in (("x", nid), ("node_label", nid), ("edge_attr", eid), ("edge_label", eid)):
        assert torch.equal(getattr(sub, name).cpu(), getattr(b, name)[index]), (what, name)
    assert sub.num_graphs == b.num_graphs and torch.equal(sub.y.cpu(), b.y)


def _check(dev, b, d, keep, mode, drop=True, what=""):
    import dp_gsat_amd as G
    keep = np.asarray(keep).astype(bool)
    o = so.subgraph_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), so.node_ptr_of(b.batch.numpy(), b.num_graphs), keep,
                           mode, drop)
    k = torch.from_numpy(keep).to(dev)
    sub = G.edge_subgraph(d, k, drop_isolated=drop) if mode == "edge" else G.node_subgraph(d, k)
    _compare(sub, o, b, f"{what} mode={mode} drop={drop}")
    return sub


def _patterns(n, seg_of, seed):
    """Keep patterns over n items; seg_of[i] = graph of item i (for the whole-graph drops)."""
    rng = np.random.RandomState(seed)
    pats = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0, "random": rng.rand(n) < 0.5}
    if n:
        first, last = np.zeros(n, bool), np.zeros(n, bool)
        first[0], last[-1] = True, True
        pats.update(first=first, last=last)
        gmax = int(seg_of.max())
        pats["graphs_dropped"] = (rng.rand(n) < 0.7) & (seg_of != gmax // 2) & (seg_of != gmax)      # one in the middle and the last
    return pats


def _sizes():
    B = _block()
    return [(1, 0), (63, 63), (64, 64), (65, 65), (B - 1, 1), (B, B - 1), (B + 1, B), (2 * B + 1, B + 1)]


@pytest.mark.parametrize("case", range(8))
def test_index_parity_at_the_block_boundaries(dev, case):
    """N in {1, 63, 64, 65, B-1, B, B+1, 2B+1} x E in {0, 1, 63, 64, 65, B-1, B, B+1} (paired), every keep pattern, both modes, isolated
    nodes dropped and kept: every output equals the oracle."""
    import dp_gsat_amd as G
    G.clear_cache()
    N, E = _sizes()[case]
    b = _sized(N, E, seed=100 + case)
    assert b.num_nodes == N and b.num_edges == E
    d = b.to(dev)
    ei, batch = b.edge_index.numpy(), b.batch.numpy()
    for name, keep in _patterns(E, batch[ei[0]], case).items():
        for drop in (True, False):
            _check(dev, b, d, keep, "edge", drop, f"N={N} E={E} {name}")
    for name, keep in _patterns(N, batch, case + 50).items():
        _check(dev, b, d, keep, "node", what=f"N={N} E={E} {name}")
    ids = torch.from_numpy(np.flatnonzero(np.arange(N) % 3 != 1)).to(dev)                 # an int64 id list instead of a mask
    o = so.subgraph_oracle(ei, N, batch, so.node_ptr_of(batch, b.num_graphs), np.arange(N) % 3 != 1, "node")
    _compare(G.node_subgraph(d, ids), o, b, "id list")


def test_index_parity_on_a_large_batch(dev):
    """~300 k nodes, > 2^20 edges: more than one wave of workgroup sums in the second scan level."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    p = synth.powerlaw_batch(num_nodes=300_000, num_edges=1_100_000, num_graphs=8, seed=3)
    b = _batch(p.edge_index.numpy(), p.batch.numpy(), 8)
    assert b.num_edges > (1 << 20) and b.num_edges // _block() > 64
    d = b.to(dev)
    rng = np.random.RandomState(5)
    keep = rng.rand(b.num_edges) < 0.5
    _check(dev, b, d, keep, "edge", True, "large")
    _check(dev, b, d, keep, "edge", False, "large")
    _check(dev, b, d, rng.rand(b.num_nodes) < 0.5, "node", what="large")
    G.clear_cache()


def test_index_parity_on_special_edge_lists(dev):
    """Shuffled edge order, a single-direction batch, self loops, duplicate edges."""
    import dp_gsat_amd as G
    G.clear_cache()
    ei, batch, N = random_batch(7, 40, 2, 40)
    one_way = random_batch(8, 40, 2, 40, undirected=False)
    loops = np.concatenate([ei.numpy(), np.stack([np.arange(0, N, 3), np.arange(0, N, 3)])], axis=1)
    dup = np.concatenate([ei.numpy(), ei.numpy()[:, ::2], ei.numpy()[:, :5]], axis=1)
    cases = {"shuffled": (shuffle_edges(ei, 3).numpy(), batch.numpy()), "one_way": (one_way[0].numpy(), one_way[1].numpy()),
             "self_loops": (loops, batch.numpy()), "duplicates": (dup, batch.numpy())}
    for name, (e, bt) in cases.items():
        b = _batch(e, bt)
        d = b.to(dev)
        rng = np.random.RandomState(len(name))
        keep = rng.rand(b.num_edges) < 0.5
        for drop in (True, False):
            _check(dev, b, d, keep, "edge", drop, name)
        _check(dev, b, d, rng.rand(b.num_nodes) < 0.6, "node", what=name)


def test_gather_rows_widths_alignment_and_empty(dev):
    """Bit-exact against table[index] for row widths of 1, 4, 8, 40, 56, 72 and 512 bytes, 1-D tensors, a table whose base is only
    4-byte aligned, n = 0."""
    import dp_gsat_amd as G
    g = torch.Generator().manual_seed(0)
    n = 5000
    tables = [torch.rand(n, generator=g) < 0.5,                                            # 1 byte, 1-D
              torch.randn(n, 1, generator=g),                                              # 4
              torch.randint(-9, 9, (n,), generator=g),                                     # 8, 1-D
              torch.randn(n, 10, generator=g), torch.randn(n, 14, generator=g),            # 40, 56
              torch.randint(0, 100, (n, 9), generator=g),                                  # 72
              torch.randn(n, 128, generator=g),                                            # 512
              torch.randn(n, 2, 6, generator=g)]                                           # 48, trailing shape of rank 2
    widths = [t[0].numel() * t.element_size() for t in tables]
    assert widths == [1, 4, 8, 40, 56, 72, 512, 48]
    idx = torch.randint(0, n, (7001,), generator=g)
    idx[:3] = torch.tensor([0, n - 1, 0])
    for t in tables:
        got = G.gather_rows(t.to(dev), idx.to(dev))
        assert got.dtype == t.dtype and torch.equal(got.cpu(), t[idx]), tuple(t.shape)
        assert G.gather_rows(t.to(dev), idx[:0].to(dev)).shape == (0,) + tuple(t.shape[1:])
    for cols in (10, 4, 1):                                                                # the view starts one element (4 bytes) in
        base = torch.randn(n * cols + 1, generator=g).to(dev)
        view = base[1:].view(n, cols)
        assert view.is_contiguous() and view.data_ptr() % 8 == 4
        assert torch.equal(G.gather_rows(view, idx.to(dev)).cpu(), view.cpu()[idx])
    bytes_view = (torch.rand(n + 1, generator=g) < 0.5).to(dev)[1:]                        # a byte table at an odd address
    assert torch.equal(G.gather_rows(bytes_view, idx.to(dev)).cpu(), bytes_view.cpu()[idx])


def _att(E, seed):
    return (np.random.RandomState(seed).randint(0, 17, size=E) / 16.0).astype(np.float32)     # "quantised": multiples of 1/16, mass ties


def _symmetrised(b, seed):
    """One value per undirected edge: every edge is tied with its reverse."""
    ei = b.edge_index.numpy()
    key = np.minimum(ei[0], ei[1]) * b.num_nodes + np.maximum(ei[0], ei[1])
    _, inv = np.unique(key, return_inverse=True)
    return np.random.RandomState(seed).rand(inv.max() + 1).astype(np.float32)[inv]


def _topk_oracle(att, b, k, ratio):
    ei, batch = b.edge_index.numpy(), b.batch.numpy()
    if k is not None:
        return xo.rank_oracle(att, ei, batch, b.num_graphs, k)[2].astype(bool)
    return xo.topk_ratio_oracle(att, ei, batch, b.num_graphs, ratio)


@pytest.mark.parametrize("kind", ["quantised", "symmetrised"])
def test_explanation_subgraph_equals_oracle_on_the_topk(dev, kind):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    p = synth.ba2motifs_batch(num_graphs=24, seed=2)
    b = _batch(p.edge_index.numpy(), p.batch.numpy(), 24)
    d = b.to(dev)
    att = _att(b.num_edges, 4) if kind == "quantised" else _symmetrised(b, 5)
    a = torch.from_numpy(att).to(dev)
    ptr = so.node_ptr_of(b.batch.numpy(), 24)
    for k, ratio in ((1, None), (5, None), (None, 0.3), (None, 1.0)):
        top = _topk_oracle(att, b, k, ratio)
        for complement in (False, True):
            keep = ~top if complement else top
            o = so.subgraph_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), ptr, keep, "edge", True)
            sub = G.explanation_subgraph(a.view(-1, 1), d, k=k, ratio=ratio, complement=complement)
            _compare(sub, o, b, f"{kind} k={k} ratio={ratio} complement={complement}")
            assert sub.edge_att.shape == (o["counts"][1], 1) and np.array_equal(sub.edge_att.view(-1).cpu().numpy(), att[o["edge_id"]])
    empty = G.explanation_subgraph(a, d, ratio=1.0, complement=True)                       # nothing left: well-formed empty tensors
    assert empty.x.shape == (0, 3) and empty.edge_index.shape == (2, 0) and empty.edge_attr.shape == (0, 1) and empty.num_graphs == 24
    assert empty.node_ptr.tolist() == [0] * 25 and empty.edge_att.shape == (0,)


def _models(dev, data, backbone, H=64):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=0.0, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=synth.in_degree_histogram(data))
    oclf = (om.GIN if backbone == "GIN" else om.PNA)(data.x.shape[1], 0, 2, False, cfg).eval()
    clf = G.get_model(data.x.shape[1], 0, 2, False, cfg, dev).eval()
    clf.load_state_dict(oclf.state_dict())
    return oclf, clf


def _differs(a, b):
    """Some graph's logits differ by more than tests.util.close would allow."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return (a - b).abs().max().item() > TOL * max(1.0, b.abs().max().item())


def test_hard_mask_equals_removed_edges_for_gin_but_not_for_pna(dev):
    """GIN: the forward on the batch without the edges equals the forward with a 0/1 edge_atten.  PNA: it does not (a message scaled by
    0 still enters mean / min / max / std and the degree) -- which is why the compacted graph exists."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    data = synth.ba2motifs_batch(num_graphs=16, seed=4)
    d = data.to(dev)
    m = torch.from_numpy(np.random.RandomState(0).rand(data.num_edges) < 0.5).to(dev)
    sub = G.edge_subgraph(d, m, drop_isolated=False)
    assert sub.num_nodes == data.num_nodes and sub.num_edges == int(m.sum())
    with torch.no_grad():
        _, gin = _models(dev, data, "GIN")
        masked = gin(d.x, d.edge_index, d.batch, None, edge_atten=m.float().view(-1, 1))
        close(gin(sub.x, sub.edge_index, sub.batch, None), masked, what="GIN removed vs masked")
        _, pna = _models(dev, data, "PNA")
        masked = pna(d.x, d.edge_index, d.batch, None, edge_atten=m.float().view(-1, 1))
        removed = pna(sub.x, sub.edge_index, sub.batch, None)
    assert removed.shape == masked.shape == (16, 1) and _differs(removed, masked)


@pytest.mark.parametrize("backbone", ["GIN", "PNA"])
def test_model_forward_on_an_extracted_batch_matches_the_oracle(dev, backbone):
    """drop_isolated=True with one graph emptied completely: its segment is empty, the model still returns one row per graph."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    data = synth.ba2motifs_batch(num_graphs=16, seed=6)
    keep = np.random.RandomState(1).rand(data.num_edges) < 0.6
    keep[data.batch.numpy()[data.edge_index.numpy()[0]] == 7] = False
    ob, o = so.extract_batch(data, keep, "edge", True)
    assert o["node_ptr"][7] == o["node_ptr"][8] and ob.batch.max() == 15
    oclf, clf = _models(dev, data, backbone)
    sub = G.edge_subgraph(data.to(dev), torch.from_numpy(keep).to(dev), drop_isolated=True)
    assert np.array_equal(sub.node_ptr.cpu().numpy(), o["node_ptr"])
    with torch.no_grad():
        got = clf(sub.x, sub.edge_index, sub.batch, None)
        ref = oclf(ob.x, ob.edge_index, ob.batch, None)
    assert got.shape == (16, 1)
    close(got, ref, what=f"{backbone} on the extracted batch")


@pytest.mark.parametrize("backbone,classes", [("GIN", 2), ("PNA", 2), ("GIN", 3)])
def test_explanation_fidelity_matches_the_oracle(dev, backbone, classes):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    data = synth.ba2motifs_batch(num_graphs=16, seed=8)
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=32, dropout_p=0.0, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=synth.in_degree_histogram(data))
    oclf = (om.GIN if backbone == "GIN" else om.PNA)(10, 0, classes, False, cfg).eval()
    clf = G.get_model(10, 0, classes, False, cfg, dev).train()
    clf.load_state_dict(oclf.state_dict())
    att = _symmetrised(data, 9)
    for k, ratio in ((5, None), (None, 0.3)):
        top = _topk_oracle(att, data, k, ratio)
        with torch.no_grad():
            full = oclf(data.x, data.edge_index, data.batch, None)
            lk, ld = (oclf(s.x, s.edge_index, s.batch, None) for s in (so.extract_batch(data, top, "edge", False)[0],
                                                                          so.extract_batch(data, ~top, "edge", False)[0]))
        if classes == 2:
            sign = torch.where(full >= 0, 1.0, -1.0).double()
            pf, pk, pd = (torch.sigmoid(sign * z.double()).view(-1) for z in (full, lk, ld))
        else:
            cls = full.argmax(dim=1, keepdim=True)
            pf, pk, pd = (torch.softmax(z.double(), dim=1).gather(1, cls).view(-1) for z in (full, lk, ld))
        res = G.explanation_fidelity(clf, data.to(dev), torch.from_numpy(att).to(dev), k=k, ratio=ratio)
        assert clf.training                                                                # the mode is restored
        bound = 0.0
        for name, ref in (("logits_full", full), ("logits_keep", lk), ("logits_drop", ld)):
            assert res[name].is_cuda and res[name].shape == (16, 1 if classes == 2 else classes)
            close(res[name], ref, what=name)
            bound = max(bound, TOL * max(1.0, ref.abs().max().item()))
        # sigmoid is 1/4-Lipschitz and softmax 1-Lipschitz: the logits' absolute bound carries over to the probabilities' means
        for name, ref in (("fidelity_plus", (pf - pd).mean()), ("fidelity_minus", (pf - pk).mean())):
            assert res[name].is_cuda and res[name].dim() == 0
            assert abs(res[name].item() - ref.item()) <= bound, (name, res[name].item(), ref.item())


def _graph_nodes(dot_text):
    """Names of the nodes a hipGraphDebugDotPrint dump declares (None when there is no dump or it declares its nodes in a form this
    does not know: then, as in tests.util, the count cannot be taken)."""
    if dot_text is None:
        return None
    names = set()
    for line in dot_text.splitlines():
        m = re.match(r'^\s*"?([\w.]+)"?\s*\[', line)
        if m and "->" not in line and m.group(1) not in ("node", "edge", "graph"):
            names.add(m.group(1))
    return names or None


def _two_masks_with_equal_counts(b, seed):
    """Two different edge masks that keep the same number of edges AND touch the same number of nodes: the second keeps the reverse
    copy of every edge the first keeps (random_batch lists an undirected edge as two consecutive entries)."""
    E = b.num_edges
    pick = np.random.RandomState(seed).rand(E // 2) < 0.5
    m0, m1 = np.zeros(E, bool), np.zeros(E, bool)
    m0[0:2 * (E // 2):2], m1[1:2 * (E // 2):2] = pick, pick
    return m0, m1


def test_capture_with_declared_sizes_and_replay_on_a_refilled_mask(dev, monkeypatch):
    import dp_gsat_amd as G
    from dp_gsat_amd import subgraph as S
    G.clear_cache()
    B = _block()
    b = _sized(B + 70, B + 1, seed=31)
    d = b.to(dev)
    ptr = so.node_ptr_of(b.batch.numpy(), b.num_graphs)
    m0, m1 = _two_masks_with_equal_counts(b, 1)
    o0, o1 = (so.subgraph_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), ptr, m, "edge", True) for m in (m0, m1))
    assert o0["counts"] == o1["counts"] and not np.array_equal(o0["edge_id"], o1["edge_id"])
    mask = torch.from_numpy(m0).to(dev)
    out = {}

    def step():
        out["sub"] = G.edge_subgraph(d, mask, drop_isolated=True, sizes=o0["counts"])

    with pytest.raises(ValueError):                                                        # never a silent read-back
        G.set_sync_free(True)
        try:
            G.edge_subgraph(d, mask)
        finally:
            G.set_sync_free(False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    _compare(out["sub"].check(), o0, b, "eager with sizes")
    graph, dot = capture_with_dump(step)
    assert_no_memset_nodes(dot, "edge_subgraph")
    nodes = _graph_nodes(dot)
    if nodes is not None:
        print(f"captured edge_subgraph: {len(nodes)} graph nodes")
        assert len(nodes) <= 6 + 4, (sorted(nodes), dot[:3000])                       # x, node_label, edge_attr, edge_label ride along
    mask.copy_(torch.from_numpy(m1).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    _compare(out["sub"].check(), o1, b, "replay on the refilled mask")
    mask.copy_(torch.from_numpy(np.ones(b.num_edges, bool)).to(dev))                       # other counts: reported, not obeyed
    graph.replay()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        out["sub"].check()
    assert out["sub"].counts.tolist()[:3] == [b.num_nodes - int((np.bincount(b.edge_index.numpy().reshape(-1), minlength=b.num_nodes) == 0).sum()),
                                              b.num_edges, 1]
    with monkeypatch.context() as mp:                                                      # nor inside a capture
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(ValueError):
            G.edge_subgraph(d, mask)
    assert S.subgraph_block_items() == B


GUARD = 16


def _raw_call(dev, d, keep, mode, drop, cap_n, cap_e, bufs=None):
    """gsat_subgraph_index itself (phases 3, exact) on outputs that carry GUARD sentinel elements behind their capacity."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.graph_index import call_size, get_index
    N, E = d.num_nodes, d.num_edges
    seg = get_index(d.edge_index, N).graphs(d.batch, d.num_graphs)
    if bufs is None:
        ws_bytes = call_size("gsat_subgraph_workspace_bytes", N, E)
        bufs = dict(node_id=torch.full((cap_n + GUARD,), -7, dtype=torch.int64, device=dev),
                    edge_id=torch.full((cap_e + GUARD,), -7, dtype=torch.int64, device=dev),
                    new_ei=torch.full((2 * cap_e + GUARD,), -7, dtype=torch.int64, device=dev),
                    new_batch=torch.full((cap_n + GUARD,), -7, dtype=torch.int64, device=dev),
                    new_ptr=torch.full((d.num_graphs + 1 + GUARD,), -7, dtype=torch.int32, device=dev),
                    edge_mask=torch.full((E + GUARD,), 7, dtype=torch.uint8, device=dev),
                    counts=torch.full((4 + GUARD,), -7, dtype=torch.int64, device=dev),
                    ws=torch.empty(ws_bytes, dtype=torch.uint8, device=dev), ws_bytes=ws_bytes)
    call("gsat_subgraph_index", ptr(d.edge_index), E, N, ptr(d.batch), ptr(seg.node_ptr), d.num_graphs, ptr(keep), mode, int(drop), 3,
         cap_n, cap_e, 1, ptr(bufs["node_id"]), ptr(bufs["edge_id"]), ptr(bufs["new_ei"]), ptr(bufs["new_batch"]), ptr(bufs["new_ptr"]),
         ptr(bufs["edge_mask"]), ptr(bufs["counts"]), ptr(bufs["ws"]), bufs["ws_bytes"], stream())
    return bufs


def _guards_intact(bufs, cap_n, cap_e, E, G):
    for name, used, val in (("node_id", cap_n, -7), ("edge_id", cap_e, -7), ("new_ei", 2 * cap_e, -7), ("new_batch", cap_n, -7),
                            ("new_ptr", G + 1, -7), ("edge_mask", E, 7), ("counts", 4, -7)):
        tail = bufs[name][used:].cpu().numpy()
        assert len(tail) == GUARD and (tail == val).all(), name


@pytest.mark.parametrize("mode,drop", [(0, 1), (0, 0), (1, 0)])
def test_wrong_capacities_set_the_flag_and_write_nothing_out_of_bounds(dev, mode, drop):
    """Captured with capacities that are right for one mask, replayed on masks that keep more and fewer: the overflow flag is set, the
    entries below the capacity are the oracle's first ones (or valid filler behind a smaller count), the guard elements behind every
    output are untouched."""
    import dp_gsat_amd as G
    G.clear_cache()
    B = _block()
    b = _sized(2 * B + 1, B + 1, seed=33)
    d = b.to(dev)
    n = b.num_nodes if mode == 1 else b.num_edges
    rng = np.random.RandomState(mode * 2 + drop)
    k0, more, fewer = rng.rand(n) < 0.5, rng.rand(n) < 0.8, rng.rand(n) < 0.2
    ptr = so.node_ptr_of(b.batch.numpy(), b.num_graphs)
    orc = lambda k: so.subgraph_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), ptr, k, "node" if mode else "edge", bool(drop))
    cap_n, cap_e = orc(k0)["counts"]
    keep = torch.from_numpy(k0).to(dev).view(torch.uint8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bufs = _raw_call(dev, d, keep, mode, drop, cap_n, cap_e)
    torch.cuda.current_stream().wait_stream(side)
    graph, dot = capture_with_dump(lambda: _raw_call(dev, d, keep, mode, drop, cap_n, cap_e, bufs))
    assert_no_memset_nodes(dot, "gsat_subgraph_index")
    nodes = _graph_nodes(dot)
    if nodes is not None:
        assert len(nodes) <= (6 if (mode == 0 and drop) else 4), (sorted(nodes), dot[:3000])
    for k, over in ((k0, 0), (more, 1), (fewer, 1), (k0, 0)):
        o = orc(k)
        keep.copy_(torch.from_numpy(k).to(dev).view(torch.uint8))
        graph.replay()
        torch.cuda.synchronize()
        assert bufs["counts"][:4].tolist() == [o["counts"][0], o["counts"][1], over, 0]
        _guards_intact(bufs, cap_n, cap_e, b.num_edges, b.num_graphs)
        wn, we = min(cap_n, o["counts"][0]), min(cap_e, o["counts"][1])
        assert np.array_equal(bufs["node_id"][:wn].cpu().numpy(), o["node_id"][:wn])
        assert np.array_equal(bufs["edge_id"][:we].cpu().numpy(), o["edge_id"][:we])
        assert np.array_equal(bufs["new_batch"][:wn].cpu().numpy(), o["batch"][:wn])
        assert np.array_equal(bufs["new_ei"][:2 * cap_e].view(2, cap_e)[:, :we].cpu().numpy(), o["edge_index"][:, :we])
        assert np.array_equal(bufs["edge_mask"][:b.num_edges].cpu().numpy(), o["edge_mask"])
        assert np.array_equal(bufs["new_ptr"][:b.num_graphs + 1].cpu().numpy(), o["node_ptr"])
        assert (bufs["node_id"][wn:cap_n] == 0).all() and (bufs["edge_id"][we:cap_e] == 0).all()      # valid filler, never garbage


def test_bad_node_ids_are_flagged_and_never_dereferenced(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import call, ptr, stream
    G.clear_cache()
    b = _sized(65, 65, seed=35)
    d = b.to(dev)
    seg = G.get_index(d.edge_index, 65).graphs(d.batch, d.num_graphs)             # node_ptr comes from the intact batch
    keep = torch.ones(65, dtype=torch.uint8, device=dev)
    bufs = _raw_call(dev, d, keep, 0, 1, 65, 65)
    assert bufs["counts"][:4].tolist()[3] == 0
    for bad_value in (65, -1, 1 << 40):
        ei = d.edge_index.clone()
        ei[1, 17] = bad_value
        call("gsat_subgraph_index", ptr(ei), 65, 65, ptr(d.batch), ptr(seg.node_ptr), d.num_graphs, ptr(keep), 0, 1, 3, 65, 65, 0,
             ptr(bufs["node_id"]), ptr(bufs["edge_id"]), ptr(bufs["new_ei"]), ptr(bufs["new_batch"]), ptr(bufs["new_ptr"]),
             ptr(bufs["edge_mask"]), ptr(bufs["counts"]), ptr(bufs["ws"]), bufs["ws_bytes"], stream())
        c = bufs["counts"][:4].tolist()
        assert c[1] == 64 and c[2] == 0 and c[3] == 1, (bad_value, c)
        assert bufs["edge_mask"][17].item() == 0 and int(bufs["edge_mask"][:65].sum()) == 64
        _guards_intact(bufs, 65, 65, 65, d.num_graphs)
    with pytest.raises(ValueError):                                                # the public call reports it
        from dp_gsat_amd.synth import Batch
        G.edge_subgraph(Batch(x=d.x, edge_index=ei, batch=d.batch, num_graphs=d.num_graphs), keep)


def test_two_calls_give_identical_bytes(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    p = synth.molhiv_batch(256, seed=6)
    d = p.to(dev)
    a = torch.from_numpy(_att(p.num_edges, 60)).to(dev)
    runs = [G.explanation_subgraph(a, d, ratio=0.5) for _ in range(2)]
    runs += [G.node_subgraph(d, torch.arange(p.num_nodes, device=dev) % 3 != 0) for _ in range(2)]
    for first, second in (runs[:2], runs[2:]):
        for name in ("x", "edge_index", "batch", "node_id", "edge_id", "edge_mask", "node_ptr", "counts"):
            x, y = getattr(first, name), getattr(second, name)
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x, y.view(torch.uint8) if y.dtype == torch.bool else y), name
    assert torch.equal(runs[0].edge_att, runs[1].edge_att)
