"""gpu: the padded extraction (gsat_subgraph_padded, dp_gsat_amd.edge_subgraph_padded / node_subgraph_padded) byte for byte against
tests/padded_subgraph_oracle.py -- every mode on unpadded, padded and ragged inputs, at the sizes the kernels branch on --, its
overflow verdicts with guard bytes around every output, determinism, the unchanged unpadded functions, the backbones on the result,
and one captured extraction replayed on a refilled mask."""
import copy
import os
import tempfile
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import padded_oracle as po
from tests import padded_subgraph_oracle as pso
from tests import subgraph_oracle as so
from tests import train_log as tl
from tests.test_gpu_subgraph import _batch, _block, _differs, _models, _sized
from tests.util import assert_no_memset_nodes, close

pytestmark = pytest.mark.gpu
MODES = [("edge", False), ("edge", True), ("node", False)]
OUT = ("node_id", "edge_id", "edge_index", "batch", "edge_mask", "valid")


def _as_padded(b, cap, graphs=None, overflow=0):
    """The Batch ``b`` as the PaddedBatch ``collate_padded`` would make of it at capacity ``cap`` (host tensors): zero rows, the padding
    graph ``b.num_graphs`` and the padding edges of tests.padded_oracle."""
    from dp_gsat_amd.collate import PaddedBatch
    N, E, G = b.num_nodes, b.num_edges, b.num_graphs
    lay = po.collate_padded([NS(x=b.x, edge_index=b.edge_index)], [0], cap)
    assert lay["valid"].tolist() == [N, E, 1, 0]
    grow = lambda t, n: torch.cat([t, t.new_zeros((n - t.shape[0],) + tuple(t.shape[1:]))])
    return PaddedBatch(x=grow(b.x, cap[0]), edge_index=torch.from_numpy(lay["edge_index"]),
                       batch=torch.cat([b.batch, torch.full((cap[0] - N,), G, dtype=torch.int64)]), edge_attr=grow(b.edge_attr, cap[1]),
                       edge_label=grow(b.edge_label, cap[1]), node_label=grow(b.node_label, cap[0]), y=grow(b.y, G + 1),
                       num_graphs=G + 1, capacity=cap, valid=torch.tensor([N, E, G if graphs is None else graphs, overflow], dtype=torch.int32))


def _oracle(b, keep, mode, drop, cap):
    """The oracle on a host Batch / PaddedBatch; ``keep`` at the input's full shape."""
    valid = b.valid.tolist() if hasattr(b, "valid") else None
    real = b.num_graphs - (1 if valid is not None else 0)
    return pso.subgraph_padded_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), real, keep, mode, drop, cap, valid, pad_graph=real), real


def _compare(sub, o, b, real, cap, what):
    got = dict(node_id=sub.node_id, edge_id=sub.edge_id, edge_index=sub.edge_index, batch=sub.batch,
               edge_mask=sub.edge_mask.view(torch.uint8), valid=sub.valid.to(torch.int64))
    for name in OUT:
        g = got[name].cpu().numpy()
        assert g.dtype == o[name].dtype and g.shape == o[name].shape and np.array_equal(g, o[name]), (what, name)
    assert sub.capacity == tuple(cap) and sub.num_graphs == real + 1 and torch.equal(sub.y.cpu(), b.y), what
    nid, eid = torch.from_numpy(o["node_id"]), torch.from_numpy(o["edge_id"])
    for name, index in (("x", nid), ("node_label", nid), ("edge_attr", eid), ("edge_label", eid)):
        table = getattr(b, name)
        want = table[index.clamp(min=0)].clone()
        want[index < 0] = 0                                                            # zero rows in the padding
        assert torch.equal(getattr(sub, name).cpu(), want), (what, name)
    pso.check_invariants({k: got[k].cpu().numpy() for k in ("node_id", "edge_id", "edge_index", "batch", "valid")}, cap, real)


def _extract(dev, d, keep, mode, drop, cap):
    import dp_gsat_amd as G
    k = torch.from_numpy(np.ascontiguousarray(keep)).to(dev)
    G.set_sync_free(True)               # nothing read back: an overflow is a result here, not an exception
    try:
        return G.edge_subgraph_padded(d, k, cap, drop_isolated=drop) if mode == "edge" else G.node_subgraph_padded(d, k, cap)
    finally:
        G.set_sync_free(False)


def _check(dev, b, d, keep, mode, drop, cap, what):
    o, real = _oracle(b, keep, mode, drop, cap)
    sub = _extract(dev, d, keep, mode, drop, cap)
    _compare(sub, o, b, real, cap, f"{what} mode={mode} drop={drop} cap={cap}")
    return sub, o


def _with_garbage(keep, b, mode, seed):
    """``keep`` over the counted items, grown to the input's full shape with random bytes behind the counts."""
    full = b.num_edges if mode == "edge" else b.num_nodes
    tail = np.random.RandomState(seed).randint(0, 256, size=full - len(keep)).astype(np.uint8)
    return np.concatenate([keep.astype(np.uint8), tail])


def _inputs(kind):
    """(host batch, counted nodes, counted edges) of the three input kinds, all made from one random batch."""
    b = _sized(150, 260, seed=11)
    if kind == "unpadded":
        return b, 150, 260
    if kind == "padded":
        return _as_padded(b, (150 + 9, 260 + 13)), 150, 260
    slots = _batch(b.edge_index.numpy(), b.batch.numpy(), b.num_graphs + 3)           # ragged: three empty slots behind the graphs
    p = _as_padded(slots, (150 + 4, 260 + 6), graphs=b.num_graphs)
    p.ragged = True
    return p, 150, 260


@pytest.mark.parametrize("mode,drop", MODES)
@pytest.mark.parametrize("kind", ["unpadded", "padded", "ragged"])
def test_padded_extraction_equals_the_oracle(dev, kind, mode, drop):
    """Every keep pattern at four capacities: n_pad = 2 with E' = E_out_cap (no padding edge), an odd and an even e_pad, and a wide one."""
    b, Nv, Ev = _inputs(kind)
    d = b.to(dev)
    n = Ev if mode == "edge" else Nv
    rng = np.random.RandomState(7)
    pats = {"random": rng.rand(n) < 0.5, "all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0}
    for name, keep in pats.items():
        full = _with_garbage(keep, b, mode, 3)
        ref, _ = _oracle(b, full, mode, drop, (b.num_nodes + 2, b.num_edges))
        n_out, e_out = int(ref["valid"][0]), int(ref["valid"][1])
        for cap in [(n_out + 2, e_out), (n_out + 2, e_out + 7), (n_out + 3, e_out + 8), (n_out + 40, e_out + 5)]:
            sub, o = _check(dev, b, d, full, mode, drop, cap, f"{kind} {name}")
            assert o["valid"].tolist()[3] == 0 and o["valid"].tolist()[:2] == [n_out, e_out]
            if kind == "ragged":
                assert sub.ragged is True and int(sub.valid[2]) == b.num_graphs - 4
    if kind != "unpadded" and mode == "edge" and not drop:                             # at the input's own row count the nodes are shared
        sub = _extract(dev, d, _with_garbage(pats["random"], b, mode, 3), mode, drop, (b.num_nodes, Ev))
        assert sub.x.data_ptr() == d.x.data_ptr() and sub.batch.data_ptr() == d.batch.data_ptr()
        assert sub.valid.tolist() == [Nv, int(pats["random"].sum()), int(b.valid[2]), 0]


@pytest.mark.parametrize("padded_input", [False, True])
@pytest.mark.parametrize("case", range(6))
def test_counts_and_input_sizes_at_the_workgroup_boundaries(dev, case, padded_input):
    """Cases 0-2: inputs of B - 1, B, B + 1 nodes and edges (B = gsat_subgraph_block_items()), random masks, every mode.  Cases 3-5: an
    input of two workgroups and more whose extraction KEEPS B - 1, B, B + 1 nodes (node mode) and edges (edge mode)."""
    B = _block()
    delta = case % 3 - 1
    if case < 3:
        b = _sized(B + delta, B + delta, seed=40 + case)
    else:
        b = _sized(2 * B + 1, B + 70, seed=40 + case)
    Nv, Ev = b.num_nodes, b.num_edges
    if padded_input:
        b = _as_padded(b, (Nv + 2 + case, Ev + case))
    d = b.to(dev)
    rng = np.random.RandomState(case)
    for mode, drop in MODES:
        n = Ev if mode == "edge" else Nv
        if case < 3:
            keep = rng.rand(n) < 0.6
        else:                                    # exactly B + delta kept, spread over both workgroups
            keep = np.zeros(n, bool)
            keep[rng.permutation(n)[:B + delta]] = True
        full = _with_garbage(keep, b, mode, case)
        ref, _ = _oracle(b, full, mode, drop, (b.num_nodes + 2, b.num_edges))
        n_out, e_out = int(ref["valid"][0]), int(ref["valid"][1])
        if case >= 3:
            assert (e_out if mode == "edge" else n_out) == B + delta
        _check(dev, b, d, full, mode, drop, (n_out + 2, e_out + 1), f"case {case}")


GUARD = 16


def _raw(dev, d, keep, mode, drop, cap, valid_in, real, bufs=None):
    """gsat_subgraph_padded itself on outputs with GUARD sentinel elements in front of and behind every one of them."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.graph_index import call_size
    N, E = d.num_nodes, d.num_edges
    if bufs is None:
        ws_bytes = call_size("gsat_subgraph_workspace_bytes", N, E)
        nan = torch.tensor(float("nan")).view(torch.int32).item()
        sizes = dict(node_id=cap[0], edge_id=cap[1], new_ei=2 * cap[1], new_batch=cap[0], edge_mask=E, valid=4)
        dtypes = dict(edge_mask=torch.uint8, valid=torch.int32)
        fill = dict(edge_mask=0xA5, valid=nan)                                         # a byte pattern, and NaN's bit pattern
        bufs = {k: torch.full((n + 2 * GUARD,), fill.get(k, -7), dtype=dtypes.get(k, torch.int64), device=dev) for k, n in sizes.items()}
        bufs.update(ws=torch.empty(ws_bytes, dtype=torch.uint8, device=dev), ws_bytes=ws_bytes, sizes=sizes, fill=fill)
    inner = lambda k: bufs[k][GUARD:]
    call("gsat_subgraph_padded", ptr(d.edge_index), E, N, ptr(d.batch), real, ptr(keep), 0 if mode == "edge" else 1, int(drop),
         ptr(valid_in) if valid_in is not None else None, real, cap[0], cap[1], ptr(inner("node_id")), ptr(inner("edge_id")),
         ptr(inner("new_ei")), ptr(inner("new_batch")), ptr(inner("edge_mask")), ptr(inner("valid")), ptr(bufs["ws"]), bufs["ws_bytes"],
         stream())
    return bufs


def _guards_intact(bufs):
    for name, used in bufs["sizes"].items():
        t = bufs[name].cpu().numpy()
        want = bufs["fill"].get(name, -7)
        assert (t[:GUARD] == want).all() and (t[GUARD + used:] == want).all() and len(t[GUARD + used:]) == GUARD, name


def _raw_equals(bufs, o, cap):
    inner = lambda k: bufs[k][GUARD:GUARD + bufs["sizes"][k]].cpu().numpy()
    assert inner("valid").tolist() == o["valid"].tolist()
    assert np.array_equal(inner("node_id"), o["node_id"]) and np.array_equal(inner("edge_id"), o["edge_id"])
    assert np.array_equal(inner("new_batch"), o["batch"]) and np.array_equal(inner("new_ei").reshape(2, cap[1]), o["edge_index"])
    assert np.array_equal(inner("edge_mask"), o["edge_mask"])


@pytest.mark.parametrize("mode,drop", MODES)
def test_overflow_is_all_padding_and_nothing_is_written_out_of_bounds(dev, mode, drop):
    """N' + 2 = N_out_cap + 1, E' = E_out_cap + 1, an input whose valid[3] is set, a bad node id: valid_out == (0, 0, 0, 1), the
    all-padding layout of the oracle, and the guard elements around every output untouched -- also in the cases that fit."""
    B = _block()
    b = _sized(B + 70, B + 1, seed=51)
    rng = np.random.RandomState(5)
    n = b.num_edges if mode == "edge" else b.num_nodes
    keep = rng.rand(n) < 0.7
    ref, real = _oracle(b, keep, mode, drop, (b.num_nodes + 2, b.num_edges))
    n_out, e_out = int(ref["valid"][0]), int(ref["valid"][1])
    assert e_out > 0
    d = b.to(dev)
    k = torch.from_numpy(keep).to(dev).view(torch.uint8)
    for cap, over in (((n_out + 2, e_out), 0), ((n_out + 1, e_out), 1), ((n_out + 2, e_out - 1), 1), ((2, 0), 1)):
        o, _ = _oracle(b, keep, mode, drop, cap)
        assert o["valid"].tolist() == ([0, 0, 0, 1] if over else [n_out, e_out, real, 0])
        bufs = _raw(dev, d, k, mode, drop, cap, None, real)
        _raw_equals(bufs, o, cap)
        _guards_intact(bufs)
    # a padded input that had itself overflowed: nothing of it is counted
    cap = (b.num_nodes + 5, b.num_edges + 3)
    p = _as_padded(b, cap, overflow=1)
    full = _with_garbage(keep, p, mode, 9)
    o, real_p = _oracle(p, full, mode, drop, cap)
    assert o["valid"].tolist() == [0, 0, 0, 1] and not o["edge_mask"].any()
    pd = p.to(dev)
    bufs = _raw(dev, pd, torch.from_numpy(full).to(dev), mode, drop, cap, pd.valid, real_p)
    _raw_equals(bufs, o, cap)
    _guards_intact(bufs)
    # bad node ids, never dereferenced: past the nodes, negative, huge
    for bad_value in (b.num_nodes, -1, 1 << 40):
        ei = b.edge_index.clone()
        ei[1, 17] = bad_value
        bb = _batch(ei.numpy(), b.batch.numpy(), b.num_graphs)
        cap = (b.num_nodes + 2, b.num_edges)
        o, _ = _oracle(bb, np.ones(n, bool), mode, drop, cap)
        assert o["valid"].tolist() == [0, 0, 0, 1] and o["edge_mask"][17] == 0
        bufs = _raw(dev, bb.to(dev), torch.ones(n, dtype=torch.uint8, device=dev), mode, drop, cap, None, real)
        _raw_equals(bufs, o, cap)
        _guards_intact(bufs)


def test_the_public_call_raises_on_overflow_and_reads_nothing_in_sync_free_mode(dev):
    import dp_gsat_amd as G
    b = _sized(65, 65, seed=35)
    d = b.to(dev)
    keep = torch.ones(65, dtype=torch.bool, device=dev)
    assert G.edge_subgraph_padded(d, keep, (67, 65)).check().valid.tolist() == [65, 65, b.num_graphs, 0]
    for cap in ((66, 65), (67, 64)):
        with pytest.raises(ValueError, match="does not fit"):
            G.edge_subgraph_padded(d, keep, cap)
        G.set_sync_free(True)
        try:
            sub = G.edge_subgraph_padded(d, keep, cap)
        finally:
            G.set_sync_free(False)
        assert sub.valid.tolist() == [0, 0, 0, 1] and not sub.x.any() and not sub.edge_attr.any()
        with pytest.raises(ValueError):
            sub.check()


def test_two_calls_give_identical_bytes_and_the_unpadded_functions_are_unchanged(dev):
    """Determinism of the padded extraction; and ``edge_subgraph`` / ``node_subgraph``, which share the flag pass, still give the bytes
    the unpadded oracle gives -- the real part of the padded result is the unpadded result."""
    import dp_gsat_amd as G
    b = _sized(_block() + 70, _block() + 1, seed=61)
    d = b.to(dev)
    rng = np.random.RandomState(6)
    for mode, drop in MODES:
        n = b.num_edges if mode == "edge" else b.num_nodes
        keep = rng.rand(n) < 0.5
        k = torch.from_numpy(keep).to(dev)
        plain = G.edge_subgraph(d, k, drop_isolated=drop) if mode == "edge" else G.node_subgraph(d, k)
        o = so.subgraph_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), so.node_ptr_of(b.batch.numpy(), b.num_graphs), keep, mode, drop)
        for name, got in (("node_id", plain.node_id), ("edge_id", plain.edge_id), ("edge_index", plain.edge_index), ("batch", plain.batch),
                          ("node_ptr", plain.node_ptr), ("edge_mask", plain.edge_mask.view(torch.uint8))):
            assert np.array_equal(got.cpu().numpy(), o[name]), (mode, drop, name)
        n_out, e_out = o["counts"]
        cap = (n_out + 6, e_out + 11)
        first, second = (_extract(dev, d, keep, mode, drop, cap) for _ in range(2))
        for name in ("x", "edge_index", "batch", "node_id", "edge_id", "valid", "edge_attr", "edge_label", "node_label"):
            assert torch.equal(getattr(first, name), getattr(second, name)), name
        assert torch.equal(first.edge_mask, second.edge_mask) and torch.equal(first.edge_mask, plain.edge_mask)
        assert torch.equal(first.node_id[:n_out], plain.node_id) and torch.equal(first.edge_index[:, :e_out], plain.edge_index)
        assert torch.equal(first.x[:n_out], plain.x) and torch.equal(first.edge_attr[:e_out], plain.edge_attr)


@pytest.mark.parametrize("backbone", ["GIN", "PNA"])
def test_backbone_on_the_padded_extraction(dev, backbone):
    """Eval-mode GIN and PNA (2 layers, hidden 32) inside padded() on the padded extraction, rows [:b]: the fp64-checked oracle model on the
    oracle-extracted graph, and the same backbone on the unpadded edge_subgraph.  PNA with a hard 0/1 mask still differs."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    data = synth.ba2motifs_batch(num_graphs=12, seed=6)
    d = data.to(dev)
    keep = np.random.RandomState(1).rand(data.num_edges) < 0.6
    m = torch.from_numpy(keep).to(dev)
    oclf, clf = _models(dev, data, backbone, H=32)
    ob, o = so.extract_batch(data, keep, "edge", False)
    cap = (data.num_nodes + 5, int(keep.sum()) + 9)
    sub = G.edge_subgraph_padded(d, m, cap)
    plain = G.edge_subgraph(d, m, drop_isolated=False)
    with torch.no_grad():
        G.get_index(sub.edge_index, cap[0]).graphs(sub.batch, sub.num_graphs)
        with G.padded(sub.valid, sub.capacity):
            got = clf(sub.x, sub.edge_index, sub.batch, None)
        same = clf(plain.x, plain.edge_index, plain.batch, None)
        ref = oclf(ob.x, ob.edge_index, ob.batch, None)
        ref64 = copy.deepcopy(oclf).double()(ob.x.double(), ob.edge_index, ob.batch, None)
        masked = clf(d.x, d.edge_index, d.batch, None, edge_atten=m.float().view(-1, 1))
    assert got.shape == (13, 1) and torch.isfinite(got).all()
    close(got[:12], ref, ref64=ref64, what=f"{backbone} padded extraction vs oracle")
    close(got[:12], same, what=f"{backbone} padded vs unpadded extraction")
    if backbone == "PNA":
        assert _differs(got[:12], masked)


def test_capture_once_and_replay_on_a_mask_with_another_count(dev):
    import dp_gsat_amd as G
    G.clear_cache()
    B = _block()
    b = _as_padded(_sized(B + 70, B + 1, seed=31), (B + 80, B + 9))
    d = b.to(dev)
    Ev = int(b.valid[1])
    rng = np.random.RandomState(2)
    m0 = _with_garbage(rng.rand(Ev) < 0.5, b, "edge", 1)
    m1 = _with_garbage(rng.rand(Ev) < 0.2, b, "edge", 2)
    cap = (b.num_nodes, Ev)
    o0, real = _oracle(b, m0, "edge", True, cap)
    o1, _ = _oracle(b, m1, "edge", True, cap)
    assert o0["valid"].tolist()[:2] != o1["valid"].tolist()[:2] and o0["valid"][3] == o1["valid"][3] == 0
    mask = torch.from_numpy(m0).to(dev)
    out = {}

    def step():
        out["sub"] = G.edge_subgraph_padded(d, mask, cap, drop_isolated=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    _compare(out["sub"], o0, b, real, cap, "eager")
    graph = tl.kept_debug_graph()                                                       # a default CUDAGraph gives its hipGraph up: no dump
    assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
    with torch.cuda.graph(graph):
        step()                                                                          # no size is declared and none is read
    path = os.path.join(tempfile.mkdtemp(), "graph.dot")
    graph.debug_dump(path)
    dot = open(path, errors="replace").read()
    assert assert_no_memset_nodes(dot, "edge_subgraph_padded")
    nodes = tl.kernel_nodes(dot)
    assert nodes is not None, dot[:2000]
    mine = [n for n in tl.library_kernels(nodes) if "k_sub" in n]
    assert len(mine) == 7 and "k_subp_fill" in mine[-1] and sum("k_subp_flags" in n for n in mine) == 2, mine      # clear, 2 x flags, scan, 2 x out, fill
    mask.copy_(torch.from_numpy(m1).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    _compare(out["sub"], o1, b, real, cap, "replay on the refilled mask")
    eager = G.edge_subgraph_padded(d, mask, cap, drop_isolated=True)
    for name in ("x", "edge_index", "batch", "node_id", "edge_id", "valid", "edge_attr", "edge_label", "node_label"):
        assert torch.equal(getattr(eager, name), getattr(out["sub"], name)), name
