"""gpu: the stacked batch of a fidelity curve (gsat_fidelity_stack, dp_gsat_amd.explanation_stack) bit for bit against the unchanged
``edge_subgraph_padded`` variant by variant and against tests/fidelity_stack_oracle.py -- unpadded, padded, ragged and overflowed inputs,
edge counts around the workgroup's items so that the scan across workgroups runs --, guard elements around every output, determinism,
a capture that holds kernel nodes only, and the backbones on the stack against the per-variant padded forwards."""
import ctypes
import os
import tempfile
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import fidelity_stack_oracle as fso
from tests import padded_oracle as po
from tests import train_log as tl
from tests.test_gpu_padded_subgraph import _as_padded
from tests.test_gpu_subgraph import _batch, _models, _sized
from tests.util import assert_no_memset_nodes, close

pytestmark = pytest.mark.gpu
GUARD = 64


def _block():
    from dp_gsat_amd import subgraph as S
    return S.fidelity_stack_block_items()


def _input(kind, E, seed=11):
    """A host batch with exactly E real edges: an unpadded Batch, a PaddedBatch with slack, a ragged one with three empty trailing graph
    slots, or a PaddedBatch whose overflow word is set."""
    N = int(E * 0.7) + 20
    b = _sized(N, E, seed=seed)
    if kind == "unpadded":
        return b
    if kind == "ragged":
        p = _as_padded(_batch(b.edge_index.numpy(), b.batch.numpy(), b.num_graphs + 3), (N + 4, E + 6), graphs=b.num_graphs)
        p.ragged = True
        return p
    return _as_padded(b, (N + 9, E + 13), overflow=int(kind == "overflowed"))


def _stack(dev, d, **kw):
    import dp_gsat_amd as G
    G.set_sync_free(True)               # nothing read back: an overflow is a result here, not an exception
    try:
        return G.explanation_stack(d, **kw)
    finally:
        G.set_sync_free(False)


def _reference_variant(dev, d, mask, cap):
    import dp_gsat_amd as G
    G.set_sync_free(True)
    try:
        return G.edge_subgraph_padded(d, mask, cap, drop_isolated=False)
    finally:
        G.set_sync_free(False)


def _check_against_the_extractions(dev, b, d, stack, what):
    """Every variant's segment, edge_id, valid word, batch rows, x rows and edge_attr rows equal ``edge_subgraph_padded``'s, shifted."""
    S, V, N_cap, Gp = len(stack.levels), stack.variants, stack.node_capacity, stack.graphs_per_variant
    padded = hasattr(b, "valid")
    assert V == 2 * S + 1 and Gp == b.num_graphs + (0 if padded else 1) and N_cap == b.num_nodes + (0 if padded else 2), what
    assert stack.num_graphs == V * Gp and stack.x.shape[0] == V * N_cap == stack.batch.shape[0], what
    off = stack.segment_offsets
    assert off[0] == 0 and stack.edge_index.shape == (2, off[-1]) and stack.edge_id.shape == (off[-1],), what
    lv = stack.edge_level
    masks = [torch.ones_like(lv, dtype=torch.bool)] + [lv <= s for s in range(S)] + [lv > s for s in range(S)]
    for v, mask in enumerate(masks):
        cap = (N_cap, off[v + 1] - off[v])
        sub = _reference_variant(dev, d, mask, cap)
        seg = slice(off[v], off[v + 1])
        assert torch.equal(stack.edge_index[:, seg], sub.edge_index + v * N_cap), (what, v, "edge_index")
        assert torch.equal(stack.edge_id[seg], sub.edge_id), (what, v, "edge_id")
        assert torch.equal(stack.valid[v], sub.valid), (what, v, stack.valid[v].tolist(), sub.valid.tolist())
        rows = slice(v * N_cap, (v + 1) * N_cap)
        assert torch.equal(stack.batch[rows], sub.batch + v * Gp), (what, v, "batch")
        if not int(sub.valid[3]):
            assert torch.equal(stack.x[rows], sub.x), (what, v, "x")
        assert torch.equal(stack.edge_attr[seg], sub.edge_attr), (what, v, "edge_attr")
    return masks


def _check_against_the_oracle(b, stack, what):
    valid_in = b.valid.tolist() if hasattr(b, "valid") else None
    real = b.num_graphs - (1 if valid_in is not None else 0)
    off = stack.segment_offsets
    caps = [off[v + 1] - off[v] for v in range(stack.variants)]
    o = fso.stack_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), real, stack.edge_level.cpu().numpy(), len(stack.levels), caps,
                         stack.node_capacity, valid_in, stack.graphs_per_variant)
    for name in ("edge_index", "edge_id", "batch"):
        assert np.array_equal(getattr(stack, name).cpu().numpy(), o[name]), (what, name)
    assert np.array_equal(stack.valid.cpu().numpy().astype(np.int64), o["valid"]) and list(off) == o["offsets"], what
    return o


@pytest.mark.parametrize("kind", ["unpadded", "padded", "ragged", "overflowed"])
@pytest.mark.parametrize("where", ["below", "at", "above", "two_blocks"])
def test_stack_equals_the_padded_extractions_variant_by_variant(dev, kind, where):
    import dp_gsat_amd as G
    G.clear_cache()
    blk = _block()
    E = {"below": blk - 1, "at": blk, "above": blk + 1, "two_blocks": 2 * blk + 1}[where]
    b = _input(kind, E)
    d = b.to(dev)
    att = torch.rand(b.num_edges, generator=torch.Generator().manual_seed(E)).to(dev)
    att[::5] = 0.5
    levels = {"below": dict(ks=[3]), "at": dict(ratios=[0.2, 0.5, 0.8]), "above": dict(ks=[1, 2, 7]),
              "two_blocks": dict(ratios=[(i + 1) / 16 for i in range(16)])}[where]
    what = f"{kind} E={E} {levels}"
    stack = _stack(dev, d, att=att, max_seg_edges=min(b.num_edges, 16384), **levels)
    _check_against_the_extractions(dev, b, d, stack, what)
    o = _check_against_the_oracle(b, stack, what)
    S = len(stack.levels)
    if kind == "overflowed":
        assert (stack.valid.cpu() == torch.tensor([0, 0, 0, 1], dtype=torch.int32)).all() and (stack.edge_id == -1).all(), what
    else:
        assert not o["valid"][:, 3].any() and int(o["valid"][0, 1]) == E and int(o["valid"][:, 1].sum()) == (S + 1) * E, what
        for s, l in enumerate(stack.levels):                                           # the levels are those of topk_edge_mask
            one = dict(ratio=l) if stack.by_ratio else dict(k=l)
            real = b.num_graphs - (1 if hasattr(b, "valid") else 0)
            want = G.topk_edge_mask(att, d.edge_index, d.batch, num_graphs=b.num_graphs, max_seg_edges=min(b.num_edges, 16384),
                                    ranked_graphs=real, **one)
            assert torch.equal((stack.edge_level <= s)[:E], want[:E]), (what, s)
    again = _stack(dev, d, att=att, max_seg_edges=min(b.num_edges, 16384), **levels)
    for name in ("edge_index", "edge_id", "batch", "valid", "x", "edge_attr", "edge_level"):
        assert torch.equal(getattr(stack, name), getattr(again, name)), (what, name)          # bitwise repeatable
    G.clear_cache()


def test_a_variant_that_does_not_fit_its_segment_overflows_alone_and_a_bad_id_spoils_all(dev):
    import dp_gsat_amd as G
    G.clear_cache()
    b = _input("padded", 300)
    d = b.to(dev)
    rng = np.random.RandomState(3)
    level = torch.from_numpy(rng.randint(0, 3, size=b.num_edges).astype(np.uint8)).to(dev)          # about a third per bin: far above k = 1
    stack = _stack(dev, d, att=None, ks=[1, 2], batch_size=2, edge_level=level)
    _check_against_the_extractions(dev, b, d, stack, "small keep segments")
    _check_against_the_oracle(b, stack, "small keep segments")
    assert stack.valid[:, 3].tolist() == [0, 1, 1, 0, 0]
    with pytest.raises(ValueError, match="does not fit"):
        G.explanation_stack(d, None, ks=[1, 2], batch_size=2, edge_level=level)       # eager: one host read reports it
    with pytest.raises(ValueError, match="does not fit"):
        stack.check()
    u = _input("unpadded", 300)
    u.edge_index[1, 17] = u.num_nodes + 1                                               # a node id out of range
    du = u.to(dev)
    stack = _stack(dev, du, att=None, ratios=[0.5], edge_level=level[:300].contiguous())
    _check_against_the_oracle(u, stack, "bad id")
    assert (stack.valid.cpu() == torch.tensor([0, 0, 0, 1], dtype=torch.int32)).all() and (stack.edge_id == -1).all()
    assert (stack.batch.view(3, -1) == (torch.arange(3, device=dev) * stack.graphs_per_variant + u.num_graphs).view(3, 1)).all()
    G.clear_cache()


def _raw_call(dev, d, level, S, Gp, N_cap, offsets, real, bufs=None):
    """gsat_fidelity_stack itself, into buffers with GUARD sentinel elements on both sides of every output."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.graph_index import call_size
    V, E_stack = 2 * S + 1, offsets[-1]
    E, N = int(d.edge_index.shape[1]), int(d.x.shape[0])
    if bufs is None:
        bufs = dict(ei=torch.full((2 * E_stack + 2 * GUARD,), -77, dtype=torch.int64, device=dev),
                    eid=torch.full((E_stack + 2 * GUARD,), -77, dtype=torch.int64, device=dev),
                    batch=torch.full((V * N_cap + 2 * GUARD,), -77, dtype=torch.int64, device=dev),
                    valid=torch.full((4 * V + 2 * GUARD,), -77, dtype=torch.int32, device=dev))
        ws_bytes = call_size("gsat_fidelity_stack_workspace_bytes", E, S)
        bufs["ws"] = torch.full((ws_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    inner = {k: t[GUARD:t.numel() - GUARD] for k, t in bufs.items()}
    valid_in = getattr(d, "valid", None)
    call("gsat_fidelity_stack", ptr(d.edge_index), E, N, ptr(d.batch), real, ptr(valid_in) if valid_in is not None else None, ptr(level), S,
         Gp, N_cap, (ctypes.c_int64 * (V + 1))(*offsets), ptr(inner["ei"]), ptr(inner["eid"]), ptr(inner["batch"]), ptr(inner["valid"]),
         ptr(inner["ws"]), inner["ws"].numel(), stream())
    return bufs, inner


@pytest.mark.parametrize("kind", ["unpadded", "ragged", "overflowed"])
def test_guards_stay_untouched_and_the_capture_holds_kernel_nodes_only(dev, kind):
    import dp_gsat_amd as G
    G.clear_cache()
    E = 2 * _block() + 1
    b = _input(kind, E)
    d = b.to(dev)
    att = torch.rand(b.num_edges, generator=torch.Generator().manual_seed(1)).to(dev)
    stack = _stack(dev, d, att=att, ratios=[0.1, 0.4, 0.9], max_seg_edges=min(b.num_edges, 16384))
    S, Gp, N_cap, off = 3, stack.graphs_per_variant, stack.node_capacity, list(stack.segment_offsets)
    real = b.num_graphs - (1 if hasattr(b, "valid") else 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bufs, inner = _raw_call(dev, d, stack.edge_level, S, Gp, N_cap, off, real)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    def verify(when):
        for name, t in bufs.items():
            sentinel = 0xA5 if name == "ws" else -77
            assert (t[:GUARD] == sentinel).all() and (t[-GUARD:] == sentinel).all(), (kind, when, name)
        assert torch.equal(inner["ei"].view(2, -1), stack.edge_index) and torch.equal(inner["eid"], stack.edge_id), (kind, when)
        assert torch.equal(inner["batch"], stack.batch) and torch.equal(inner["valid"].view(-1, 4), stack.valid), (kind, when)

    verify("eager")
    graph = tl.kept_debug_graph()
    assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
    for name in ("ei", "eid", "batch", "valid"):
        inner[name].fill_(-5)
    with torch.cuda.graph(graph):
        _raw_call(dev, d, stack.edge_level, S, Gp, N_cap, off, real, bufs)
    path = os.path.join(tempfile.mkdtemp(), "graph.dot")
    graph.debug_dump(path)
    dot = open(path, errors="replace").read()
    assert assert_no_memset_nodes(dot, "gsat_fidelity_stack") and "memcpy" not in dot.lower()
    nodes = tl.kernel_nodes(dot)
    assert nodes is not None, dot[:2000]
    assert len(nodes) == 4 and [n for k in ("k_stk_hist", "k_stk_scan", "k_stk_scatter", "k_stk_fill") for n in nodes if k in n] == nodes, nodes
    graph.replay()
    torch.cuda.synchronize()
    verify("replayed")
    G.clear_cache()


@pytest.mark.parametrize("backbone", ["GIN", "PNA"])
def test_one_forward_on_the_stack_equals_the_padded_forwards_variant_by_variant(dev, backbone):
    """The reference is the path ReplayedFidelity._forward takes today: ``clf`` on ``edge_subgraph_padded``'s batch inside ``padded()``.  The
    GEMM plan changes with the row count, so the comparison is tests.util.close's forward tolerance, not bitwise."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    from dp_gsat_amd.collate import PaddedBatch
    G.clear_cache()
    data = synth.ba2motifs_batch(num_graphs=12, seed=4)
    data.edge_attr = None
    _, clf = _models(dev, data, backbone)
    d = data.to(dev)
    N, E, B = data.num_nodes, data.num_edges, data.num_graphs
    cap = (N + 7, E + 10)
    lay = po.collate_padded([NS(x=data.x, edge_index=data.edge_index)], [0], cap)
    grow = lambda t, n: torch.cat([t, t.new_zeros((n - t.shape[0],) + tuple(t.shape[1:]))])
    pb = PaddedBatch(x=grow(data.x, cap[0]), edge_index=torch.from_numpy(lay["edge_index"]),
                     batch=torch.cat([data.batch, torch.full((cap[0] - N,), B, dtype=torch.int64)]), edge_attr=None, y=data.y,
                     num_graphs=B + 1, capacity=cap, valid=torch.tensor([N, E, B, 0], dtype=torch.int32)).to(dev)
    att = torch.rand(cap[1], generator=torch.Generator().manual_seed(9)).to(dev)
    for inp, name in ((pb, "padded"), (d, "unpadded")):
        a = att if inp is pb else att[:E].contiguous()
        with torch.no_grad():
            stack = G.explanation_stack(inp, a, ratios=[0.2, 0.5, 0.8], max_seg_edges=E)
            S, V, Gp, N_cap = 3, stack.variants, stack.graphs_per_variant, stack.node_capacity
            logits = clf(stack.x, stack.edge_index, stack.batch, None).view(V, Gp, -1)
            lv, off = stack.edge_level, stack.segment_offsets
            masks = [torch.ones_like(lv, dtype=torch.bool)] + [lv <= s for s in range(S)] + [lv > s for s in range(S)]
            for v, mask in enumerate(masks):
                sub = G.edge_subgraph_padded(inp, mask, (N_cap, off[v + 1] - off[v]))
                G.get_index(sub.edge_index, int(sub.x.shape[0])).graphs(sub.batch, int(sub.num_graphs))
                with G.padded(sub.valid, sub.capacity):
                    ref = clf(sub.x, sub.edge_index, sub.batch, None)
                assert ref.shape[0] == Gp
                close(logits[v, :B], ref[:B], what=f"{backbone} {name} variant {v}")
    G.clear_cache()
