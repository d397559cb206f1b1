"""gpu: the node-induced stack of a fidelity curve (gsat_fidelity_stack_nodes, dp_gsat_amd.explanation_stack_nodes) bit for bit against
tests/node_stack_oracle.py and against 2 S + 1 calls of the unchanged ``node_subgraph_padded`` -- unpadded, padded and ragged inputs whose
nodes and edges both span several workgroups, garbage behind the valid counts, guard elements around every output, the four overflow
cases, repeatability, and a capture replayed after the levels changed in place."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import node_stack_oracle as nso
from tests import train_log as tl
from tests.test_gpu_padded_subgraph import _as_padded
from tests.test_gpu_subgraph import _batch
from tests.util import assert_no_memset_nodes

pytestmark = pytest.mark.gpu
GUARD = 64
OUT = ("edge_index", "edge_id", "node_id", "batch", "valid")


def _block():
    from dp_gsat_amd import subgraph as S
    return S.fidelity_stack_block_items()


def _host_batch(seed=5, extra_graphs=0):
    """blk + 37 nodes and more than twice as many edges, neither a multiple of a workgroup's share: graph 0 is a single node without
    edges, the last two nodes of every larger graph are isolated, edges are drawn with replacement inside a graph (self loops and
    duplicates happen; one of each is forced)."""
    rng = np.random.RandomState(seed)
    N = _block() + 37
    sizes = [1, 40, 30, 64, 65, 300, 7, 2]
    sizes.append(N - sum(sizes))
    assert sizes[-1] > 4
    batch = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])
    E = 2 * N + 301
    big = [g for g, n in enumerate(sizes) if n >= 4]
    g = rng.choice(big, size=E, p=np.array([sizes[i] for i in big]) / sum(sizes[i] for i in big))
    span = np.array(sizes)[g] - 2
    ei = np.stack([start[g] + rng.randint(0, 1 << 30, size=E) % span, start[g] + rng.randint(0, 1 << 30, size=E) % span]).astype(np.int64)
    ei[:, 5] = ei[:, 4]                                                                # a duplicate edge
    ei[1, 7] = ei[0, 7]                                                                # a self loop
    return _batch(ei, batch, len(sizes) + extra_graphs), sizes, start


def _levels(b, sizes, start, S, seed=1):
    """uint8[N] over 0 .. S + 1 (S + 1 counts as S); graph 1 is swallowed whole by every keep level, graph 2 is emptied by the first."""
    lv = np.random.RandomState(seed).randint(0, S + 2, size=b.num_nodes).astype(np.uint8)
    lv[start[1]:start[2]] = 0
    lv[start[2]:start[3]] = np.maximum(lv[start[2]:start[3]], 1)
    return lv


def _input(kind, S):
    """(host batch, uint8 levels at its full shape)."""
    b, sizes, start = _host_batch(extra_graphs=3 if kind == "ragged" else 0)
    lv = _levels(b, sizes, start, S)
    if kind == "unpadded":
        return b, lv
    N, E, G = b.num_nodes, b.num_edges, len(sizes)
    p = _as_padded(b, (N + 9, E + 13), graphs=G if kind == "ragged" else None, overflow=int(kind == "spoiled"))
    if kind == "ragged":
        p.ragged = True
    # behind the valid counts: level bytes 0 and 255 and edge_index words out of range, none of which may ever matter
    lv = np.concatenate([lv, np.array([0, 255] * 5, np.uint8)[:9]])
    p.edge_index[:, E:] = torch.tensor([[10 ** 9], [-5]])
    return p, lv


def _real(b):
    return b.num_graphs - (1 if hasattr(b, "valid") else 0)


def _raw_call(dev, d, level, S, Gp, N_cap, offsets, real, bufs=None, cap_nodes_arg=None):
    """gsat_fidelity_stack_nodes itself, into buffers with GUARD sentinel elements on both sides of every output."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.graph_index import call_size
    V, E_stack = 2 * S + 1, offsets[-1]
    E, N = int(d.edge_index.shape[1]), int(d.x.shape[0])
    if bufs is None:
        mk = lambda n, dt=torch.int64: torch.full((n + 2 * GUARD,), -77, dtype=dt, device=dev)
        bufs = dict(edge_index=mk(2 * E_stack), edge_id=mk(E_stack), node_id=mk(V * N_cap), batch=mk(V * N_cap), valid=mk(4 * V, torch.int32))
        ws_bytes = call_size("gsat_fidelity_stack_nodes_workspace_bytes", N, E, S)
        bufs["ws"] = torch.full((ws_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    inner = {k: t[GUARD:t.numel() - GUARD] for k, t in bufs.items()}
    valid_in = getattr(d, "valid", None)
    call("gsat_fidelity_stack_nodes", ptr(d.edge_index), E, N, ptr(d.batch), real, ptr(valid_in) if valid_in is not None else None, ptr(level),
         S, Gp, N_cap if cap_nodes_arg is None else cap_nodes_arg, (ctypes.c_int64 * (V + 1))(*offsets), ptr(inner["edge_index"]), ptr(inner["edge_id"]), ptr(inner["node_id"]),
         ptr(inner["batch"]), ptr(inner["valid"]), ptr(inner["ws"]), inner["ws"].numel(), stream())
    return bufs, inner


def _guards_intact(bufs, what):
    for name, t in bufs.items():
        sentinel = 0xA5 if name == "ws" else -77
        assert (t[:GUARD] == sentinel).all() and (t[-GUARD:] == sentinel).all(), (what, name)


def _equals_oracle(inner, o, what):
    for name in OUT:
        got = inner[name].cpu().numpy().astype(np.int64).reshape(o[name].shape)
        assert np.array_equal(got, o[name]), (what, name, np.nonzero(got != o[name]))


def _oracle(b, lv, S, caps, N_cap, Gp):
    valid_in = b.valid.tolist() if hasattr(b, "valid") else None
    return nso.node_stack_oracle(b.edge_index.numpy(), b.num_nodes, b.batch.numpy(), _real(b), lv, S, caps, N_cap, valid_in, Gp)


def _padded_call(G, fn, *a, **kw):
    G.set_sync_free(True)               # nothing read back: an overflow is a result here, not an exception
    try:
        return fn(*a, **kw)
    finally:
        G.set_sync_free(False)


def _equals_the_extractions(G, d, level, stack, what):
    """Every variant equals ``node_subgraph_padded`` on its mask at (node_capacity, segment length), shifted; x, node_label and edge_attr
    are gathered by the ids."""
    S, V, N_cap, Gp, off = len(stack.levels), stack.variants, stack.node_capacity, stack.graphs_per_variant, stack.segment_offsets
    lv = level.clamp(max=S)
    masks = [torch.ones_like(lv, dtype=torch.bool)] + [lv <= s for s in range(S)] + [lv > s for s in range(S)]
    for v, mask in enumerate(masks):
        sub = _padded_call(G, G.node_subgraph_padded, d, mask, (N_cap, off[v + 1] - off[v]))
        seg, rows = slice(off[v], off[v + 1]), slice(v * N_cap, (v + 1) * N_cap)
        assert torch.equal(stack.valid[v], sub.valid), (what, v, stack.valid[v].tolist(), sub.valid.tolist())
        assert torch.equal(stack.edge_index[:, seg], sub.edge_index + v * N_cap), (what, v, "edge_index")
        assert torch.equal(stack.edge_id[seg], sub.edge_id) and torch.equal(stack.node_id[rows], sub.node_id), (what, v, "ids")
        assert torch.equal(stack.batch[rows], sub.batch + v * Gp), (what, v, "batch")
        assert torch.equal(stack.x[rows], sub.x) and torch.equal(stack.node_label[rows], sub.node_label), (what, v, "node rows")
        assert torch.equal(stack.edge_attr[seg], sub.edge_attr), (what, v, "edge_attr")


@pytest.mark.parametrize("kind", ["unpadded", "padded", "ragged"])
@pytest.mark.parametrize("S", [1, 3, 16])
def test_stack_equals_the_oracle_and_the_padded_extractions(dev, kind, S):
    import dp_gsat_amd as G
    G.clear_cache()
    b, lv = _input(kind, S)
    d = b.to(dev)
    level = torch.from_numpy(lv).to(dev)
    N, E, V = b.num_nodes, b.num_edges, 2 * S + 1
    assert N > _block() and N % _block() and E > 2 * _block() and E % _block()
    padded = hasattr(b, "valid")
    Gp, N_cap = (b.num_graphs, N) if padded else (b.num_graphs + 1, N + 2)
    offsets = [v * E for v in range(V + 1)]
    what = f"{kind} S={S}"
    bufs, inner = _raw_call(dev, d, level, S, Gp, N_cap, offsets, _real(b))
    torch.cuda.synchronize()
    _guards_intact(bufs, what)
    o = _oracle(b, lv, S, [E] * V, N_cap, Gp)
    _equals_oracle(inner, o, what)
    Nv, Ev = (N, E) if not padded else b.valid[:2].tolist()
    assert not o["valid"][:, 3].any() and o["valid"][0].tolist() == [Nv, Ev, b.valid[2].item() if padded else b.num_graphs, 0]
    again = _raw_call(dev, d, level, S, Gp, N_cap, offsets, _real(b))[1]
    for name in OUT:
        assert torch.equal(inner[name], again[name]), (what, name)                    # bitwise repeatable
    stack = _padded_call(G, G.explanation_stack_nodes, d, None, ratios=[(i + 1) / (S + 1) for i in range(S)], node_level=level)
    assert stack.variants == V and stack.graphs_per_variant == Gp and stack.node_capacity == N_cap and list(stack.segment_offsets) == offsets
    assert stack.num_graphs == V * Gp and stack.x.shape[0] == V * N_cap
    for name in OUT:
        assert torch.equal(getattr(stack, name).reshape(-1), inner[name].to(getattr(stack, name).dtype)), (what, name)
    _equals_the_extractions(G, d, level, stack, what)
    G.clear_cache()


def test_cap_nodes_of_n_plus_one_spoils_the_variants_that_need_two_padding_rows(dev):
    import dp_gsat_amd as G
    G.clear_cache()
    S = 3
    b, lv = _input("unpadded", S)
    d, level = b.to(dev), torch.from_numpy(lv).to(dev)
    N, E, V = b.num_nodes, b.num_edges, 2 * S + 1
    N_cap, Gp = N + 1, b.num_graphs + 1
    offsets = [v * E for v in range(V + 1)]
    bufs, inner = _raw_call(dev, d, level, S, Gp, N_cap, offsets, b.num_graphs)
    torch.cuda.synchronize()
    _guards_intact(bufs, "cap N + 1")
    o = _oracle(b, lv, S, [E] * V, N_cap, Gp)
    _equals_oracle(inner, o, "cap N + 1")
    assert o["valid"][:, 3].tolist() == [1, 0, 0, 0, 0, 0, 0]                          # every strict subset leaves two rows
    lvc = level.clamp(max=S)
    for v, mask in ((0, torch.ones_like(lvc, dtype=torch.bool)), (2, lvc <= 1), (5, lvc > 1)):
        sub = _padded_call(G, G.node_subgraph_padded, d, mask, (N_cap, E))
        assert torch.equal(inner["valid"].view(V, 4)[v], sub.valid) and torch.equal(inner["node_id"].view(V, N_cap)[v], sub.node_id)
        assert torch.equal(inner["edge_index"].view(2, V, E)[:, v], sub.edge_index + v * N_cap)
    G.clear_cache()


def test_one_short_segment_spoils_that_variant_only(dev):
    import dp_gsat_amd as G
    G.clear_cache()
    S = 3
    b, lv = _input("padded", S)
    d, level = b.to(dev), torch.from_numpy(lv).to(dev)
    N, E, V = b.num_nodes, b.num_edges, 2 * S + 1
    fit = _oracle(b, lv, S, [E] * V, N, b.num_graphs)["valid"]
    short = 1 + S + 1                                                                  # "without level 1"
    assert fit[short, 1] > 1
    caps = [E] * V
    caps[short] = int(fit[short, 1]) - 1
    offsets = np.concatenate([[0], np.cumsum(caps)]).tolist()
    bufs, inner = _raw_call(dev, d, level, S, b.num_graphs, N, offsets, _real(b))
    torch.cuda.synchronize()
    _guards_intact(bufs, "short segment")
    o = _oracle(b, lv, S, caps, N, b.num_graphs)
    _equals_oracle(inner, o, "short segment")
    assert o["valid"][:, 3].tolist() == [int(v == short) for v in range(V)]
    G.clear_cache()


@pytest.mark.parametrize("how", ["spoiled_input", "bad_endpoint"])
def test_an_overflowed_input_or_a_bad_endpoint_spoils_every_variant(dev, how):
    import dp_gsat_amd as G
    G.clear_cache()
    S = 3
    b, lv = _input("spoiled" if how == "spoiled_input" else "unpadded", S)
    if how == "bad_endpoint":
        b.edge_index[1, 17] = b.num_nodes + 1
    d, level = b.to(dev), torch.from_numpy(lv).to(dev)
    N, E, V = b.num_nodes, b.num_edges, 2 * S + 1
    padded = hasattr(b, "valid")
    Gp, N_cap = (b.num_graphs, N) if padded else (b.num_graphs + 1, N + 2)
    offsets = [v * E for v in range(V + 1)]
    bufs, inner = _raw_call(dev, d, level, S, Gp, N_cap, offsets, _real(b))
    torch.cuda.synchronize()
    _guards_intact(bufs, how)
    _equals_oracle(inner, _oracle(b, lv, S, [E] * V, N_cap, Gp), how)
    assert (inner["valid"].view(V, 4).cpu() == torch.tensor([0, 0, 0, 1], dtype=torch.int32)).all()
    assert (inner["edge_id"] == -1).all() and (inner["node_id"] == -1).all()
    assert (inner["batch"].view(V, N_cap) == (torch.arange(V, device=dev) * Gp + Gp - 1).view(V, 1)).all()
    with pytest.raises(ValueError, match="does not fit"):
        G.explanation_stack_nodes(d, None, ks=[1, 2, 3], node_level=level)           # eager: one host read reports it
    G.clear_cache()


def test_bad_arguments_are_refused(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import GsatHipError
    b, lv = _input("unpadded", 1)
    d, level = b.to(dev), torch.from_numpy(lv).to(dev)
    E = b.num_edges
    for S, N_cap, code in ((0, b.num_nodes + 2, -2), (17, b.num_nodes + 2, -2), (1, 1, -2)):          # GSAT_ERR_ARG, before anything is written
        with pytest.raises(GsatHipError, match=f"code {code}"):
            _raw_call(dev, d, level, S, b.num_graphs + 1, N_cap, [0] * (2 * S + 2), b.num_graphs)
    with pytest.raises(GsatHipError, match="code -4"):                                  # GSAT_ERR_UNSUPPORTED: V * cap_nodes at or above 2^31
        _raw_call(dev, d, level, 1, b.num_graphs + 1, b.num_nodes + 2, [0, E, 2 * E, 3 * E], b.num_graphs,
                  {k: torch.zeros(2 * GUARD + 8 * E, dtype=dt, device=dev)
                   for k, dt in (("edge_index", torch.int64), ("edge_id", torch.int64), ("node_id", torch.int64), ("batch", torch.int64),
                                 ("valid", torch.int32), ("ws", torch.uint8))}, cap_nodes_arg=(1 << 31) // 3)
    with pytest.raises(ValueError):
        G.explanation_stack_nodes(d, None, ks=[1], node_level=level[:-1])
    with pytest.raises(ValueError):
        G.explanation_stack_nodes(d, torch.zeros(3, device=dev), ks=[1])
    G.clear_cache()


def test_a_capture_holds_five_kernel_nodes_and_follows_the_levels_changed_in_place(dev):
    import dp_gsat_amd as G
    G.clear_cache()
    S = 3
    b, lv = _input("ragged", S)
    d, level = b.to(dev), torch.from_numpy(lv).to(dev)
    N, E, V = b.num_nodes, b.num_edges, 2 * S + 1
    offsets = [v * E for v in range(V + 1)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bufs, inner = _raw_call(dev, d, level, S, b.num_graphs, N, offsets, _real(b))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = tl.kept_debug_graph()
    assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
    with torch.cuda.graph(graph):
        _raw_call(dev, d, level, S, b.num_graphs, N, offsets, _real(b), bufs)
    path = os.path.join(tempfile.mkdtemp(), "graph.dot")
    graph.debug_dump(path)
    dot = open(path, errors="replace").read()
    assert assert_no_memset_nodes(dot, "gsat_fidelity_stack_nodes") and "memcpy" not in dot.lower()
    nodes = tl.kernel_nodes(dot)
    assert nodes is not None, dot[:2000]
    want = ("k_stkn_hist", "k_stkn_scan", "k_stkn_nodes", "k_stkn_edges", "k_stkn_fill")
    assert len(nodes) == 5 and [n for k in want for n in nodes if k in n] == nodes, nodes
    lv2 = _levels(b, *_host_batch(extra_graphs=3)[1:], S, seed=9)
    lv2 = np.concatenate([lv2, lv[len(lv2):]])
    assert not np.array_equal(lv, lv2)
    level.copy_(torch.from_numpy(lv2).to(dev))                                         # in place: the graph reads the same buffer
    for name in OUT:
        inner[name].fill_(-5)
    graph.replay()
    torch.cuda.synchronize()
    _guards_intact(bufs, "replayed")
    _equals_oracle(inner, _oracle(b, lv2, S, [E] * V, N, b.num_graphs), "replayed")
    eager = _raw_call(dev, d, level, S, b.num_graphs, N, offsets, _real(b))[1]
    for name in OUT:
        assert torch.equal(inner[name], eager[name]), name
    G.clear_cache()
