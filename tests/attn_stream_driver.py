"""C-ABI driver of the streamed-extractor tests: one gsat_attn_stream_fwd + gsat_attn_stream_bwd call for a case of
tests/extractor_cases.py / tests/attn_stream_cases.py at a row budget, every output NaN-prefilled, no a1 buffer and no row order passed."""
import ctypes

import torch

from tests.extractor_driver import _sync


def host_plan(seg_ptr, budget):
    """gsat_attn_stream_plan on a host list: (group_ptr as a list, scratch_rows).  No GPU needed."""
    from dp_gsat_amd._lib import call
    G = len(seg_ptr) - 1
    seg = (ctypes.c_int32 * (G + 1))(*seg_ptr)
    group_ptr = (ctypes.c_int32 * (G + 1))(*([-1] * (G + 1)))
    n, rows = ctypes.c_int64(-1), ctypes.c_int64(-1)
    call("gsat_attn_stream_plan", seg, G, budget, group_ptr, ctypes.byref(n), ctypes.byref(rows))
    return [int(group_ptr[i]) for i in range(n.value + 1)], rows.value


def workspace_bytes(rows, nodes, H, budget):
    """(forward, backward) workspace of the streamed entry points for graphs of ``rows`` edge rows and ``nodes`` nodes each, width H: host
    arithmetic on the extents alone.  No GPU needed."""
    from dp_gsat_amd import _lib
    lib = _lib.load()
    G = len(rows)
    a = _lib.AttnArgs()
    a.M, a.N, a.G, a.H, a.C1, a.C2, a.edge_mode, a.training, a.p_drop = sum(rows), sum(nodes), G, H, 4 * H, H, 1, 1, 0.5
    seg = [0]
    for r in rows:
        seg.append(seg[-1] + r)
    gp, scratch = host_plan(seg, budget)
    fwd = lib.gsat_attn_stream_fwd_workspace_bytes(ctypes.byref(a), scratch)
    bwd = lib.gsat_attn_stream_bwd_workspace_bytes(ctypes.byref(a), (ctypes.c_int32 * len(gp))(*gp), len(gp) - 1, (ctypes.c_int32 * (G + 1))(*seg), scratch)
    return int(fwd), int(bwd), gp, scratch


def verdict(dev, ei, batch, G):
    """gsat_attn_stream_check of a batch, through the tables the package builds for it."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.graph_index import BatchIndex
    index = BatchIndex(ei.to(dev), int(batch.shape[0]))
    seg = index.graphs(batch.to(dev), G)
    eptr, _, _, eg32 = seg.edge_segments
    word = torch.full((1,), -1, dtype=torch.int32, device=dev)
    call("gsat_attn_stream_check", ptr(index.src32), ptr(index.dst32), ptr(seg.node_seg32), ptr(eptr), ptr(eg32), index.E, index.N, G, ptr(word),
         stream())
    _sync()
    return int(word.item())


def run_stream(dev, case, budget, philox_seed=None):
    """Streamed forward + backward of ``case`` at ``budget`` rows.  ``philox_seed``: pass no mask and no noise tensor, draw in the kernels."""
    from dp_gsat_amd import _lib
    from dp_gsat_amd._lib import AttnGrads, call, ptr, stream
    from dp_gsat_amd.graph_index import BatchIndex
    from dp_gsat_amd.ops import _attn_args
    assert case["edge_mode"]
    training, G_ = case["training"], case["G"]
    emb = case["emb"].to(dev)
    params = tuple(t.to(dev) for t in case["params"])
    index = BatchIndex(case["ei"].to(dev), emb.shape[0])
    seg = index.graphs(case["batch"].to(dev), G_)
    plan = seg.stream_plan(budget)
    N, H = emb.shape
    C1, C2 = params[0].shape[0], params[2].shape[0]
    M = index.E
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    P, Q = nan(N, C1), nan(N, C1)
    h2, stats, logits, att = nan(M, C2), nan(max(G_, 1) * (2 * C1 + 2 * C2)), nan(M), nan(M)
    m1 = m2 = u = None
    seed = 7
    if training and philox_seed is None:
        m1, m2 = (t.to(dev) for t in case["masks"])
        u = case["u"].to(dev)
    elif training:
        seed = philox_seed
    args = _attn_args(emb, params, index, seg, True, training, 0.5, seed, m1, m2, u, (P, Q, None, h2, stats, logits, att), None,
                      philox_seed is not None)
    args.seg_order = None
    lib = _lib.load()
    n = int(lib.gsat_attn_stream_fwd_workspace_bytes(ctypes.byref(args), plan.scratch_rows))
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
    args.fwd_workspace, args.fwd_workspace_bytes = ptr(ws), n
    call("gsat_attn_stream_fwd", ctypes.byref(args), plan.group_ptr, plan.n_groups, plan.seg_ptr, plan.node_ptr, plan.scratch_rows, stream())
    _sync()
    n1, n2 = G_ * C1, G_ * C2
    out = dict(plan=plan, fwd_bytes=n, logits=logits, att=att, P=P, Q=Q, h2=h2, stats=stats,
               mean1=stats[:n1].view(G_, C1), rstd1=stats[n1:2 * n1].view(G_, C1),
               mean2=stats[2 * n1:2 * n1 + n2].view(G_, C2), rstd2=stats[2 * n1 + n2:2 * n1 + 2 * n2].view(G_, C2))
    g = AttnGrads()
    dl, da = case["dlogits"].to(dev), case["datt"].to(dev)
    g.dlogits, g.datt = ptr(dl), ptr(da)
    g.rowptr_src, g.eid_by_src = ptr(index.rowptr_src), ptr(index.eid_by_src)
    g.rowptr_dst, g.eid_by_dst = ptr(index.rowptr_dst), ptr(index.eid_by_dst)
    g.chunk_ptr_dst, g.chunk_ptr_src = (ptr(t) for t in index.long_rows)
    out["hubs"] = tuple(t is not None for t in index.long_rows)
    demb = torch.full_like(emb, float("nan"))
    grads = [torch.full_like(t, float("nan")) for t in params]
    g.demb = ptr(demb)
    g.dW1, g.db1, g.dW2, g.db2, g.dW3, g.db3 = (ptr(t) for t in grads)
    nb = int(lib.gsat_attn_stream_bwd_workspace_bytes(ctypes.byref(args), plan.group_ptr, plan.n_groups, plan.seg_ptr, plan.scratch_rows))
    wsb = torch.empty(nb, dtype=torch.uint8, device=dev)
    g.workspace, g.workspace_bytes = ptr(wsb), nb
    call("gsat_attn_stream_bwd", ctypes.byref(args), ctypes.byref(g), plan.group_ptr, plan.n_groups, plan.seg_ptr, plan.node_ptr,
         plan.scratch_rows, stream())
    _sync()
    out.update(bwd_bytes=nb, demb=demb, dW1=grads[0], db1=grads[1], dW2=grads[2], db2=grads[3], dW3=grads[4].view(1, -1), db3=grads[5])
    return out
