"""C-ABI driver of the extractor path tests: one gsat_attn_fwd (+ gsat_attn_bwd) call for a case of tests/extractor_cases.py, every output
NaN-prefilled, plus what gsat_attn_paths reports for exactly those arguments under the environment of the call."""
import ctypes

import torch

ORDERS = ("auto", "none", "identity")


def _sync():
    """Wait for the device; a HIP error here (a fault in a kernel) ends the whole run -- nothing more is started on a faulted device."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        import pytest
        pytest.exit(f"HIP error after an extractor launch, stopping the run: {e}", returncode=3)


def shape_args(case, fused, with_order):
    """AttnArgs holding only the extents and switches of ``case`` (no device memory): what gsat_attn_paths needs.  Pointers the predicates
    test for NULL get a placeholder."""
    from dp_gsat_amd._lib import AttnArgs
    from tests.extractor_cases import widths
    a = AttnArgs()
    _, C1, C2 = widths(case["edge_mode"], case["H"])
    a.M, a.N, a.G, a.H, a.C1, a.C2 = case["M"], case["N"], case["G"], case["H"], C1, C2
    a.edge_mode, a.training, a.p_drop, a.fused = int(case["edge_mode"]), int(case["training"]), 0.5, fused
    a.seg_order = 8 if with_order else None
    a.node_ptr = 8
    return a


def run(dev, case, fused=-1, order="auto", backward=True, dlogits=True, datt=True):
    """Forward (+ backward) of ``case`` through the C ABI.  ``fused``: gsat_attn_args.fused (-1 staged / 0 automatic / 1 one-launch forward).
    ``order``: "auto" = what the package passes (edge mode: the row order of its edge segments; node mode: none), "none" = no seg_order
    (the rows must be grouped by graph), "identity" = an explicit identity order.  Returns the outputs, the saved tensors with the
    statistics split into mean / variance, the gradients, and ``paths`` = gsat_attn_paths of the arguments."""
    from dp_gsat_amd import _lib
    from dp_gsat_amd._lib import AttnGrads, attn_paths, call, ptr, stream
    from dp_gsat_amd.graph_index import BatchIndex
    from dp_gsat_amd.ops import _attn_args
    assert order in ORDERS
    edge_mode, training, G_ = case["edge_mode"], case["training"], case["G"]
    emb = case["emb"].to(dev)
    params = tuple(t.to(dev) for t in case["params"])
    index = BatchIndex(case["ei"].to(dev), emb.shape[0])
    seg = index.graphs(case["batch"].to(dev), G_)
    N, H = emb.shape
    C1, C2 = params[0].shape[0], params[2].shape[0]
    M = index.E if edge_mode else N
    assert M == case["M"]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    P, Q = nan(N, C1), (nan(N, C1) if edge_mode else None)
    a1, h2, stats, logits, att = nan(M, C1), nan(M, C2), nan(max(G_, 1) * (2 * C1 + 2 * C2)), nan(M), nan(M)
    m1, m2 = (t.to(dev) for t in case["masks"]) if training else (None, None)
    u = case["u"].to(dev) if training else None
    args = _attn_args(emb, params, index, seg, edge_mode, training, 0.5, 7, m1, m2, u, (P, Q, a1, h2, stats, logits, att), None, False)
    args.fused = fused
    keep = None
    if order == "none":
        args.seg_order = None
    elif order == "identity":
        keep = torch.arange(M, dtype=torch.int32, device=dev)
        args.seg_order = ptr(keep)
    n = int(_lib.load().gsat_attn_fwd_workspace_bytes(ctypes.byref(args)))
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
    args.fwd_workspace, args.fwd_workspace_bytes = ptr(ws), n
    paths = attn_paths(args)
    assert paths["fwd_kind"] == int(_lib.load().gsat_attn_fwd_kind(ctypes.byref(args)))
    call("gsat_attn_fwd", ctypes.byref(args), stream())
    _sync()
    n1, n2 = G_ * C1, G_ * C2
    out = dict(paths=paths, logits=logits, att=att, P=P, Q=Q, a1=a1, h2=h2, stats=stats,
               mean1=stats[:n1].view(G_, C1), rstd1=stats[n1:2 * n1].view(G_, C1),
               mean2=stats[2 * n1:2 * n1 + n2].view(G_, C2), rstd2=stats[2 * n1 + n2:2 * n1 + 2 * n2].view(G_, C2))
    if not backward:
        return out
    g = AttnGrads()
    dl, da = case["dlogits"].to(dev), case["datt"].to(dev)
    g.dlogits, g.datt = (ptr(dl) if dlogits else None), (ptr(da) if datt else None)
    if edge_mode:
        g.rowptr_src, g.eid_by_src = ptr(index.rowptr_src), ptr(index.eid_by_src)
        g.rowptr_dst, g.eid_by_dst = ptr(index.rowptr_dst), ptr(index.eid_by_dst)
        g.chunk_ptr_dst, g.chunk_ptr_src = (ptr(t) for t in index.long_rows)
    demb = torch.full_like(emb, float("nan"))
    grads = [torch.full_like(t, float("nan")) for t in params]
    g.demb = ptr(demb)
    g.dW1, g.db1, g.dW2, g.db2, g.dW3, g.db3 = (ptr(t) for t in grads)
    nb = int(_lib.load().gsat_attn_bwd_workspace_bytes(ctypes.byref(args)))
    wsb = torch.empty(nb, dtype=torch.uint8, device=dev)
    g.workspace, g.workspace_bytes = ptr(wsb), nb
    assert attn_paths(args) == paths
    call("gsat_attn_bwd", ctypes.byref(args), ctypes.byref(g), stream())
    _sync()
    out.update(demb=demb, dW1=grads[0], db1=grads[1], dW2=grads[2], db2=grads[3], dW3=grads[4].view(1, -1), db3=grads[5])
    return out
