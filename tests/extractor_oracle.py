"""fp64 / fp32 reference of one extractor step (forward, saved tensors, every gradient) for the cases of tests/extractor_cases.py, and the
comparison rule of the path tests.  CPU only: oracle.modules.ExtractorMLP + oracle.ops.concrete_sample under autograd."""
import torch

from oracle import modules as om
from oracle import ops as oops
from tests.util import TOL

EPS = 1e-5

_cache = {}


def _segment_stats(x, seg, G):
    """Per-graph mean and biased variance of the centred values; a graph without rows: mean 0, variance 0."""
    n = oops.seg_count(seg, G, x.dtype).clamp_(min=1).view(-1, 1)
    mean = oops.scatter_sum(x, seg, G) / n
    xc = x - mean.index_select(0, seg)
    return mean, oops.scatter_sum(xc * xc, seg, G) / n


def reference_one(case, dtype):
    """Everything the kernels write for ``case``, evaluated in ``dtype``.  Saved tensors follow the library's layout: P / Q and h2 without
    their biases, a1 after ReLU and dropout, statistics of the biased pre-activations."""
    H, edge_mode, training, G = case["H"], case["edge_mode"], case["training"], case["G"]
    ei, batch = case["ei"], case["batch"]
    ext = om.ExtractorMLP(H, edge_mode, dropout=0.5).to(dtype)
    keys = [f"feature_extractor.{i}.{p}" for i in (0, 4, 8) for p in ("weight", "bias")]
    ext.load_state_dict({k: v.to(dtype) for k, v in zip(keys, case["params"])})
    ext.train(training)
    masks = [m.to(dtype) for m in case["masks"]] if training else None
    u = case["u"].to(dtype).view(-1, 1) if training else None
    emb = case["emb"].to(dtype).clone().requires_grad_(True)
    if case["M"] == 0:
        raise ValueError("a case needs at least one row")
    # the oracle takes the graph count from the batch vector; a trailing empty graph has no rows and changes nothing
    z = ext(emb, ei, batch, masks=masks)
    att = oops.concrete_sample(z, u, training)
    torch.autograd.backward([z, att], [case["dlogits"].to(dtype).view(-1, 1), case["datt"].to(dtype).view(-1, 1)])
    W1, b1, W2, b2, W3, b3 = (p for lin in ext.feature_extractor.weights() for p in lin)
    out = dict(logits=z.detach().view(-1), att=att.detach().view(-1), demb=emb.grad, dW1=W1.grad, db1=b1.grad, dW2=W2.grad, db2=b2.grad,
               dW3=W3.grad, db3=b3.grad)
    with torch.no_grad():
        e = emb.detach()
        if edge_mode:
            seg = batch[ei[0]]
            out["P"], out["Q"] = e @ W1[:, :H].T, e @ W1[:, H:].T
            x = torch.cat([e[ei[0]], e[ei[1]]], dim=-1)
        else:
            seg = batch
            out["P"], out["Q"] = e @ W1.T, None
            x = e
        _, hidden = oops.mlp_forward(x, seg, G, ext.feature_extractor.weights(), 0.5, masks, training, return_hidden=True)
        out["a1"] = hidden[0]
        out["h2"] = hidden[0] @ W2.T
        out["mean1"], out["var1"] = _segment_stats(x @ W1.T + b1, seg, G)
        out["mean2"], out["var2"] = _segment_stats(out["h2"] + b2, seg, G)
        # distance of the centred pre-activations from the kink of ReLU (exact zeros aside), see extractor_cases.RELU_MARGIN
        xc = [(x @ W1.T + b1) - out["mean1"].index_select(0, seg), (out["h2"] + b2) - out["mean2"].index_select(0, seg)]
        out["relu_margin"] = min(float(t[t != 0].abs().min()) if bool((t != 0).any()) else float("inf") for t in xc)
    return out


def references(case, key=None):
    """(fp32, fp64) references of a case, computed once per ``key`` and left unchanged."""
    if key is None:
        key = (case["family"], case["name"], case["edge_mode"], case["H"], case["training"], case["sorted_edges"])
    if key not in _cache:
        _cache[key] = (reference_one(case, torch.float32), reference_one(case, torch.float64))
    return _cache[key]


def gap(r32, r64):
    """(|r32 - r64|max, scale) with scale = max(1, |r64|max): the reference's own rounding error and the unit it is measured in."""
    a, b = r32.detach().double(), r64.detach().double()
    if b.numel() == 0:
        return 0.0, 1.0
    return (a - b).abs().max().item(), max(1.0, b.abs().max().item())


def close64(actual, r32, r64, what, cap):
    """The project's rule against the fp64 reference, |actual - r64|max <= TOL * scale + 4 * |r32 - r64|max, after asserting that the slack
    term is at most ``cap`` * scale -- so a comparison can never pass on slack alone.  Returns err / allowed."""
    a = actual.detach().cpu().double()
    b = r64.detach().double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} != {tuple(b.shape)}"
    if a.numel() == 0:
        return 0.0
    assert not torch.isnan(a).any(), f"{what}: NaN entries (unwritten rows?)"
    g, scale = gap(r32, r64)
    assert 4.0 * g <= cap * scale, f"{what}: the reference's own slack 4 * {g:.3e} exceeds the cap {cap:.1e} * scale {scale:.3e}"
    allowed = TOL * scale + 4.0 * g
    err = (a - b).abs().max().item()
    assert err <= allowed, f"{what}: max abs err {err:.3e} > allowed {allowed:.3e} (scale {scale:.3e}, slack {4.0 * g:.3e})"
    return err / allowed
