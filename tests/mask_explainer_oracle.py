"""Independent restatements for the mask-explainer tests.

fp64 numpy of the formulas of csrc/mask_explainer.hip (the step, the per-graph objective terms, the per-graph min-max rule), and the
whole GNNExplainer loop on the CPU oracle with torch autograd and torch.optim.Adam -- which restates neither the derivative nor the
optimiser by hand, so the two check each other (tests/test_mask_explainer_host.py)."""
import numpy as np
import torch

LOG_EPS = 1e-15
HYPER = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, size_coef=0.005, ent_coef=1.0)


def sigmoid64(m):
    m = np.asarray(m, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-m))


def entropy64(a):
    a = np.asarray(a, np.float64)
    return -a * np.log(a + LOG_EPS) - (1.0 - a) * np.log(1.0 - a + LOG_EPS)


def dentropy64(a):
    a = np.asarray(a, np.float64)
    c = 1.0 - a
    return -np.log(a + LOG_EPS) - a / (a + LOG_EPS) + np.log(c + LOG_EPS) + c / (c + LOG_EPS)


def step_state(t, b1=HYPER["b1"], b2=HYPER["b2"]):
    """float32[4] the kernels keep after ``t`` steps: (t, 1 / (1 - b1^(t+1)), 1 / sqrt(1 - b2^(t+1)), 0)."""
    return np.array([t, 1.0 / (1.0 - b1 ** (t + 1)), 1.0 / np.sqrt(1.0 - b2 ** (t + 1)), 0.0], np.float32)


def mask_step64(m, mu, nu, a, g_a, inv_eg, t, b, m_valid, lr, b1, b2, eps, size_coef, ent_coef):
    """One step from ``t`` steps taken, on the first ``m_valid`` entries; the other entries come back unchanged.  ``a`` is the mask
    the backward ran with (what the buffer holds)."""
    m, mu, nu, a = (np.array(v, np.float64) for v in (m, mu, nu, a))
    s = slice(0, m_valid)
    av = a[s]
    G = av * (1.0 - av) * (b * np.asarray(g_a, np.float64)[s] + size_coef + ent_coef * dentropy64(av) * np.asarray(inv_eg, np.float64)[s])
    t1 = t + 1
    mu[s] = b1 * mu[s] + (1.0 - b1) * G
    nu[s] = b2 * nu[s] + (1.0 - b2) * G * G
    m[s] = m[s] - (lr / (1.0 - b1 ** t1)) * mu[s] / (np.sqrt(nu[s]) / np.sqrt(1.0 - b2 ** t1) + eps)
    a[s] = sigmoid64(m[s])
    return m, mu, nu, a


def graph_terms64(a, edge_ptr, edge_order, graphs, m_valid):
    """float64[G, 2]: per graph (sum a, mean H(a)) over its slots; rows at or beyond ``graphs`` are 0."""
    G = len(edge_ptr) - 1
    out = np.zeros((G, 2))
    a = np.asarray(a, np.float64)
    for g in range(min(graphs, G)):
        e = np.asarray(edge_order[edge_ptr[g]:edge_ptr[g + 1]], np.int64)
        n = len(e)
        e = e[e < m_valid]
        out[g] = (a[e].sum(), entropy64(a[e]).sum() / max(n, 1))
    return out


def minmax64(att, edge_ptr, edge_order, power, eps, graphs=None, m_valid=None):
    att = np.asarray(att, np.float64)
    G = len(edge_ptr) - 1
    graphs = G if graphs is None else graphs
    m_valid = len(att) if m_valid is None else m_valid
    out = np.zeros(len(att))
    for g in range(min(graphs, G)):
        e = np.asarray(edge_order[edge_ptr[g]:edge_ptr[g + 1]], np.int64)
        e = e[e < m_valid]
        if len(e) == 0:
            continue
        v = att[e] ** power
        out[e] = (v - v.min()) / (v.max() - v.min() + eps)
    return out


def segments(edge_graph, G):
    """(edge_ptr int32[G + 1], edge_order int32[E]): the slots grouped by graph, ascending inside a graph (a stable sort)."""
    edge_graph = np.asarray(edge_graph, np.int64)
    order = np.argsort(edge_graph, kind="stable").astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(edge_graph, minlength=G))]).astype(np.int32)
    return ptr, order


# ---- the whole explainer on the CPU oracle ----------------------------------------------------------------------------------------------------
def _edge_attr(data, dtype):
    return None if data.edge_attr is None else data.edge_attr.to(dtype)


def predicted(logits):
    return (logits > 0).to(logits.dtype) if logits.shape[1] == 1 else logits.argmax(dim=1)


def objective_terms(oclf, data, m, targets):
    """(pred, size, entropy, logits) with autograd through ``m``: sum of the per-graph criteria, sum of a, sum of per-graph mean H."""
    a = torch.sigmoid(m)
    logits = oclf(data.x.to(m.dtype), data.edge_index, data.batch, _edge_attr(data, m.dtype), edge_atten=a.view(-1, 1))
    if logits.shape[1] == 1:
        pred = torch.nn.functional.binary_cross_entropy_with_logits(logits, targets.to(m.dtype), reduction="sum")
    else:
        pred = torch.nn.functional.cross_entropy(logits, targets.long(), reduction="sum")
    G = int(data.batch.max()) + 1
    eg = data.batch[data.edge_index[0]]
    counts = torch.bincount(eg, minlength=G).clamp(min=1).to(m.dtype)
    H = -a * torch.log(a + LOG_EPS) - (1 - a) * torch.log(1 - a + LOG_EPS)
    ent = torch.zeros(G, dtype=m.dtype).index_add_(0, eg, H) / counts
    return pred, a.sum(), ent.sum(), logits


def oracle_explain(oclf, data, steps, dtype=torch.float32, init=None, target="model", lr=0.01, b1=0.9, b2=0.999, eps=1e-8, size_coef=0.005,
                   ent_coef=1.0):
    """torch.optim.Adam on the mask logits of the eval-mode oracle backbone.  Returns dict(mask_logits, a, history [steps, 3], objective
    [3] of the final mask, first_grad = dL/dm of the first step, logits of the unmasked batch, targets)."""
    import copy
    clf = copy.deepcopy(oclf).to(dtype).eval()
    for p in clf.parameters():
        p.requires_grad_(False)
    E = int(data.edge_index.shape[1])
    with torch.no_grad():
        logits0 = clf(data.x.to(dtype), data.edge_index, data.batch, _edge_attr(data, dtype), edge_atten=None)
    targets = predicted(logits0) if target == "model" else (data.y.view(-1, 1) if logits0.shape[1] == 1 else data.y.view(-1))
    m = (torch.zeros(E) if init is None else init.detach().clone()).to(dtype).requires_grad_(True)
    opt = torch.optim.Adam([m], lr=lr, betas=(b1, b2), eps=eps)
    hist, first_grad = [], None
    for _ in range(steps):
        opt.zero_grad()
        pred, size, ent, _ = objective_terms(clf, data, m, targets)
        (pred + size_coef * size + ent_coef * ent).backward()
        if first_grad is None:
            first_grad = m.grad.detach().clone()
        hist.append(torch.stack([pred.detach(), size.detach(), ent.detach()]))
        opt.step()
    with torch.no_grad():
        pred, size, ent, _ = objective_terms(clf, data, m, targets)
    return dict(mask_logits=m.detach(), a=torch.sigmoid(m.detach()), history=torch.stack(hist), objective=torch.stack([pred, size, ent]),
                first_grad=first_grad, logits=logits0, targets=targets)


def oracle_saliency(oclf, data, dtype=torch.float32, target="model"):
    """d z_target / d edge_atten at edge_atten = 1 on the eval-mode oracle backbone, signed."""
    import copy
    clf = copy.deepcopy(oclf).to(dtype).eval()
    att = torch.ones(int(data.edge_index.shape[1]), 1, dtype=dtype, requires_grad=True)
    logits = clf(data.x.to(dtype), data.edge_index, data.batch, _edge_attr(data, dtype), edge_atten=att)
    t = predicted(logits.detach()) if target == "model" else (data.y.view(-1, 1) if logits.shape[1] == 1 else data.y.view(-1))
    score = (logits * (2 * t.to(dtype) - 1)).sum() if logits.shape[1] == 1 else logits.gather(1, t.long().view(-1, 1)).sum()
    grad, = torch.autograd.grad(score, att)
    return grad.view(-1)


def set_running_stats(oclf, seed=0):
    """Running statistics away from (0, 1), as a trained backbone has them."""
    g = torch.Generator().manual_seed(seed)
    for mod in oclf.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.3)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) * 1.5 + 0.5)
    return oclf
