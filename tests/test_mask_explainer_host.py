"""Host-side checks of the post-hoc baselines: the C ABI of csrc/mask_explainer.hip, the constructors' refusals, and the two
restatements the GPU tests compare against (tests/mask_explainer_oracle.py) checked against each other."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mask_explainer_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsat_mask_init", "gsat_mask_step", "gsat_mask_objective", "gsat_segment_minmax_norm")
CTYPE = {"int64_t": "I64", "int": "INT", "float": "F32", "size_t": "SZ", "double": "F64"}


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes
    import __graft_entry__ as ge
    from dp_gsat_amd import _lib
    ge.build()
    header = open(os.path.join(ROOT, "include", "gsat_hip.h")).read()
    assert re.search(r"#define\s+GSAT_ABI_VERSION\s+4\b", header)
    assert _lib.load().gsat_abi_version() == 4
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/gsat_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        args = [a.strip() for a in m.group(1).split(",")]
        res, sig = _lib.SIGNATURES[name]
        assert res is _lib.INT and len(sig) == len(args), (name, len(sig), args)
        for a, c in zip(args, sig):
            want = _lib.P if "*" in a else getattr(_lib, CTYPE[a.split()[0]])
            assert c is want, (name, a, c)


def _clf():
    import dp_gsat_amd as G
    return G.get_model(4, 0, 2, False, dict(model_name="GIN", n_layers=1, hidden_size=8, dropout_p=0.0), "cpu")


def test_constructor_refusals():
    import dp_gsat_amd as G
    clf = _clf()
    crit = G.Criterion(2, False)
    G.GNNExplainer(clf, crit)                                      # the defaults are taken
    with pytest.raises(ValueError, match="multi-label"):
        G.GNNExplainer(clf, G.Criterion(3, True, capturable=True))
    gsat = G.GSAT(clf, G.ExtractorMLP(8, True), crit, None)
    with pytest.raises(ValueError, match="backbone"):
        G.GNNExplainer(gsat, crit)
    with pytest.raises(ValueError, match="backbone"):
        G.edge_saliency(gsat, None)
    for bad in (dict(steps=0), dict(steps=1.5), dict(lr=0.0), dict(lr=-1e-3), dict(size_coef=-1.0), dict(ent_coef=-0.5),
                dict(betas=(1.0, 0.999)), dict(target="truth")):
        with pytest.raises(ValueError):
            G.GNNExplainer(clf, crit, **bad)
    with pytest.raises(ValueError, match="target"):
        G.edge_saliency(clf, None, target="truth")


def test_sync_group_batchnorm_is_refused():
    import dp_gsat_amd as G
    clf = _clf()
    bn = next(m for m in clf.modules() if type(m).__name__ == "BatchNorm1d")
    bn.sync_group = object()
    with pytest.raises(ValueError, match="sync_group"):
        G.GNNExplainer(clf, G.Criterion(2, False))
    with pytest.raises(ValueError, match="sync_group"):
        G.edge_saliency(clf, None)


def test_replayed_refusals_come_before_any_launch():
    """No GPU here: every refusal must be raised before the first device call."""
    import dp_gsat_amd as G
    from types import SimpleNamespace as NS
    clf, crit = _clf(), G.Criterion(2, False)
    ds = NS(y_all=torch.zeros(4, 1), edge_label_all=None, num_graphs=4)
    with pytest.raises(ValueError, match="edge_label_all"):
        G.ReplayedGNNExplainer(clf, crit, ds, 2, 5)
    with pytest.raises(ValueError, match="multi-label"):
        G.ReplayedGNNExplainer(clf, G.Criterion(3, True), NS(y_all=torch.zeros(4, 1), edge_label_all=torch.zeros(3), num_graphs=4), 2, 5)
    with pytest.raises(ValueError, match="bare backbone"):
        G.ReplayedGNNExplainer(G.GSAT(clf, G.ExtractorMLP(8, True), crit, None), crit, ds, 2, 5)
    with pytest.raises(ValueError, match="steps"):
        G.ReplayedGNNExplainer(clf, crit, NS(y_all=torch.zeros(4, 1), edge_label_all=torch.zeros(3), num_graphs=4), 2, 5, steps=0)


def test_frozen_context_restores_every_flag():
    from dp_gsat_amd.baselines import _frozen
    clf = _clf().train()
    params = list(clf.parameters())
    params[0].requires_grad_(False)
    clf.convs[0].eval()
    before = ([m.training for m in clf.modules()], [p.requires_grad for p in params])
    with pytest.raises(RuntimeError):
        with _frozen(clf):
            assert not any(m.training for m in clf.modules()) and not any(p.requires_grad for p in params)
            raise RuntimeError("inside")
    assert ([m.training for m in clf.modules()], [p.requires_grad for p in params]) == before


# ---- the restatements against each other -------------------------------------------------------------------------------------------------
def test_entropy_derivative_matches_autograd():
    a = torch.tensor([1e-12, 1e-6, 0.1, 0.5, 0.73, 1 - 1e-6, 1 - 1e-12], dtype=torch.float64, requires_grad=True)
    H = -a * torch.log(a + mo.LOG_EPS) - (1 - a) * torch.log(1 - a + mo.LOG_EPS)
    g, = torch.autograd.grad(H.sum(), a)
    np.testing.assert_allclose(mo.dentropy64(a.detach().numpy()), g.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(mo.entropy64(a.detach().numpy()), H.detach().numpy(), rtol=1e-14)


def test_saturated_logits_give_finite_zero_gradients():
    for v in (40.0, -40.0, 104.0, -104.0):
        a32 = np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-v), dtype=np.float32)) if v > -80 else np.float32(0.0)
        d = mo.dentropy64(np.float64(a32))
        assert np.isfinite(d)
        assert abs(float(a32) * (1.0 - float(a32)) * d) < 1e-15


def test_numpy_step_is_torch_adam_on_the_stated_objective():
    """Five steps of the numpy restatement (a synthetic linear criterion: g_a constant per edge) against torch.optim.Adam with autograd
    through sigmoid and both regularisers, fp64."""
    rng = np.random.RandomState(3)
    edge_graph = np.repeat(np.arange(4), [1, 7, 0, 12])            # graph 2 has no edge
    E, G = len(edge_graph), 4
    counts = np.bincount(edge_graph, minlength=G)
    inv_eg = 1.0 / counts[edge_graph]
    w = rng.randn(E)                                               # d(sum criterion)/da, held fixed: the mean criterion's is w / G
    m0 = rng.randn(E) * 2
    h = mo.HYPER
    m = torch.tensor(m0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([m], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"])
    eg = torch.from_numpy(edge_graph)
    for _ in range(5):
        opt.zero_grad()
        a = torch.sigmoid(m)
        H = -a * torch.log(a + mo.LOG_EPS) - (1 - a) * torch.log(1 - a + mo.LOG_EPS)
        ent = (torch.zeros(G, dtype=torch.float64).index_add_(0, eg, H) / torch.from_numpy(np.maximum(counts, 1).astype(np.float64))).sum()
        ((torch.from_numpy(w) * a).sum() + h["size_coef"] * a.sum() + h["ent_coef"] * ent).backward()
        opt.step()
    mn, mu, nu = m0.copy(), np.zeros(E), np.zeros(E)
    a = mo.sigmoid64(mn)
    for t in range(5):
        mn, mu, nu, a = mo.mask_step64(mn, mu, nu, a, w / G, inv_eg, t, G, E, **h)
    np.testing.assert_allclose(mn, m.detach().numpy(), rtol=1e-10, atol=1e-12)
    state = mo.step_state(5)
    assert state[0] == 5 and abs(state[1] - 1 / (1 - 0.9 ** 6)) < 1e-6 and abs(state[2] - 1 / np.sqrt(1 - 0.999 ** 6)) < 1e-5


def test_minmax_and_terms_restatements():
    ptr, order = mo.segments([2, 0, 2, 2, 0, 3], 5)
    assert ptr.tolist() == [0, 2, 2, 5, 6, 6] and order.tolist() == [1, 4, 0, 2, 3, 5]
    att = np.array([0.2, 0.9, 0.4, 0.8, 0.1, 0.7])
    out = mo.minmax64(att, ptr, order, 1.0, 1e-6)
    np.testing.assert_allclose(out[[1, 4]], [0.8 / (0.8 + 1e-6), 0.0])
    assert out[5] == 0.0                                            # a one-edge graph
    np.testing.assert_allclose(mo.minmax64(att, ptr, order, 10.0, 1e-6)[3], (0.8 ** 10 - 0.2 ** 10) / (0.8 ** 10 - 0.2 ** 10 + 1e-6))
    terms = mo.graph_terms64(att, ptr, order, 5, 6)
    np.testing.assert_allclose(terms[2], [1.4, mo.entropy64(att[[0, 2, 3]]).mean()])
    assert terms[1].tolist() == [0.0, 0.0]
