"""The normalisation references of tests/norm_oracle.py against torch in fp64 (what makes them trustworthy), and the shared input recipe
against the bounds of the GPU tests: a plain fp32 evaluation of the formulas must sit inside every bound with a factor 4 to spare, or the
input would be unfair to any fp32 kernel."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ops as oops
from tests import norm_oracle as no


def _rel(a, b):
    if a.numel() == 0:
        return 0.0 if a.shape == b.shape else 1.0
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu,tail", [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize("N,C", [(2, 4), (17, 8), (300, 12)])
def test_bn_reference_matches_torch_autograd(N, C, relu, tail, training):
    g = torch.Generator().manual_seed(100 * N + C)
    x = torch.randn(N, C, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    rm0, rv0 = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    res = torch.randn(N, C, generator=g, dtype=torch.float64) if tail else None
    p = 0.3 if tail else 0.0
    keep = (torch.rand(N, C, generator=g) > p).double() if tail else None
    dy = torch.randn(N, C, generator=g, dtype=torch.float64)
    xt, gt, bt = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rt = res.clone().requires_grad_(True) if tail else None
    rm, rv = rm0.clone(), rv0.clone()
    yt = F.batch_norm(xt, rm, rv, gt, bt, training, 0.1, 1e-5)
    yt = torch.relu(yt) if relu else yt
    if tail:
        yt = (yt + rt) * keep / (1 - p)
    yt.backward(dy)
    ref = no.bn_reference(x, gamma, beta, rm0, rv0, training, 0.1, 1e-5, relu, res, keep, p, None, dy)
    pairs = [(ref.y, yt), (ref.dx, xt.grad), (ref.dgamma, gt.grad), (ref.dbeta, bt.grad), (ref.new_running_mean, rm),
             (ref.new_running_var, rv)] + ([(ref.dresidual, rt.grad)] if tail else [])
    for i, (a, b) in enumerate(pairs):
        assert _rel(a, b.detach()) <= 1e-12, (i, _rel(a, b.detach()))
    if not training:
        assert torch.equal(ref.new_running_mean, rm0) and torch.equal(ref.new_running_var, rv0)


@pytest.mark.parametrize("n_valid", [1, 2, 37, 64, 100, 130, -3])
@pytest.mark.parametrize("tail", [False, True])
def test_bn_reference_n_valid_is_the_plain_form_on_the_counted_rows(n_valid, tail):
    N, C = 100, 8
    inp = no.bn_inputs(N, C, 5, True, tail, n_valid)
    n = no.counted(n_valid, N)
    assert n == inp.n
    keep = (torch.rand(N, C, generator=torch.Generator().manual_seed(1)) > 0.3).float() if tail else None
    p = 0.3 if tail else 0.0
    res = inp.residual if tail else None
    full = no.bn_reference(inp.x, inp.gamma, inp.beta, inp.rm, inp.rv, True, 0.1, 1e-5, tail, res, keep, p, n_valid, inp.dy)
    cut = no.bn_reference(inp.x[:n], inp.gamma, inp.beta, inp.rm, inp.rv, True, 0.1, 1e-5, tail, res[:n] if tail else None,
                          keep[:n] if tail else None, p, None, inp.dy[:n])
    for a, b in zip(full, cut):
        if a is None:
            assert b is None
        else:
            assert _rel(a[:n] if a.dim() == 2 else a, b) <= 1e-13
    assert not full.dx[n:].any() and (not tail or not full.dresidual[n:].any())
    # rows beyond the count: the forward formula with the counted rows' statistics
    mean, var, _, _ = no.bn_stats(inp.x, inp.rm, inp.rv, True, n_valid)
    z = (inp.x.double() - mean) / torch.sqrt(var + 1e-5) * inp.gamma.double() + inp.beta.double()
    y = ((torch.relu(z) + res.double()) * keep.double() / (1 - p)) if tail else z
    assert _rel(full.y, y) <= 1e-12


def test_bn_reference_pins_the_degenerate_counts():
    """n = 1: variance 0, y = act(beta), running_var <- (1 - m) running_var (the biased variance of one row is 0); n = 0: mean 0 too."""
    inp = no.bn_inputs(5, 8, 3, True, True, None)
    one = no.bn_reference(inp.x[:1], inp.gamma, inp.beta, inp.rm, inp.rv, True, 0.1, 1e-5, True, dy=inp.dy[:1])
    assert torch.equal(one.y[0], torch.relu(inp.beta.double()))
    assert torch.equal(one.new_running_var, 0.9 * inp.rv.double()) and not one.dx.any() and not one.dgamma.any()
    none = no.bn_reference(inp.x, inp.gamma, inp.beta, inp.rm, inp.rv, True, 0.1, 1e-5, True, n_valid=0, dy=inp.dy)
    assert torch.equal(none.new_running_mean, 0.9 * inp.rm.double()) and torch.equal(none.new_running_var, 0.9 * inp.rv.double())
    assert not none.dx.any() and not none.dgamma.any() and not none.dbeta.any()


@pytest.mark.parametrize("permuted", [False, True])
def test_instance_norm_reference_matches_the_oracle(permuted):
    inp = no.in_inputs(8, 11, permuted)
    x = torch.randn(inp.M, 8, generator=torch.Generator().manual_seed(2), dtype=torch.float64).requires_grad_(True)
    yo = oops.instance_norm(x, inp.seg, inp.G)
    yo.backward(inp.dy.double())
    y, dx = no.instance_norm_reference(x.detach(), inp.seg, inp.G, 1e-5, inp.dy)
    assert _rel(y, yo.detach()) <= 1e-12 and _rel(dx, x.grad) <= 1e-12
    single = inp.seg == no.IN_LENGTHS.index(1)
    assert int(single.sum()) == 1 and not y[single].any() and not dx[single].any()


# ---- the input recipe is fair ---------------------------------------------------------------------------------------------------------
def _bn_cases():
    cases = [(N, 68, True, relu, False, None) for N in no.ROW_SWEEP for relu in (False, True)]
    cases += [(129, C, True, True, False, None) for C in no.COL_SWEEP]
    cases += [(N, 68, False, True, False, None) for N in no.EVAL_ROWS]
    cases += [(N, C, True, True, True, None) for N, C in no.TAIL_SHAPES + (no.BIG_SHAPE,)]
    cases += [(no.VALID_CAPACITY, no.VALID_C, True, tail, tail, nv) for nv in no.VALID_COUNTS for tail in (False, True)]
    return cases


@pytest.mark.parametrize("N,C,training,relu,tail,n_valid", _bn_cases())
def test_bn_recipe_is_fair_to_fp32(N, C, training, relu, tail, n_valid):
    inp = no.bn_inputs(N, C, no.case_seed(N, C), training, relu, n_valid)
    s, off = no.column_scales(C, no.counted(n_valid, N) if training else None)
    assert float((off.abs() / s).max()) <= 100.0 and (N < 1112 or n_valid is not None or float((off.abs() / s).max()) == 100.0)
    assert bool((inp.x[:, no.CONST_COL] == no.CONST).all()) and float(inp.gamma[no.GAMMA0_COL]) == 0.0
    assert float(inp.gamma.min()) >= 0.0 and float(inp.gamma.max()) <= 1.5
    args = (inp.x, inp.gamma, inp.beta, inp.rm, inp.rv, training)
    kw = dict(relu=relu, residual=inp.residual if tail else None, n_valid=n_valid, dy=inp.dy)
    r64, r32 = no.bn_reference(*args, **kw), no.bn_reference(*args, **kw, dtype=torch.float32)
    kw.pop("residual")
    s1, s2 = no.bn_abs_sums(*args, **kw)
    assert bool(((r32.dbeta.double() - r64.dbeta).abs() <= no.SUM_TOL * s1 / 4).all()), "dbeta"
    err, bound = (r32.dgamma.double() - r64.dgamma).abs(), no.SUM_TOL * s2 / 4
    assert bool((err <= bound).all()), ("dgamma", float((err / bound.clamp(min=1e-300)).max()))
    m64, v64, _, n = no.bn_stats(inp.x, inp.rm, inp.rv, training, n_valid)
    _, v32, _, _ = no.bn_stats(inp.x, inp.rm, inp.rv, training, n_valid, torch.float32)
    got = no.variance_from_rstd(1.0 / torch.sqrt(v32 + torch.tensor(1e-5)))
    assert bool(((got - v64).abs() <= no.variance_bound(v64, m64) / 4).all()), "variance"
    if relu and n > 0:          # both precisions see the same ReLU mask
        z64 = (inp.x.double() - m64) / torch.sqrt(v64 + 1e-5) * inp.gamma.double() + inp.beta.double()
        assert float(z64[:n].abs().min()) >= no.MARGIN / 2
        assert torch.equal(r32.y[:n] > 0, r64.y[:n] > 0) or tail
        top, span = z64[:n].amax(0), z64[:n].abs().amax(0)          # no column is clipped to a sliver: all of it, or a tenth at least
        assert bool(((top < 0) | (top >= 0.1 * span)).all())
    if training and n > 0:      # a relative bound on the batch mean needs a mean
        free = torch.ones(C, dtype=torch.bool)
        free[no.CONST_COL] = False
        assert bool((m64.abs() >= 0.01 * s)[free].all())


@pytest.mark.parametrize("C", [4, 60, 64, 68, 132])
@pytest.mark.parametrize("permuted", [False, True])
def test_instance_norm_recipe_is_fair_to_fp32(C, permuted):
    inp = no.in_inputs(C, 100 + C, permuted)
    assert tuple(torch.bincount(inp.seg, minlength=inp.G).tolist()) == no.IN_LENGTHS
    assert bool((inp.seg[1:] >= inp.seg[:-1]).all()) != permuted
    y64, dx64 = no.instance_norm_reference(inp.x, inp.seg, inp.G, 1e-5, inp.dy)
    y32, dx32 = no.instance_norm_reference(inp.x, inp.seg, inp.G, 1e-5, inp.dy, torch.float32)
    assert torch.isfinite(y32).all() and torch.isfinite(dx32).all()
    # the cells whose reference is identically 0 are the length-1 segments (every column) and the constant column (y only)
    single = inp.seg == no.IN_LENGTHS.index(1)
    assert not y64[single].any() and not dx64[single].any() and not y32[single].any() and not dx32[single].any()
    assert not y64[:, no.CONST_COL].any() and not y32[:, no.CONST_COL].any()
