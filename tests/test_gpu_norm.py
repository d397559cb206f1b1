"""The normalisation kernels (csrc/norm.hip, the stand-alone InstanceNorm of csrc/attn.hip) against the fp64 references of
tests/norm_oracle.py, at the shapes where their loops branch: one row block and the cap of 256, the second trip and the clamped tail of
the 128-record partial sweeps, empty row slots, ragged column blocks, the second trip of the element-wise grid-stride loops, counts that
cut or skip whole blocks, segments around the 32 rows InstanceNorm keeps in registers.

How results are judged (tests/norm_oracle.py holds the numbers and their derivation; none is tuned to the kernels):
- element-wise outputs per column (InstanceNorm: per segment and column): |got - ref64| <= 1e-4 max|ref64| + 4 max|ref32 - ref64|, ref32
  being the same formulas evaluated in fp32 on the CPU; a column whose reference is identically 0 must be exactly 0;
- column reductions: |got - ref64| <= 1e-5 sum|terms|;
- rstd as a variance: |rstd^-2 - eps - var64| <= 1e-5 var64 + 1e-6 mean^2 + 2^-20 (var64 + eps).
The opt-out two-pass statistics (GSAT_BN_ONE_PASS=0, read once per process) are not run here: k_bn_partial<0/1> and k_bn_sum_finalize
are covered through gsat_bn_local_sum, k_bn_finalize<STAGE> is not."""
import pytest
import torch

from tests import norm_oracle as no
from tests.norm_oracle import EPS, MOMENTUM

pytestmark = pytest.mark.gpu

SEED, P = 0x5EED_1234_ABCD, 0.3


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def assert_columns(got, ref64, ref32, what):
    g = got.detach().double().cpu()
    assert g.shape == ref64.shape, f"{what}: shape {tuple(g.shape)} != {tuple(ref64.shape)}"
    if g.dim() == 1:
        g, ref64, ref32 = g[None], ref64[None], ref32[None]
    assert torch.isfinite(g).all(), f"{what}: not finite"
    bound = no.column_bound(ref64, ref32)
    err = (g - ref64).abs().amax(0)
    zero = ref64.abs().amax(0) == 0
    assert not g[:, zero].any(), f"{what}: columns {zero.nonzero().flatten().tolist()} must be exactly 0"
    bad = err > bound
    if bad.any():
        c = int((err / bound.clamp(min=1e-300)).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} columns out of bound; column {c}: err {float(err[c]):.3e} > {float(bound[c]):.3e} "
                             f"(max |ref| {float(ref64[:, c].abs().max()):.3e})")


def assert_sums(got, ref64, abs_sum, what):
    g = got.detach().double().cpu()
    err, bound = (g - ref64).abs(), no.SUM_TOL * abs_sum
    assert torch.isfinite(g).all(), f"{what}: not finite"
    bad = err > bound
    if bad.any():
        c = int((err / bound.clamp(min=1e-300)).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} columns out of bound; column {c}: err {float(err[c]):.3e} > {float(bound[c]):.3e}")


def assert_rstd(rstd, var64, mean64, what):
    err, bound = (no.variance_from_rstd(rstd) - var64).abs(), no.variance_bound(var64, mean64)
    bad = err > bound
    if bad.any():
        c = int((err / bound).argmax())
        raise AssertionError(f"{what}: column {c}: variance err {float(err[c]):.3e} > {float(bound[c]):.3e} (var {float(var64[c]):.3e})")


def keep_mask(dev, N, C, p, seed=SEED, stream_id=3):
    """The Philox keep mask the BatchNorm tail draws (stream 3, keyed by row and column), read back from the device."""
    from dp_gsat_amd._lib import call, ptr, stream
    keep = torch.ones(N, C, device=dev)
    if p > 0 and N > 0:
        call("gsat_philox_keep_mask", seed, stream_id, N, C, p, ptr(keep), stream())
    return keep


def run_bn(dev, inp, training=True, relu=False, tail=False, p=0.0, seed=0, seed_dev=None, n_valid=None, x=None):
    from dp_gsat_amd.ops import BatchNormFn
    from types import SimpleNamespace as NS
    xd = (inp.x if x is None else x).to(dev).requires_grad_(True)
    gd, bd = inp.gamma.to(dev).requires_grad_(True), inp.beta.to(dev).requires_grad_(True)
    rd = inp.residual.to(dev).requires_grad_(True) if tail else None
    rm, rv = inp.rm.to(dev), inp.rv.to(dev)
    nv = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int32, device=dev)
    y = BatchNormFn.apply(xd, gd, bd, rm, rv, training, MOMENTUM, EPS, relu, rd, p, seed, seed_dev, nv)
    mean, rstd = y.grad_fn.saved_tensors[3:5]
    y.backward(inp.dy.to(dev))
    torch.cuda.synchronize()
    return NS(y=y.detach(), dx=xd.grad, dresidual=rd.grad if tail else None, dgamma=gd.grad, dbeta=bd.grad, running_mean=rm,
              running_var=rv, save_mean=mean, save_rstd=rstd)


def check_bn(out, inp, what, training=True, relu=False, tail=False, p=0.0, keep=None, n_valid=None, x=None):
    x = inp.x if x is None else x
    args = (x, inp.gamma, inp.beta, inp.rm, inp.rv, training)
    kw = dict(relu=relu, keep=keep, p=p, n_valid=n_valid, dy=inp.dy)
    res = inp.residual if tail else None
    r64 = no.bn_reference(*args, residual=res, **kw)
    r32 = no.bn_reference(*args, residual=res, dtype=torch.float32, **kw)
    s1, s2 = no.bn_abs_sums(*args, **kw)
    m64, v64, _, _ = no.bn_stats(x, inp.rm, inp.rv, training, n_valid)
    m32, _, _, _ = no.bn_stats(x, inp.rm, inp.rv, training, n_valid, torch.float32)
    assert_columns(out.y, r64.y, r32.y, what + " y")
    assert_columns(out.dx, r64.dx, r32.dx, what + " dx")
    if tail:
        assert_columns(out.dresidual, r64.dresidual, r32.dresidual, what + " dresidual")
    assert_sums(out.dbeta, r64.dbeta, s1, what + " dbeta")
    assert_sums(out.dgamma, r64.dgamma, s2, what + " dgamma")
    assert_columns(out.save_mean, m64, m32, what + " save_mean")
    assert_rstd(out.save_rstd, v64, m64, what + " save_rstd")
    if training:
        assert_columns(out.running_mean, r64.new_running_mean, r32.new_running_mean, what + " running_mean")
        assert_columns(out.running_var, r64.new_running_var, r32.new_running_var, what + " running_var")
    else:
        assert torch.equal(out.running_mean.cpu(), inp.rm) and torch.equal(out.running_var.cpu(), inp.rv), what + ": eval moved the running statistics"
    return r64


def same_bytes(a, b, what):
    for k, v in vars(a).items():
        if v is not None:
            assert torch.equal(v, getattr(b, k)), f"{what}: {k} differs between two identical calls"


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("N", no.ROW_SWEEP)
def test_bn_row_sweep(dev, N, relu):
    """C = 68 (a full column block and a ragged one).  N <= 64 is one row block, 8193 reaches the second 128-record trip of the partial
    sweeps with a last block of one row, 16384 the cap of 256 blocks, 16385 RB = 253 != the 256 it was sized from, 20001 79 rows a block."""
    inp = no.bn_inputs(N, 68, no.case_seed(N, 68), True, relu)
    check_bn(run_bn(dev, inp, relu=relu), inp, f"N={N} relu={relu}", relu=relu)


@pytest.mark.parametrize("C", no.COL_SWEEP)
def test_bn_column_sweep(dev, C):
    inp = no.bn_inputs(129, C, no.case_seed(129, C), True, True)
    check_bn(run_bn(dev, inp, relu=True), inp, f"C={C}", relu=True)


@pytest.mark.parametrize("N", no.EVAL_ROWS)
def test_bn_eval_mode(dev, N):
    """Eval mode through the module: running statistics normalise and stay as they are, bit for bit, and so does num_batches_tracked."""
    from dp_gsat_amd.encoders import BatchNorm1d
    from types import SimpleNamespace as NS
    C = 68
    inp = no.bn_inputs(N, C, no.case_seed(N, C), False, True)
    bn = BatchNorm1d(C, eps=EPS, momentum=MOMENTUM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(inp.gamma); bn.bias.copy_(inp.beta); bn.running_mean.copy_(inp.rm); bn.running_var.copy_(inp.rv)
        bn.num_batches_tracked.fill_(7)
    bn.eval()
    xd = inp.x.to(dev).requires_grad_(True)
    y = bn(xd, fused_relu=True)
    mean, rstd = y.grad_fn.saved_tensors[3:5]
    y.backward(inp.dy.to(dev))
    torch.cuda.synchronize()
    out = NS(y=y.detach(), dx=xd.grad, dresidual=None, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
             running_var=bn.running_var, save_mean=mean, save_rstd=rstd)
    check_bn(out, inp, f"eval N={N}", training=False, relu=True)
    assert int(bn.num_batches_tracked) == 7
    assert torch.equal(mean.cpu(), inp.rm)


@pytest.mark.parametrize("N,C,p", [(N, C, p) for N, C in no.TAIL_SHAPES for p in (0.0, P)] + [no.BIG_SHAPE + (P,)])
def test_bn_fused_tail(dev, N, C, p):
    """y = dropout(relu(BN(x)) + residual); the seed word on the device draws the same mask as the seed by value.  (16400, 512) is the
    one shape whose N C / 4 float4 items exceed the 8192 x 256 threads of the element-wise grid: the grid-stride loops of k_bn_apply and
    k_bn_bwd_apply take their second trip there."""
    inp = no.bn_inputs(N, C, no.case_seed(N, C), True, True)
    keep = keep_mask(dev, N, C, p)
    if p > 0 and N * C >= 1 << 20:
        assert abs(float(keep.mean()) - (1 - p)) < 0.01
    out = run_bn(dev, inp, relu=True, tail=True, p=p, seed=SEED)
    check_bn(out, inp, f"tail N={N} C={C} p={p}", relu=True, tail=True, p=p, keep=keep.cpu())
    sd = torch.tensor([SEED], dtype=torch.int64, device=dev)
    same_bytes(out, run_bn(dev, inp, relu=True, tail=True, p=p, seed=0, seed_dev=sd), "seed_dev")


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("n_valid", no.VALID_COUNTS)
def test_bn_n_valid(dev, n_valid, tail):
    """Capacity 8193 rows (129 blocks of 64): counts that leave every block empty, cut the first block, end on a block edge, leave 64
    whole blocks uncounted, and counts from outside [0, N] (clamped).  The rows beyond the count must not move any output of the
    counted rows: three calls that differ only in those rows of x (the recipe's, 1e30, -2e30) agree bit for bit."""
    N, C = no.VALID_CAPACITY, no.VALID_C
    p = P if tail else 0.0
    inp = no.bn_inputs(N, C, no.case_seed(N, C), True, tail, n_valid)
    n = inp.n
    keep = keep_mask(dev, N, C, p)
    kw = dict(relu=tail, tail=tail, p=p, seed=SEED, n_valid=n_valid)
    out = run_bn(dev, inp, **kw)
    what = f"n_valid={n_valid} tail={tail}"
    ref = check_bn(out, inp, what, relu=tail, tail=tail, p=p, keep=keep.cpu(), n_valid=n_valid)
    assert not out.dx[n:].any(), what + ": dx beyond the count must be exactly 0"
    assert not tail or not out.dresidual[n:].any(), what + ": dresidual beyond the count must be exactly 0"
    assert not ref.dx[n:].any()
    for fill in (1e30, -2e30):
        x = inp.x.clone()
        x[n:] = fill
        other = run_bn(dev, inp, x=x, **kw)
        assert torch.equal(other.y[:n], out.y[:n]), what + f": padding rows of {fill} moved y"
        for k in ("dx", "dresidual", "dgamma", "dbeta", "running_mean", "running_var", "save_mean", "save_rstd"):
            if getattr(out, k) is not None:
                assert torch.equal(getattr(other, k), getattr(out, k)), what + f": padding rows of {fill} moved {k}"


@pytest.mark.parametrize("N", [8193, 16385])
def test_bn_bitwise_repeatable(dev, N):
    inp = no.bn_inputs(N, 68, no.case_seed(N, 68), True, True)
    kw = dict(relu=True, tail=True, p=P, seed=SEED)
    same_bytes(run_bn(dev, inp, **kw), run_bn(dev, inp, **kw), f"N={N}")


def test_bn_one_row_is_pinned(dev):
    """N = 1 in training, which torch refuses: the batch variance is 0, so rstd = 1 / sqrt(eps), xhat = 0, y = act(beta), every input
    gradient is exactly 0, dbeta = dy'.  The running variance takes the BIASED variance of the row (0): running_var <- (1 - m)
    running_var -- the kernels switch from 1 / (n - 1) to 1 / n at n <= 1 instead of dividing by 0.  A model fed single-row batches would
    see its running variance decay towards 0; nothing in the project does that, so the behaviour is pinned, not changed."""
    for relu in (False, True):
        inp = no.bn_inputs(1, 68, no.case_seed(1, 68), True, relu)
        out = run_bn(dev, inp, relu=relu)
        act = torch.relu(inp.beta) if relu else inp.beta
        assert torch.equal(out.y[0].cpu(), act)
        assert torch.equal(out.save_mean.cpu(), inp.x[0])
        r = out.save_rstd.double().cpu()
        assert float((r - EPS ** -0.5).abs().max()) <= 4 * 2.0 ** -23 * EPS ** -0.5 and float(r.min()) == float(r.max())
        assert not out.dx.any() and not out.dgamma.any()
        assert torch.equal(out.dbeta.cpu(), inp.dy[0] * (act > 0).float() if relu else inp.dy[0])
        rv = (1 - MOMENTUM) * inp.rv.double()
        assert float(((out.running_var.double().cpu() - rv).abs() / rv).max()) <= 2.0 ** -22


def test_bn_argument_errors_launch_nothing(dev):
    """C % 4 != 0 is GSAT_ERR_UNSUPPORTED (-4), dropout_p = 1 and a null row count to the _valid entry points GSAT_ERR_ARG (-2); the
    outputs keep their bytes."""
    from dp_gsat_amd._lib import GsatHipError, call, load, ptr, stream
    N = 8
    nv = torch.tensor([N], dtype=torch.int32, device=dev)

    def attempt(C, p, valid, n_valid, code):
        x, dy = torch.randn(N, C, device=dev), torch.randn(N, C, device=dev)
        g, b, rm, rv = torch.ones(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.ones(C, device=dev)
        outs = [torch.full((N, C), 7.0, device=dev) for _ in range(2)] + [torch.full((C,), 7.0, device=dev) for _ in range(4)]
        y, dx, mean, rstd, dg, db = outs
        ws = torch.empty(max(int(load().gsat_bn_workspace_floats(N, C)), 1), device=dev)
        fwd = (ptr(x), ptr(g), ptr(b), ptr(rm), ptr(rv), N, C, 1, MOMENTUM, EPS, 1, None, p, 1, None, ptr(y), ptr(mean), ptr(rstd), ptr(ws))
        bwd = (ptr(x), ptr(dy), ptr(g), ptr(b), ptr(mean), ptr(rstd), N, C, 1, 1, p, 1, None, ptr(dx), None, ptr(dg), ptr(db), ptr(ws))
        tail = (n_valid, stream()) if valid else (stream(),)
        suffix = "_valid" if valid else ""
        for name, a in (("gsat_bn_act_fwd" + suffix, fwd), ("gsat_bn_act_bwd" + suffix, bwd)):
            with pytest.raises(GsatHipError, match=rf"code {code}\)"):
                call(name, *a, *tail)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in outs) and not rm.any() and bool((rv == 1).all())

    attempt(6, 0.0, False, None, -4)
    attempt(6, 0.0, True, ptr(nv), -4)
    attempt(8, 1.0, False, None, -2)
    attempt(8, 1.0, True, ptr(nv), -2)
    attempt(8, 0.0, True, None, -2)


# ---- the data-parallel pieces, called directly ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["one", "none", "third"])
@pytest.mark.parametrize("N", no.DP_ROWS)
def test_bn_data_parallel_pieces(dev, N, split):
    """One [N, 68] tensor cut into two row shards, the [C] vectors of the shards added with torch where a process group would all-reduce:
    gsat_bn_local_sum (plain, then centred), gsat_bn_apply_fwd, gsat_bn_local_bwd_sums, gsat_bn_apply_bwd with the row count on the
    device.  An empty shard returns zeros and is given no buffer it could write."""
    from dp_gsat_amd._lib import call, load, ptr, stream
    C, p = 68, P
    first = {"one": 1, "none": 0, "third": N // 3}[split]
    inp = no.bn_inputs(N, C, no.case_seed(N, C), True, True)
    bounds = [(0, first), (first, N)]
    gd, bd = inp.gamma.to(dev), inp.beta.to(dev)
    shards = [NS_shard(inp, a, b, dev) for a, b in bounds]
    ws = torch.empty(int(load().gsat_bn_workspace_floats(N, C)), device=dev)

    def local(name, make_args, count):
        total = []
        for s in shards:
            outs = [torch.full((C,), float("nan"), device=dev) for _ in range(count)]
            call(name, *make_args(s, outs), ptr(ws) if s.n else None, stream())
            total.append(outs)
        for outs, s in zip(total, shards):
            assert s.n or not any(bool(o.any()) for o in outs), name + ": an empty shard must return zeros"
        return [sum(o[i] for o in total) for i in range(count)]

    (sx,) = local("gsat_bn_local_sum", lambda s, o: (ptr(s.x), None, s.n, C, ptr(o[0])), 1)
    x64 = inp.x.double()
    assert_sums(sx, x64.sum(0), x64.abs().sum(0), "sum x")
    mean = sx / N
    (q,) = local("gsat_bn_local_sum", lambda s, o: (ptr(s.x), ptr(mean), s.n, C, ptr(o[0])), 1)
    q64 = ((x64 - mean.double().cpu()) ** 2).sum(0)                   # the same operation: centred on the centre it was given
    assert_sums(q, q64, q64, "sum (x - centre)^2")
    rstd = torch.rsqrt(q / N + EPS)
    m64, v64, _, _ = no.bn_stats(inp.x, inp.rm, inp.rv)
    assert_rstd(rstd, v64, m64, "rstd")
    keep = torch.cat([keep_mask(dev, s.n, C, p) for s in shards])
    for s in shards:
        s.y = torch.full((s.n, C), float("nan"), device=dev)
        call("gsat_bn_apply_fwd", ptr(s.x), ptr(gd), ptr(bd), ptr(mean), ptr(rstd), s.n, C, 1, ptr(s.res), p, SEED, None, ptr(s.y), stream())
    sdy, sdyx = local("gsat_bn_local_bwd_sums", lambda s, o: (ptr(s.x), ptr(s.dy), ptr(gd), ptr(bd), ptr(mean), ptr(rstd), s.n, C, 1, p,
                                                              SEED, None, ptr(o[0]), ptr(o[1])), 2)
    rows = torch.tensor([float(N)], device=dev)
    for s in shards:
        s.dx, s.dres = torch.full((s.n, C), float("nan"), device=dev), torch.full((s.n, C), float("nan"), device=dev)
        call("gsat_bn_apply_bwd", ptr(s.x), ptr(s.dy), ptr(gd), ptr(bd), ptr(mean), ptr(rstd), ptr(sdy), ptr(sdyx), 0, ptr(rows), s.n, C, 1,
             p, SEED, None, ptr(s.dx), ptr(s.dres), stream())
    torch.cuda.synchronize()
    args = (inp.x, inp.gamma, inp.beta, inp.rm, inp.rv, True)
    kw = dict(relu=True, keep=keep.cpu(), p=p, dy=inp.dy)
    r64 = no.bn_reference(*args, residual=inp.residual, **kw)
    r32 = no.bn_reference(*args, residual=inp.residual, dtype=torch.float32, **kw)
    s1, s2 = no.bn_abs_sums(*args, **kw)
    what = f"N={N} shards {bounds}:"
    assert_columns(torch.cat([s.y for s in shards]), r64.y, r32.y, what + " y")
    assert_columns(torch.cat([s.dx for s in shards]), r64.dx, r32.dx, what + " dx")
    assert_columns(torch.cat([s.dres for s in shards]), r64.dresidual, r32.dresidual, what + " dresidual")
    assert_sums(sdy, r64.dbeta, s1, what + " dbeta")
    assert_sums(sdyx, r64.dgamma, s2, what + " dgamma")


def NS_shard(inp, a, b, dev):
    from types import SimpleNamespace as NS
    cut = lambda t: t[a:b].contiguous().to(dev) if b > a else None
    return NS(n=b - a, x=cut(inp.x), dy=cut(inp.dy), res=cut(inp.residual))


# ---- InstanceNorm ------------------------------------------------------------------------------------------------------------------------
def check_cells(got, ref64, ref32, seg, G, what):
    for g in range(G):
        rows = seg == g
        if rows.any():
            assert_columns(got[rows], ref64[rows], ref32[rows], f"{what} segment {g} ({int(rows.sum())} rows)")


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("C", [4, 60, 64, 68, 132])
def test_instance_norm_segments(dev, C, permuted):
    """Segments of 0, 1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 100 and 600 rows: empty row slots, exactly the 32 rows k_seg_stats keeps in
    registers, one more, and tails it re-reads; sorted rows and shuffled ones (the order array).  The last segment is empty and lies
    beyond batch.max(), so the module sees 13 segments; test_instance_norm_writes_in_place passes all 14."""
    import dp_gsat_amd as G
    inp = no.in_inputs(C, 100 + C, permuted)
    y64, dx64 = no.instance_norm_reference(inp.x, inp.seg, inp.G, EPS, inp.dy)
    y32, dx32 = no.instance_norm_reference(inp.x, inp.seg, inp.G, EPS, inp.dy, torch.float32)
    xd = inp.x.to(dev).requires_grad_(True)
    y = G.InstanceNorm(C)(xd, inp.seg.to(dev))
    y.backward(inp.dy.to(dev))
    torch.cuda.synchronize()
    what = f"C={C} permuted={permuted}:"
    check_cells(y.detach().cpu(), y64, y32, inp.seg, inp.G, what + " y")
    check_cells(xd.grad.cpu(), dx64, dx32, inp.seg, inp.G, what + " dx")
    single = inp.seg == no.IN_LENGTHS.index(1)
    assert not y.detach().cpu()[single].any() and not xd.grad.cpu()[single].any(), what + " a one-row segment normalises to exactly 0"


@pytest.mark.parametrize("permuted", [False, True])
def test_instance_norm_writes_in_place(dev, permuted):
    """Every buffer of the two C entry points sits between NaN guards: inputs (a read out of place would bring NaN into the outputs),
    outputs and the statistics (a write out of place would overwrite a guard).  All 14 segments are passed, the empty ones included."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.get_model import _SegmentCache
    C, pad = 68, 64
    inp = no.in_inputs(C, 100 + C, permuted)
    M, G = inp.M, inp.G
    sptr, order, seg32, G_, _ = _SegmentCache().get(inp.seg.to(dev), num_seg=G)
    assert G_ == G

    def guarded(rows, src=None):
        buf = torch.full((rows + 2 * pad, C), float("nan"), device=dev)
        if src is not None:
            buf[pad:pad + rows] = src.to(dev)
        return buf, buf[pad:pad + rows]

    xb, x = guarded(M, inp.x)
    db, dy = guarded(M, inp.dy)
    yb, y = guarded(M)
    gb, dx = guarded(M)
    sb, stats = guarded(2 * G)
    wb, ws = guarded(2 * G)
    call("gsat_instance_norm_fwd", ptr(x), ptr(sptr), ptr(order), ptr(seg32), M, G, C, ptr(y), ptr(stats), stream())
    call("gsat_instance_norm_bwd", ptr(y), ptr(dy), ptr(stats), ptr(sptr), ptr(order), ptr(seg32), M, G, C, ptr(dx), ptr(ws), stream())
    torch.cuda.synchronize()
    for name, buf, rows in (("x", xb, M), ("dy", db, M), ("y", yb, M), ("dx", gb, M), ("stats", sb, 2 * G), ("workspace", wb, 2 * G)):
        assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + rows:]).all(), f"{name}: a guard row was written"
        assert torch.isfinite(buf[pad:pad + rows]).all(), f"{name}: NaN inside"
    y64, dx64 = no.instance_norm_reference(inp.x, inp.seg, G, EPS, inp.dy)
    y32, dx32 = no.instance_norm_reference(inp.x, inp.seg, G, EPS, inp.dy, torch.float32)
    check_cells(y.cpu(), y64, y32, inp.seg, G, "y")
    check_cells(dx.cpu(), dx64, dx32, inp.seg, G, "dx")
    empty = [g for g, n in enumerate(no.IN_LENGTHS) if n == 0]
    mean = stats.reshape(2, G, C)[0].cpu()
    assert not mean[empty].any(), "an empty segment has mean 0"


# ---- ReLU + dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, P])
@pytest.mark.parametrize("N,C", [(1, 4), (16383, 512), (16400, 512)])
def test_relu_dropout_grid_stride(dev, N, C, p):
    """N C / 4 = 2 097 024 items fit the 8192 x 256 threads of the element-wise grid, 2 099 200 need the loop's second trip.  On
    strictly positive inputs the keep mask is y > 0; it must be the Philox mask of stream 5.  Signed inputs then check the ReLU."""
    from dp_gsat_amd.ops import ReluDropout, relu_dropout
    g = torch.Generator().manual_seed(N + C)
    s = 1.0 / (1.0 - p)
    dy = torch.randn(N, C, generator=g).to(dev)
    pos = (torch.rand(N, C, generator=g) + 0.1).to(dev).requires_grad_(True)
    y = relu_dropout(pos, p, True)
    keep = (y > 0).float()
    if N * C >= 1 << 20:
        assert abs(float(keep.mean()) - (1 - p)) < 0.01
    if p == 0:
        assert bool(keep.all())
    assert torch.allclose(y, pos.detach() * keep * s, rtol=1e-6, atol=0)
    y.backward(dy)
    assert torch.allclose(pos.grad, dy * keep * s, rtol=1e-6, atol=0)
    x = (torch.randn(N, C, generator=g) * 3).to(dev).requires_grad_(True)
    keep = keep_mask(dev, N, C, p, SEED, 5)
    y = ReluDropout.apply(x, p, SEED, None)
    assert torch.allclose(y, torch.relu(x.detach()) * keep * s, rtol=1e-6, atol=0)
    y.backward(dy)
    assert torch.allclose(x.grad, dy * keep * (x.detach() > 0).float() * s, rtol=1e-6, atol=0)
    sd = torch.tensor([SEED], dtype=torch.int64, device=dev)
    assert torch.equal(ReluDropout.apply(x.detach(), p, 0, sd), y.detach())
