"""Plain references of BatchNorm (with the fused PNA layer tail and the n_valid form) and of per-segment InstanceNorm, written from the
formulas so that N = 1 and n_valid are defined, plus the input recipe the normalisation tests share.  Every function casts its inputs
to ``dtype`` first: float64 is the reference, float32 the "plain fp32 evaluation of the same formula" whose own error the tests grant
as slack."""
from functools import lru_cache
from types import SimpleNamespace as NS
from typing import NamedTuple, Optional

import torch

EPS, MOMENTUM = 1e-5, 0.1


class BnRef(NamedTuple):
    y: torch.Tensor
    dx: Optional[torch.Tensor]
    dresidual: Optional[torch.Tensor]
    dgamma: Optional[torch.Tensor]
    dbeta: Optional[torch.Tensor]
    new_running_mean: torch.Tensor
    new_running_var: torch.Tensor


def counted(n_valid, N):
    return N if n_valid is None else min(max(int(n_valid), 0), N)


def bn_stats(x, running_mean, running_var, training=True, n_valid=None, dtype=torch.float64):
    """(mean, biased variance, M2, n) the normalisation uses: over the first clamp(n_valid, 0, N) rows in training (0 rows: mean 0,
    variance 0), the running statistics in eval."""
    x = x.to(dtype)
    n = counted(n_valid, x.shape[0])
    if not training:
        return running_mean.to(dtype), running_var.to(dtype), None, n
    xs = x[:n]
    mean = xs.sum(0) / max(n, 1)
    m2 = ((xs - mean) ** 2).sum(0)
    return mean, m2 / max(n, 1), m2, n


def _bn_parts(x, gamma, beta, running_mean, running_var, training, eps, relu, keep, p, n_valid, dy, dtype):
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean, var, m2, n = bn_stats(x, running_mean, running_var, training, n_valid, dtype)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    z = xhat * gamma + beta
    scale = (keep.to(dtype) if keep is not None else torch.ones_like(x)) / (1.0 - p)
    d = dz = None
    if dy is not None:
        d = dy.to(dtype) * scale                      # gradient behind the dropout = gradient of the residual branch
        d[n:] = 0
        dz = d * (z > 0).to(dtype) if relu else d
    return NS(x=x, gamma=gamma, beta=beta, mean=mean, var=var, m2=m2, n=n, rstd=rstd, xhat=xhat, z=z, scale=scale, d=d, dz=dz)


def bn_reference(x, gamma, beta, running_mean, running_var, training=True, momentum=MOMENTUM, eps=EPS, relu=False, residual=None,
                 keep=None, p=0.0, n_valid=None, dy=None, dtype=torch.float64) -> BnRef:
    """y = (relu(BN(x)) + residual) * keep / (1 - p) and its backward.  Statistics, backward sums and 1/n run over the first
    n = clamp(n_valid, 0, N) rows; the rows beyond get the forward formula with those statistics and exact-zero dx / dresidual.  The
    running variance takes the unbiased batch variance for n > 1 and the biased one (M2 / max(n, 1)) for n <= 1."""
    q = _bn_parts(x, gamma, beta, running_mean, running_var, training, eps, relu, keep, p, n_valid, dy, dtype)
    a = torch.relu(q.z) if relu else q.z
    if residual is not None:
        a = a + residual.to(dtype)
    y = a * q.scale
    rm, rv = running_mean.to(dtype), running_var.to(dtype)
    if training:
        ub = 1.0 / (q.n - 1) if q.n > 1 else 1.0 / max(q.n, 1)
        rm, rv = (1 - momentum) * rm + momentum * q.mean, (1 - momentum) * rv + momentum * q.m2 * ub
    if dy is None:
        return BnRef(y, None, None, None, None, rm, rv)
    dbeta, dgamma = q.dz.sum(0), (q.dz * q.xhat).sum(0)
    if training:
        inv = 1.0 / max(q.n, 1)
        dx = q.gamma * q.rstd * (q.dz - dbeta * inv - q.xhat * dgamma * inv)
    else:
        dx = q.gamma * q.rstd * q.dz
    dx[q.n:] = 0
    return BnRef(y, dx, q.d if residual is not None else None, dgamma, dbeta, rm, rv)


def bn_abs_sums(x, gamma, beta, running_mean, running_var, training=True, eps=EPS, relu=False, keep=None, p=0.0, n_valid=None,
                dy=None, dtype=torch.float64):
    """(sum |dy'|, sum |dy' xhat|) per column: the scale of the rounding error of any summation order of dbeta / dgamma."""
    q = _bn_parts(x, gamma, beta, running_mean, running_var, training, eps, relu, keep, p, n_valid, dy, dtype)
    return q.dz.abs().sum(0), (q.dz * q.xhat).abs().sum(0)


def _seg_mean(v, seg, cnt):
    return torch.zeros(cnt.shape[0], v.shape[1], dtype=v.dtype).index_add_(0, seg, v) / cnt


def instance_norm_reference(x, seg, G, eps=EPS, dy=None, dtype=torch.float64):
    """(y, dx) of the per-segment InstanceNorm with the biased variance; rows may come in any order (``seg`` = segment id per row)."""
    x, seg = x.to(dtype), seg.long()
    cnt = torch.bincount(seg, minlength=G).clamp_(min=1).to(dtype).view(-1, 1)
    xc = x - _seg_mean(x, seg, cnt)[seg]
    rstd = 1.0 / torch.sqrt(_seg_mean(xc * xc, seg, cnt) + eps)
    y = xc * rstd[seg]
    if dy is None:
        return y, None
    d = dy.to(dtype)
    return y, rstd[seg] * (d - _seg_mean(d, seg, cnt)[seg] - y * _seg_mean(d * y, seg, cnt)[seg])


def instance_norm_abs_sums(x, seg, G, eps=EPS, dy=None):
    """(sum |dy|, sum |dy y|) per (segment, column) cell."""
    y, _ = instance_norm_reference(x, seg, G, eps)
    d, one = dy.double(), torch.ones(G, 1, dtype=torch.float64)
    return _seg_mean(d.abs(), seg.long(), one), _seg_mean((d * y).abs(), seg.long(), one)


# ---- the shared input recipe --------------------------------------------------------------------------------------------------------------
STDS = (1e-3, 1e-2, 1.0, 10.0, 100.0)
GAMMA0_COL, CONST_COL, CONST = 1, 2, 0.5
MARGIN = 1e-3            # |gamma xhat + beta| of every counted element stays above this, so that fp32 and fp64 agree on the ReLU mask


def ratio_cap(n=None):
    """Largest |mean| / std of a column normalised over n rows: 100, cut to 3 sqrt(n) below 1112 rows.  An fp32 mean of a column at
    ratio r is off by about 2^-24 r std, which shifts every xhat of the column by 2^-24 r and dgamma by that times sum dy'.  Over many rows
    sum dy' is ~ sum |dy'| / sqrt(n) and the shift drowns; over a few rows it does not, and at ratio 100 a plain fp32 evaluation misses
    the reduction bound (SUM_TOL) by a factor 8 at n = 2 -- an unfair input, so the ratio follows sqrt(n).  Two rows
    normalise to +-1 from their difference alone, which may be a small part of one std: ratio 1 there."""
    return 100.0 if n is None else 1.0 if n <= 2 else min(100.0, 3.0 * n ** 0.5)


TWO_ROW_STD = 3e-3       # ~ sqrt(eps): see column_scales


def column_scales(C, n=None):
    """(std, offset) per column: stds cycle through STDS; offsets through {0, +1, -1, +r std, -r std} with r = ratio_cap(n), the +-1 cut
    to r std so that |mean| / std <= r <= 100 everywhere.  Twenty-five columns see every pair.
    Two rows (n <= 2) normalise to +-a with a^2 = var / (var + eps), and their dx is (1 - a^2) g rstd (dy'_1 - dy'_2) / 2: with var >> eps
    the factor 1 - a^2 = eps / (var + eps) is what rounding leaves of a^2 (0, 2^-24 or 2^-23 in fp32), and no fp32 evaluation resolves it.
    So the stds of a two-row batch or segment are cut to TWO_ROW_STD, where var ~ eps and the factor is ~ 1/2, and its rows are set
    to offset +- u std with u in [0.5, 1.5] (two_rows): two draws that happen to fall together would be a column at a high ratio."""
    c = torch.arange(C)
    s = torch.tensor(STDS, dtype=torch.float64)[c % 5]
    if n is not None and n <= 2:
        s = s.clamp(max=TWO_ROW_STD)
    kind = (c + c // 5) % 5
    r = ratio_cap(n)
    unit = torch.minimum(torch.ones_like(s), r * s)
    off = torch.stack([torch.zeros_like(s), unit, -unit, r * s, -r * s])[kind, c]
    return s, off


def two_rows(C, g):
    u = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    return torch.stack([u, -u])


def bn_inputs(N, C, seed, training=True, relu=False, n_valid=None):
    """fp32 inputs of one BatchNorm case (cached: treat as read-only).  Columns differ in scale and offset (column_scales); column
    CONST_COL is the constant 0.5; gamma is in [0.5, 1.5] with gamma[GAMMA0_COL] = 0; beta is normal with |beta| >= 0.05; the running
    statistics are near the columns' own, not equal.  Two adjustments keep the inputs fair to any fp32 implementation:
    - a column whose mean over the counted rows is below 0.02 std is shifted by 0.05 std (a relative bound on the mean needs a mean);
    - with relu, counted elements whose pre-activation is within MARGIN of 0 are moved away from it (the ReLU mask of an element on
      the edge is decided by rounding, and a flipped mask is a full-size difference in dx);
    - with relu, a column of which less than a tenth of its pre-activation range survives the ReLU gets its beta raised by half that
      range (y is judged relative to the column's largest entry; clipped to a sliver, that is not the scale y was computed at)."""
    return _bn_inputs(N, C, seed, bool(training), bool(relu), n_valid)


@lru_cache(maxsize=None)
def _bn_inputs(N, C, seed, training, relu, n_valid):
    g = torch.Generator().manual_seed(seed)
    n = counted(n_valid, N)
    s, off = column_scales(C, n if training else None)
    noise = torch.randn(N, C, generator=g, dtype=torch.float64)
    if training and n == 2:
        noise[:2] = two_rows(C, g)
    x = noise * s + off
    x[:, CONST_COL] = CONST
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[GAMMA0_COL] = 0.0
    beta = torch.randn(C, generator=g)
    beta = torch.where(beta.abs() < 0.05, torch.full_like(beta, 0.05), beta)
    rm = (off + 0.3 * s * torch.randn(C, generator=g, dtype=torch.float64)).float()
    rv = (s * s * (0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64))).float()
    residual = torch.randn(N, C, generator=g)
    dy = torch.randn(N, C, generator=g) * torch.tensor([1.0, 0.01, 10.0])[torch.arange(C) % 3]
    free = torch.ones(C, dtype=torch.bool)
    free[CONST_COL] = False
    if training and n > 0:
        low = (x[:n].mean(0).abs() < 0.02 * s) & free
        x[:, low] += 0.05 * s[low]
    x = x.float()
    if relu and n > 0:
        movable = free & (gamma != 0)
        z = _bn_parts(x, gamma, beta, rm, rv, training, EPS, False, None, 0.0, n_valid, None, torch.float64).z[:n]
        top, span = z.amax(0), z.abs().amax(0)
        beta = torch.where((top > 0) & (top < 0.1 * span), beta + (0.5 * span).float(), beta)
        for trip in range(40):
            q = _bn_parts(x, gamma, beta, rm, rv, training, EPS, False, None, 0.0, n_valid, None, torch.float64)
            near = q.z.abs() < MARGIN
            near[n:] = False
            if not near.any():
                break
            if trip < 20:          # move x by 3 MARGIN of pre-activation, away from the edge
                step = 3 * MARGIN / (q.gamma * q.rstd).abs().clamp_(min=1e-30) * torch.where(q.z * q.gamma >= 0, 1.0, -1.0)
                x = torch.where(near & movable, (x.double() + step).float(), x)
            if trip >= 20 or (near & ~movable).any():        # columns that x cannot move (constant, gamma = 0, two rows): move beta
                stuck = near.any(0) if trip >= 20 else (near & ~movable).any(0)
                beta = torch.where(stuck, beta + 4 * MARGIN, beta)
        else:
            raise AssertionError("bn_inputs: could not clear the ReLU edge")
    return NS(N=N, C=C, n=n, n_valid=n_valid, training=training, relu=relu, x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, residual=residual,
              dy=dy)


IN_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 100, 600, 0)


@lru_cache(maxsize=None)
def in_inputs(C, seed, permuted):
    """One batch with segments of IN_LENGTHS rows, each segment with the column recipe above under its own draw (cached: read-only).
    ``permuted``: the rows are shuffled, so the batch vector is unsorted and the kernels go through their order array."""
    g = torch.Generator().manual_seed(seed)
    scales = [column_scales(C, n if n <= 2 else None) for n in IN_LENGTHS]                   # two-row segments: see column_scales
    s, off = torch.stack([a for a, _ in scales]), torch.stack([b for _, b in scales])
    seg = torch.repeat_interleave(torch.arange(len(IN_LENGTHS)), torch.tensor(IN_LENGTHS))
    M = seg.shape[0]
    shrink = 1 - 0.2 * torch.rand(len(IN_LENGTHS), C, generator=g, dtype=torch.float64)      # per-segment offsets, still <= 100 std
    noise = torch.randn(M, C, generator=g, dtype=torch.float64)
    noise[seg == IN_LENGTHS.index(2)] = two_rows(C, g)
    x = noise * s[seg] + (off * shrink)[seg]
    x[:, CONST_COL] = CONST
    dy = torch.randn(M, C, generator=g) * torch.tensor([1.0, 0.01, 10.0])[torch.arange(C) % 3]
    if permuted:
        perm = torch.randperm(M, generator=g)
        x, dy, seg = x[perm], dy[perm], seg[perm]
    return NS(M=M, C=C, G=len(IN_LENGTHS), x=x.float().contiguous(), dy=dy.contiguous(), seg=seg.contiguous())


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------------
TOL = 1e-4               # tests/util.TOL
SUM_TOL = 1e-5           # column reductions: at most 53 fp32 adds in a chain (53 * 2^-24 = 3.2e-6 of sum |terms|), x3 for xhat's rounding


def column_bound(ref64, ref32):
    """Allowed |got - ref64| per column (dim 0 reduced; a [C] vector is C columns of one entry):
    TOL * max |ref64| + 4 * max |ref32 - ref64|."""
    r64 = ref64.reshape(-1, ref64.shape[-1]) if ref64.dim() else ref64.reshape(1, 1)
    r32 = ref32.double().reshape(r64.shape)
    return TOL * r64.abs().amax(0) + 4.0 * (r32 - r64).abs().amax(0)


def variance_from_rstd(rstd, eps=EPS):
    return rstd.detach().double().cpu() ** -2 - eps


def variance_bound(var64, mean64, eps=EPS):
    """rstd is judged as a variance: |rstd^-2 - eps - var64| <= 1e-5 var64 + 1e-6 mean64^2 (the fp32 floor of a centred sum)
    + 2^-20 (var64 + eps).  The last term is the fp32 rstd itself, which the first two forget: 1 / sqrtf(v + eps) carries the rounding of
    the sum (1/2 ulp, halved by the root), of sqrtf (<= 1 ulp) and of the division (<= 2.5 ulp), under 4 ulp = 2^-21 relative, twice
    that once squared.  It only matters where the variance is below eps (one row, a constant column, two close rows): there the first
    two terms can be 0 while no fp32 number is closer to 1 / sqrt(eps) than 1e-12 in these units."""
    return 1e-5 * var64 + 1e-6 * mean64 ** 2 + 2.0 ** -20 * (var64 + eps)


# ---- the shapes both the host fairness test and the GPU tests run ----------------------------------------------------------------------
ROW_SWEEP = (1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 2049, 8192, 8193, 16384, 16385, 20001)      # at C = 68
COL_SWEEP = (4, 60, 64, 68, 128, 132)                                                             # at N = 129
EVAL_ROWS = (1, 17, 8193)
TAIL_SHAPES = ((17, 4), (65, 68), (8193, 132))
BIG_SHAPE = (16400, 512)                          # N C / 4 > 8192 blocks x 256 threads: the element-wise grid-stride loops take a second trip
VALID_CAPACITY, VALID_C = 8193, 68
VALID_COUNTS = (0, 1, 63, 64, 65, 4100, 8192, 8193, 9000, -3)
DP_ROWS = (65, 8193)


def case_seed(N, C):
    return 7919 * N + C
