"""-m gpu: the MFMA GEMMs on every dispatch path (tests/gemm_path_cases.py), each case pinned to its kernel by `gsat_gemm_plan`.

Every operand lives inside a larger flat buffer with a leading dimension larger than its extent.  Guards and row padding of A and B are
NaN (an over-read that reaches an output shows without a fault); guards and padding of C and of the workspace hold a fixed bit pattern
that must be bit-identical after the call.  Two input regimes against an fp64 product computed on the device:

  exact   small integers: every partial sum is an integer below 2^24 and exact in bf16, so fp32 and split-bf16 MFMA results are exact in
          any summation order -> torch.equal.
  scaled  rows of A and columns of B scaled by 10^U(-3, 3): componentwise bound |C - ref|_ij <= g (|A||B|)_ij + n u (|A||B| + |bias| +
          |C0|)_ij with u = 2^-24 and n the number of additions of bias and C0 the call performs (0, 1 or 2; without either the
          bound is g |A||B| alone).  fp32 families g = 2 K u (the inner-product bound K u, doubled for the undocumented rounding
          inside the MFMA's k-pair); split families g = 2^-16 + 2 K u.  bf16 carries 8 significand bits: |lo| <= 2^-8 |x| and the
          rounding of lo leaves hi + lo within 2^-17 of x, so the four products lo*lo + lo*hi + hi*lo + hi*hi leave (1 + 2^-17)^2 - 1
          ~ 2^-16 of |a||b| per term for any data.  Derived, not measured.

Measured on an MI355X, worst err / (|A||B|) over the calls without bias and C0 (printed per test, recorded in DESIGN.md):
k_gemm_f32 1.9e-7, k_gemm_ws 4.5e-7, k_gemm_ws_x3 4.5e-6, k_gemm_bf16x3 1.16e-5 (at K = 4, where g = 1.574e-5).
"""
import ctypes

import pytest
import torch

from tests import gemm_path_cases as gc

pytestmark = pytest.mark.gpu

GUARD = 64                     # floats before and after every operand (256 bytes: offsets stay 16-byte aligned)
PATTERN = 0x7FC5A5A5           # a quiet NaN: C or workspace padding that is read into a sum shows up in the payload as well
U = 2.0 ** -24
WORST = {}                     # family -> worst err / (|A||B|) seen in the scaled regime on calls without bias and C0 (printed per test)
WORST_ALL = {}                 # family -> worst err / (|A||B| + |bias| + |C0|) over all scaled calls


class Region:
    """rows x cols payload at column offset `coff` of a rows x ld matrix, GUARD floats inside a flat fp32 device buffer."""

    def __init__(self, dev, rows, cols, form, fill):
        self.rows, self.cols = rows, cols
        self.ld, self.coff = (2 * _up4(cols), _up4(cols)) if form == "half" else (_up4(cols) + 8, 0)
        self.buf = torch.empty(2 * GUARD + max(rows * self.ld, 4), device=dev, dtype=torch.float32)
        if fill == "nan":
            self.buf.fill_(float("nan"))
        else:
            self.buf.view(torch.int32).fill_(PATTERN)
        self.view = self.buf[GUARD:GUARD + rows * self.ld].view(rows, self.ld)[:, self.coff:self.coff + cols]
        self.ptr = self.buf.data_ptr() + 4 * (GUARD + self.coff)
        assert self.ptr % 16 == 0 and self.ld % 4 == 0

    def snapshot(self):
        """int32 image of everything outside the payload (payload words zeroed)"""
        img = self.buf.view(torch.int32).clone()
        img[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, self.coff:self.coff + self.cols] = 0
        return img


def _up4(n):
    return (n + 3) // 4 * 4


def _plan(case, M, bias, acc, ldb):
    from dp_gsat_amd._lib import call
    out = (ctypes.c_int32 * 8)()
    call("gsat_gemm_plan", int(case.precision == "bf16x3"), case.a_t, case.b_t, M, case.N, case.K, int(bias), int(acc), ldb, out)
    return tuple(out)


def _inputs(regime, M, N, K, g, dev):
    """logical A [M, K], B [K, N], bias [N], C0 [M, N] as fp32 device tensors"""
    if regime == "exact":
        def ints(*shape):
            return torch.randint(-8, 9, shape, generator=g, device=dev).float()
        return ints(M, K), ints(K, N), ints(N), ints(M, N)
    def factor(n):
        return 10.0 ** (torch.rand(n, generator=g, device=dev) * 6.0 - 3.0)
    rf, cf = factor(M), factor(N)
    A = torch.randn(M, K, generator=g, device=dev) * rf[:, None]
    B = torch.randn(K, N, generator=g, device=dev) * cf[None, :]
    return A, B, torch.randn(N, generator=g, device=dev) * cf, torch.randn(M, N, generator=g, device=dev) * rf[:, None] * cf[None, :]


def run_call(dev, case, M, bias, acc, regime):
    from dp_gsat_amd._lib import call, load, stream
    N, K, a_t, b_t = case.N, case.K, case.a_t, case.b_t
    g = torch.Generator(device=dev).manual_seed(M * 7 + N * 3 + K + (1 << 20) * (regime == "exact"))
    A, B, bv, C0 = _inputs(regime, M, N, K, g, dev)
    rA = Region(dev, K if a_t else M, M if a_t else K, "pad", "nan")
    rB = Region(dev, N if b_t else K, K if b_t else N, case.b_form, "nan")
    rC = Region(dev, M, N, case.c_form, "pattern")
    rbias = Region(dev, 1, N, "pad", "nan")
    rA.view.copy_(A.t() if a_t else A)
    rB.view.copy_(B.t() if b_t else B)
    rbias.view.copy_(bv[None, :])
    if acc:
        rC.view.copy_(C0)
    plan = _plan(case, M, bias, acc, rB.ld)
    assert plan == case.plan, (case.name, M, plan, case.plan)
    wsf = int(load().gsat_gemm_workspace_floats(a_t, M, N, K))
    assert wsf == (plan[3] * M * N if plan[3] > 1 else 0)
    ws = torch.empty(2 * GUARD + wsf, device=dev, dtype=torch.float32)
    ws.view(torch.int32).fill_(PATTERN)
    c_before = rC.snapshot()
    call("gsat_gemm_bf16x3" if case.precision == "bf16x3" else "gsat_gemm_f32", a_t, b_t, M, N, K, rA.ptr, rA.ld, rB.ptr, rB.ld, rC.ptr, rC.ld,
         rbias.ptr if bias else None, int(acc), ws.data_ptr() + 4 * GUARD, wsf, stream())
    torch.cuda.synchronize()
    what = (case.name, regime, f"M={M} bias={bias} acc={acc}", f"plan={plan}")
    # ---- nothing outside the payload of C or outside the workspace was written ----
    assert torch.equal(rC.snapshot(), c_before), ("C guard / padding / other half changed",) + what
    wsi = ws.view(torch.int32)
    assert bool((wsi[:GUARD] == PATTERN).all()) and bool((wsi[GUARD + wsf:] == PATTERN).all()), ("workspace guard changed",) + what
    got = rC.view.double()
    assert not bool(torch.isnan(got).any()), ("NaN in the output: padding was read, or an element was not written",) + what
    # ---- fp64 reference ----
    A64, B64 = A.double(), B.double()
    ref = A64 @ B64
    extra = torch.zeros_like(ref)
    if bias:
        ref += bv.double()[None, :]
        extra += bv.double().abs()[None, :]
    if acc:
        ref += C0.double()
        extra += C0.double().abs()
    if regime == "exact":
        if not torch.equal(got, ref):
            bad = (got != ref).nonzero()
            r, c = (int(v) for v in bad[0])
            raise AssertionError(("exact sums differ", f"{len(bad)} elements, first at (row {r}, col {c}): got {got[r, c].item()} "
                                  f"expected {ref[r, c].item()}") + what)
        return
    absab = A64.abs() @ B64.abs()
    gfac = 2.0 * K * U + (2.0 ** -16 if plan[0] in (gc.TILE_X3, gc.WS_X3) else 0.0)
    err = (got - ref).abs()
    denom = absab + extra
    ratio = (err / denom).max().item()                 # denom == absab on a call without bias and C0
    WORST_ALL[plan[0]] = max(WORST_ALL.get(plan[0], 0.0), ratio)
    if not bias and not acc:
        WORST[plan[0]] = max(WORST.get(plan[0], 0.0), ratio)
    bound = gfac * absab + (int(bias) + int(acc)) * U * denom          # one u per addition of bias / C0 actually performed
    over = err > bound
    if bool(over.any()):
        r, c = (int(v) for v in over.nonzero()[0])
        raise AssertionError(("componentwise bound exceeded", f"{int(over.sum())} elements, first at (row {r}, col {c}): err {err[r, c].item():.3e} "
                              f"bound {bound[r, c].item():.3e}", f"worst err / (|A||B| + |bias| + |C0|) {ratio:.3e} against g = {gfac:.3e}") + what)


def run_case(dev, monkeypatch, case):
    monkeypatch.setenv("GSAT_GEMM_PRECISION", case.precision)
    if case.tile is None:
        monkeypatch.delenv("GSAT_GEMM_TILE", raising=False)
    else:
        monkeypatch.setenv("GSAT_GEMM_TILE", case.tile)
    failures = []                                      # every call of the case runs, so one miss does not hide the checks after it
    for M, bias, acc in case.runs:
        for regime in ("exact", "scaled"):
            try:
                run_call(dev, case, M, bias, acc, regime)
            except AssertionError as e:
                failures.append(e.args[0] if e.args else str(e))
    fam = case.plan[0]
    print(f"\nGEMM-RATIO {gc.FAMILY_NAMES[fam]} worst err/(|A||B|) so far {WORST.get(fam, 0.0):.3e}, with bias / C0 calls "
          f"err/(|A||B|+|bias|+|C0|) {WORST_ALL.get(fam, 0.0):.3e}  ({case.name})")
    assert not failures, failures


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", gc.TILE_CASES, ids=_ids(gc.TILE_CASES))
def test_tile_kernels(dev, monkeypatch, case):
    """k_gemm_f32 / k_gemm_bf16x3 in all four layouts x {64, 128}^2 tiles at a shape ragged in M, N and K, and at K = 4."""
    run_case(dev, monkeypatch, case)


@pytest.mark.parametrize("case", gc.SPLITK_CASES, ids=_ids(gc.SPLITK_CASES))
def test_split_k_and_slab_sums(dev, monkeypatch, case):
    """a_t = 1 products split over K into workspace slabs (ldo = N) and summed into C (ldc > N, also as the right half of a wider
    matrix) by the scalar, 4-, 8- and 16-lane sums, with and without accumulate."""
    run_case(dev, monkeypatch, case)


@pytest.mark.parametrize("case", gc.WS_CASES, ids=_ids(gc.WS_CASES))
def test_weight_stationary_kernels(dev, monkeypatch, case):
    """k_gemm_ws / k_gemm_ws_x3 in every geometry reachable on the grid, at the row threshold and around a 32-row tile edge, with
    strided A, B (b_t = 1: the right half of a [N, 2K] weight) and C, bias (fp32) or accumulate (split-bf16)."""
    run_case(dev, monkeypatch, case)
