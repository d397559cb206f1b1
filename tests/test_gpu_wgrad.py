"""-m gpu: the streaming split-bf16 weight gradient (csrc/gemm.hip: k_wgrad_x3, entry gsat_gemm_wgrad_x3) against an fp64 product computed
on the device, in the buffer style of tests/test_gpu_gemm_paths.py: A [K, Mo] and B [K, No] sit inside larger flat buffers whose column
padding, guards and 32 further rows beyond K are NaN; the padding of C (ldc = No + 8, or C as the right half of a [Mo, 2 No] matrix) and
the guards of the workspace hold a fixed bit pattern that must be unchanged after the call.

  exact   integers in [-8, 8]: every partial sum is an integer below 2^24 and exact in bf16 -> torch.equal in any summation order.
  scaled  rows and columns scaled by 10^U(-3, 3): |C - ref|_ij <= (2^-16 + 2 K 2^-24) (|A||B|)_ij, the split-bf16 bound of
          tests/test_gpu_gemm_paths.py (2^-16 from the hi/lo split of both operands, 2 K u for K fp32 additions in any order; derived, not
          measured).  The ordered sum over the S partial tiles is part of those K additions.

S, the rows per range and the eligibility threshold are read from gsat_gemm_wgrad_plan; the K of every case is found by asking the plan.
"""
import ctypes

import pytest
import torch

from tests.test_gpu_gemm_paths import GUARD, PATTERN, U, Region, _inputs

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128), (128, 256), (256, 128)]          # one tile, two column tiles, two row tiles
EXTRA_ROWS = 32                                        # NaN rows of A and B beyond K


def plan(Mo, No, K):
    from dp_gsat_amd._lib import call
    out = (ctypes.c_int32 * 4)()
    call("gsat_gemm_wgrad_plan", Mo, No, K, out)
    return tuple(out)                                  # (eligible, S, rows per range, workspace floats)


def smallest_eligible_k(Mo, No):
    lo, hi = 4, 1 << 24                                # eligibility is monotone in K: bisect over multiples of 4
    assert plan(Mo, No, hi)[0] == 1 and plan(Mo, No, lo)[0] == 0
    while hi - lo > 4:
        mid = (lo + hi) // 8 * 4
        if plan(Mo, No, mid)[0]:
            hi = mid
        else:
            lo = mid
    return hi


def first_k(Mo, No, start, pred):
    """first K > start (multiples of 4) whose plan (S, rows) satisfies pred(K, S, rows)"""
    for K in range(start + 4, start + (1 << 16), 4):
        el, S, rows, _ = plan(Mo, No, K)
        if el and pred(K, S, rows):
            return K
    raise AssertionError("no such K near the threshold")


def k_cases(Mo, No):
    kmin = smallest_eligible_k(Mo, No)
    return {
        "kmin": kmin,
        "below": kmin - 4,                                                                   # not eligible: the tile kernel
        "last4": first_k(Mo, No, kmin, lambda K, S, rows: K - (S - 1) * rows == 4),          # last range: 4 rows, one partial slab
        "full": first_k(Mo, No, kmin, lambda K, S, rows: K == S * rows),                     # last range exactly full
        "ragged": kmin + 37,                                                                 # not a multiple of 32 (nor of 4)
    }


def run(dev, Mo, No, K, regime, c_forms, acc=False, twice=False):
    from dp_gsat_amd._lib import call, stream
    el, S, rows, wsf = plan(Mo, No, K)
    if el:
        assert wsf == S * Mo * No and rows % 32 == 0 and (S - 1) * rows < K <= S * rows, (el, S, rows, wsf, K)
    g = torch.Generator(device=dev).manual_seed(Mo * 7 + No * 3 + K + (1 << 20) * (regime == "exact"))
    A, B, _, C0 = _inputs(regime, Mo, No, K, g, dev)              # logical A [Mo, K], B [K, No]
    rA = Region(dev, K + EXTRA_ROWS, Mo, "pad", "nan")
    rB = Region(dev, K + EXTRA_ROWS, No, "pad", "nan")
    rA.view[:K].copy_(A.t())
    rB.view[:K].copy_(B)
    A64, B64 = A.double(), B.double()
    ref = A64 @ B64 + (C0.double() if acc else 0.0)               # once per (shape, K, regime), shared by the output layouts
    absab = A64.abs() @ B64.abs()
    for c_form in c_forms:
        rC = Region(dev, Mo, No, c_form, "pattern")
        if acc:
            rC.view.copy_(C0)
        ws = torch.empty(2 * GUARD + wsf, device=dev, dtype=torch.float32)
        ws.view(torch.int32).fill_(PATTERN)
        c_before = rC.snapshot()
        images = []
        for _ in range(2 if twice else 1):
            if acc:
                rC.view.copy_(C0)
            call("gsat_gemm_wgrad_x3", Mo, No, K, rA.ptr, rA.ld, rB.ptr, rB.ld, rC.ptr, rC.ld, int(acc), ws.data_ptr() + 4 * GUARD, wsf, stream())
            torch.cuda.synchronize()
            images.append(rC.buf.view(torch.int32).clone())
        what = (f"Mo={Mo} No={No} K={K}", regime, c_form, f"acc={acc}", f"plan={(el, S, rows, wsf)}")
        if twice:
            assert torch.equal(images[0], images[1]), ("two calls on the same inputs differ",) + what
        assert torch.equal(rC.snapshot(), c_before), ("C guard / padding / other half changed",) + what
        wsi = ws.view(torch.int32)
        assert bool((wsi[:GUARD] == PATTERN).all()) and bool((wsi[GUARD + wsf:] == PATTERN).all()), ("workspace guard changed",) + what
        got = rC.view.double()
        assert not bool(torch.isnan(got).any()), ("NaN in the output: padding was read, or an element was not written",) + what
        if regime == "exact":
            assert torch.equal(got, ref), ("exact sums differ", f"{int((got != ref).sum())} elements") + what
            continue
        err = (got - ref).abs()
        bound = (2.0 ** -16 + 2.0 * K * U) * absab + (U * (absab + C0.double().abs()) if acc else 0.0)
        ratio = (err / absab).max().item()
        print(f"\nWGRAD-RATIO Mo={Mo} No={No} K={K} eligible={el} S={S} rows={rows}: worst err/(|A||B|) {ratio:.3e} against {2.0 ** -16 + 2.0 * K * U:.3e}")
        assert not bool((err > bound).any()), ("componentwise bound exceeded", f"worst err / (|A||B|) {ratio:.3e}") + what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("which", ["kmin", "below", "last4", "full", "ragged"])
def test_wgrad_against_fp64(dev, shape, which):
    """every K case of every tile count, both regimes; ldc = No + 8 and C as the right half of [Mo, 2 No] at the threshold"""
    Mo, No = shape
    K = k_cases(Mo, No)[which]
    assert plan(Mo, No, K)[0] == (0 if which == "below" else 1)
    forms = ["pad", "half"] if which in ("kmin", "below") else (["half"] if which == "last4" else ["pad"])
    for regime in ("exact", "scaled"):
        run(dev, Mo, No, K, regime, forms)


def test_wgrad_is_bitwise_reproducible_and_accumulates(dev):
    Mo, No = 128, 256
    K = k_cases(Mo, No)["ragged"]
    run(dev, Mo, No, K, "scaled", ["half"], twice=True)
    run(dev, Mo, No, K, "exact", ["pad"], acc=True, twice=True)
    run(dev, Mo, No, K, "scaled", ["pad"], acc=True)


def test_attn_bwd_weight_gradients_take_the_streaming_kernel(dev, monkeypatch):
    """gsat_attn_bwd in node mode at H = 128, C1 = 256, C2 = 128 with as many rows as the smallest eligible K of its two weight gradients,
    in graphs of 20-40 rows: dW1 and dW2 against the same call on the exact-fp32 products (GSAT_ATTN_BWD_SPLIT=0), within 1e-4 of each
    gradient's largest magnitude."""
    from tests.test_gpu_attn_fused import _fwd_bwd, _params
    H, C1, C2 = 128, 256, 128
    N = max(smallest_eligible_k(C2, C1), smallest_eligible_k(C1, H))
    assert plan(C2, C1, N)[0] == 1 and plan(C1, H, N)[0] == 1
    g = torch.Generator().manual_seed(3)
    sizes = []
    while sum(sizes) < N:
        sizes.append(min(int(torch.randint(20, 41, (1,), generator=g)), N - sum(sizes)))
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    v = torch.arange(1, N)
    v = v[batch[v] == batch[v - 1]]                    # a path through every graph
    ei = torch.stack([torch.cat([v - 1, v]), torch.cat([v, v - 1])])
    emb = torch.randn(N, H, generator=g).to(dev)
    params = _params(H, False, dev, 11, C1, C2)
    dl, da = torch.randn(N, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
    monkeypatch.delenv("GSAT_ATTN_BWD_SPLIT", raising=False)
    new = _fwd_bwd(dev, emb, params, ei, batch, len(sizes), False, None, None, dl, da, False, monkeypatch, training=False)
    monkeypatch.setenv("GSAT_ATTN_BWD_SPLIT", "0")
    ref = _fwd_bwd(dev, emb, params, ei, batch, len(sizes), False, None, None, dl, da, False, monkeypatch, training=False)
    for k in ("dW1", "dW2"):
        assert not torch.isnan(new[k]).any(), f"{k}: unwritten entries"
        err, scale = (new[k] - ref[k]).abs().max().item(), ref[k].abs().max().item()
        print(f"\nWGRAD-ATTN {k}: max err {err:.3e}, largest magnitude {scale:.3e}")
        assert err <= 1e-4 * scale, (k, err, scale)
