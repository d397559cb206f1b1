"""-m gpu: the paired backward products (csrc/gemm.hip: k_pair_x3, entry gsat_gemm_pair_x3): OUT[R, Co] = G W and DW[Cg, Cy] (+)= G^T Y in one
launch, against the two separate calls it replaces -- gsat_gemm_bf16x3(a_t = 0, b_t = 0) on k_gemm_ws_x3 and gsat_gemm_wgrad_x3 on k_wgrad_x3 -- on
the SAME input buffers, in the buffer style of tests/test_gpu_gemm_paths.py: G [R, Cg] and Y [R, Cy] sit inside larger flat buffers whose column
padding, guards and 32 further rows beyond R are NaN; padding and guards of OUT, DW and the workspace hold a fixed bit pattern.

  bits    both regimes of that file: the int32 images of the whole OUT and DW buffers (payload, padding, guards) are torch.equal to those the two
          separate calls leave -- the pair runs both kernel bodies unchanged, so there is no tolerance.
  exact   integers in [-8, 8]: every partial sum is an integer below 2^24 and exact in bf16 -> torch.equal to an fp64 product.

The row counts come from the plans: the smallest R at which gsat_gemm_pair_plan pairs, R + 37 (ragged last 32-row tile and last range), an R whose
last weight-gradient range holds 4 rows, and the last R below the threshold, which must take the separate kernels.
"""
import ctypes

import pytest
import torch

from tests.test_gpu_gemm_paths import GUARD, PATTERN, Region, _inputs

pytestmark = pytest.mark.gpu

SHAPES = [(128, 256, 256), (256, 128, 128)]            # (Cg, Co, Cy): the extractor's dh2 -> (da1, dW2) and dh1 -> (demb, dW1)
# the remaining instantiations of k_pair_x3, <4,2>, <4,4> and <2,4>: narrower OUT, hence two, four and eight k-splits in the backward-data body
MORE_SHAPES = [(128, 128, 128), (256, 64, 128), (256, 32, 128)]
EXTRA_ROWS = 32                                        # NaN rows of G and Y beyond R
WS_X3 = 3                                              # gsat_gemm_plan family of k_gemm_ws_x3


def _call_plan(name, n, *args):
    from dp_gsat_amd._lib import call
    out = (ctypes.c_int32 * n)()
    call(name, *args, out)
    return tuple(out)


def pair_plan(R, Cg, Co, Cy):
    return _call_plan("gsat_gemm_pair_plan", 4, R, Cg, Co, Cy)         # (paired, wgrad workgroups, dgrad workgroups, LDS bytes)


def wgrad_plan(R, Cg, Cy):
    return _call_plan("gsat_gemm_wgrad_plan", 4, Cg, Cy, R)            # (eligible, S, rows per range, workspace floats)


def dgrad_plan(R, Cg, Co):
    return _call_plan("gsat_gemm_plan", 8, 1, 0, 0, R, Co, Cg, 0, 0, Co + 8)


def smallest_paired_r(Cg, Co, Cy):
    lo, hi = 4, 1 << 24                                # pairing is monotone in R: bisect over multiples of 4
    assert pair_plan(hi, Cg, Co, Cy)[0] == 1 and pair_plan(lo, Cg, Co, Cy)[0] == 0
    while hi - lo > 4:
        mid = (lo + hi) // 8 * 4
        if pair_plan(mid, Cg, Co, Cy)[0]:
            hi = mid
        else:
            lo = mid
    return hi


def r_cases(Cg, Co, Cy):
    rmin = smallest_paired_r(Cg, Co, Cy)
    last4 = None
    for R in range(rmin + 4, rmin + (1 << 16), 4):     # last range of the weight gradient: 4 rows, one partial slab
        el, S, rows, _ = wgrad_plan(R, Cg, Cy)
        if el and R - (S - 1) * rows == 4 and pair_plan(R, Cg, Co, Cy)[0]:
            last4 = R
            break
    assert last4 is not None, "no R near the threshold whose last range holds 4 rows"
    return {"rmin": rmin, "ragged": rmin + 37, "last4": last4, "below": rmin - 4}


def _images(dev, Cg, Co, Cy, R, G, W, Y, DW0, entry, acc, dw_form, twice):
    """run `entry` ("pair" | "separate") on fresh output regions; the int32 images of the whole OUT and DW buffers and the two payload views"""
    from dp_gsat_amd._lib import call, stream
    wsf = wgrad_plan(R, Cg, Cy)[3]
    rOUT = Region(dev, R, Co, "pad", "pattern")
    rDW = Region(dev, Cg, Cy, dw_form, "pattern")
    ws = torch.empty(2 * GUARD + wsf, device=dev, dtype=torch.float32)
    ws.view(torch.int32).fill_(PATTERN)
    out_before, dw_before = rOUT.snapshot(), rDW.snapshot()
    images = []
    for _ in range(2 if twice else 1):
        if acc:
            rDW.view.copy_(DW0)
        wsp = ws.data_ptr() + 4 * GUARD
        if entry == "pair":
            call("gsat_gemm_pair_x3", R, Cg, Co, Cy, G.ptr, G.ld, W.ptr, W.ld, rOUT.ptr, rOUT.ld, Y.ptr, Y.ld, rDW.ptr, rDW.ld, int(acc), wsp, wsf, stream())
        else:
            call("gsat_gemm_wgrad_x3", Cg, Cy, R, G.ptr, G.ld, Y.ptr, Y.ld, rDW.ptr, rDW.ld, int(acc), wsp, wsf, stream())
            call("gsat_gemm_bf16x3", 0, 0, R, Co, Cg, G.ptr, G.ld, W.ptr, W.ld, rOUT.ptr, rOUT.ld, None, 0, None, 0, stream())
        torch.cuda.synchronize()
        images.append((rOUT.buf.view(torch.int32).clone(), rDW.buf.view(torch.int32).clone()))
    if twice:
        assert torch.equal(images[0][0], images[1][0]) and torch.equal(images[0][1], images[1][1]), ("two calls on the same inputs differ", entry)
    assert torch.equal(rOUT.snapshot(), out_before), ("OUT guard / padding changed", entry)
    assert torch.equal(rDW.snapshot(), dw_before), ("DW guard / padding / other half changed", entry)
    wsi = ws.view(torch.int32)
    assert bool((wsi[:GUARD] == PATTERN).all()) and bool((wsi[GUARD + wsf:] == PATTERN).all()), ("workspace guard changed", entry)
    return images[-1], rOUT.view, rDW.view


def run(dev, Cg, Co, Cy, R, regime, paired, acc=False, dw_form="pad", twice=False):
    pp = pair_plan(R, Cg, Co, Cy)
    what = (f"Cg={Cg} Co={Co} Cy={Cy} R={R}", regime, f"acc={acc}", f"plan={pp}")
    assert pp[0] == int(paired), what
    if paired:                                         # the two kernels being paired are the ones the separate calls run
        assert dgrad_plan(R, Cg, Co)[0] == WS_X3 and wgrad_plan(R, Cg, Cy)[0] == 1, what
    g = torch.Generator(device=dev).manual_seed(Cg * 7 + Co * 3 + R + (1 << 20) * (regime == "exact"))
    Gm, Wm, _, _ = _inputs(regime, R, Co, Cg, g, dev)                  # G [R, Cg], W [Cg, Co]
    _, Ym, _, DW0 = _inputs(regime, Cg, Cy, R, g, dev)                 # Y [R, Cy], DW0 [Cg, Cy]
    rG = Region(dev, R + EXTRA_ROWS, Cg, "pad", "nan")
    rY = Region(dev, R + EXTRA_ROWS, Cy, "pad", "nan")
    rW = Region(dev, Cg, Co, "pad", "nan")
    rG.view[:R].copy_(Gm)
    rY.view[:R].copy_(Ym)
    rW.view.copy_(Wm)
    (out_p, dw_p), OUT, DW = _images(dev, Cg, Co, Cy, R, rG, rW, rY, DW0, "pair", acc, dw_form, twice)
    assert not bool(torch.isnan(OUT).any()) and not bool(torch.isnan(DW).any()), ("NaN in an output: padding was read, or an element was not written",) + what
    if regime == "exact":
        G64 = Gm.double()
        ref_out, ref_dw = G64 @ Wm.double(), G64.t() @ Ym.double() + (DW0.double() if acc else 0.0)
        assert torch.equal(OUT.double(), ref_out), ("exact OUT differs", f"{int((OUT.double() != ref_out).sum())} elements") + what
        assert torch.equal(DW.double(), ref_dw), ("exact DW differs", f"{int((DW.double() != ref_dw).sum())} elements") + what
    (out_s, dw_s), _, _ = _images(dev, Cg, Co, Cy, R, rG, rW, rY, DW0, "separate", acc, dw_form, False)
    assert torch.equal(out_p, out_s), ("OUT differs from gsat_gemm_bf16x3", f"{int((out_p != out_s).sum())} words") + what
    assert torch.equal(dw_p, dw_s), ("DW differs from gsat_gemm_wgrad_x3", f"{int((dw_p != dw_s).sum())} words") + what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("which", ["rmin", "ragged", "last4", "below"])
def test_pair_has_the_bits_of_the_two_calls(dev, shape, which):
    """every row count of both shapes, both regimes, without and with accumulation into DW; two calls give the same bits"""
    Cg, Co, Cy = shape
    R = r_cases(Cg, Co, Cy)[which]
    paired = which != "below"
    run(dev, Cg, Co, Cy, R, "exact", paired, acc=False, dw_form="half" if which == "rmin" else "pad", twice=True)
    run(dev, Cg, Co, Cy, R, "scaled", paired, acc=False)
    run(dev, Cg, Co, Cy, R, "exact", paired, acc=True)
    run(dev, Cg, Co, Cy, R, "scaled", paired, acc=True, dw_form="half", twice=True)


@pytest.mark.parametrize("shape", MORE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_other_instantiations(dev, shape):
    """the kernels no workload of the benchmark reaches, at a ragged row count just above their threshold"""
    Cg, Co, Cy = shape
    R = smallest_paired_r(Cg, Co, Cy) + 37
    assert dgrad_plan(R, Cg, Co)[5:8] == {(128, 128): (4, 4, 2), (256, 64): (2, 4, 4), (256, 32): (1, 2, 4)}[(Cg, Co)]       # NB, KSTEPS, NQ
    run(dev, Cg, Co, Cy, R, "exact", True, acc=False, twice=True)
    run(dev, Cg, Co, Cy, R, "scaled", True, acc=True, dw_form="half")
