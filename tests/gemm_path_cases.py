"""The GEMM dispatch cases shared by tests/test_gpu_gemm_paths.py (runs them) and tests/test_gemm_plan_host.py (checks that they name
every plan the dispatcher can reach).  Plain data, no torch, no GPU.

Every case carries the plan `gsat_gemm_plan` must report for it, written out by hand from ws_geometry / wsx3_geometry / gemm_tile /
gemm_splits in csrc/gemm.hip: (family, TM, TN, splits, reduce, NB, KR | KSTEPS, NQ).  A dispatch change then fails the plan assertion
instead of quietly moving a case onto another kernel.
"""
from collections import namedtuple

TILE_F32, TILE_X3, WS_F32, WS_X3 = 0, 1, 2, 3
FAMILY_NAMES = {TILE_F32: "k_gemm_f32", TILE_X3: "k_gemm_bf16x3", WS_F32: "k_gemm_ws", WS_X3: "k_gemm_ws_x3"}

# precision: value of GSAT_GEMM_PRECISION ("fp32" | "bf16x3"); the split cases go through gsat_gemm_bf16x3, the others through gsat_gemm_f32
# tile: value of GSAT_GEMM_TILE or None;  runs: (M, bias, accumulate) per call -- all calls of a case share N, K, layout and plan
# b_form / c_form: how the operand sits in its buffer: "pad" = leading dimension extent + 8; "half" = the right half of a matrix twice
# as wide (B = W + K with ldb = 2K, the extractor's `W1 + H`; C = base + N' with ldc = 2N', the dW1 pair's form)
Case = namedtuple("Case", "name precision tile a_t b_t N K runs b_form c_form plan")


def _id(*parts):
    return "-".join(str(p) for p in parts)


# ---- 1. tile kernels: every layout x (TM, TN) x precision at one ragged shape, and K = 4 under the default tile choice ----------------
LAYOUTS = [(0, 1), (0, 0), (1, 0), (1, 1)]            # (a_t, b_t)
RAGGED = (132, 68, 36)                                # two 64- or 128-row blocks, N just past 64, K just past one 32-deep slab


def _tile_runs(M, a_t):
    # bias only where the header allows it (a_t == 0); accumulate everywhere
    return [(M, False, False), (M, False, True)] + ([(M, True, False)] if not a_t else [])


TILE_CASES = []
for _prec, _fam in (("fp32", TILE_F32), ("bf16x3", TILE_X3)):
    for _a_t, _b_t in LAYOUTS:
        for _tm in (1, 2):
            for _tn in (1, 2):
                M, N, K = RAGGED
                TILE_CASES.append(Case(_id("tile", _prec, f"at{_a_t}bt{_b_t}", f"{_tm}{_tn}"), _prec, f"{_tm}{_tn}", _a_t, _b_t, N, K,
                                       _tile_runs(M, _a_t), "pad", "pad", (_fam, _tm, _tn, 1, 0, 0, 0, 0)))
        # K = 4: one slab of 4 live k.  No override: fp32 takes 128 x 64 (gemm_tile: 4 blocks cost 1 round, 2 blocks of 128 x 128 cost 2),
        # split-bf16 always the largest tile
        M, N, K = RAGGED[0], RAGGED[1], 4
        TILE_CASES.append(Case(_id("tile", _prec, f"at{_a_t}bt{_b_t}", "k4"), _prec, None, _a_t, _b_t, N, K, _tile_runs(M, _a_t), "pad", "pad",
                               (_fam, 2, 1, 1, 0, 0, 0, 0) if _fam == TILE_F32 else (_fam, 2, 2, 1, 0, 0, 0, 0)))

# ---- 2. split-K (a_t = 1) and the four slab sums ---------------------------------------------------------------------------------------
# gemm_splits: one 128 x 128 tile -> min(768, ceil(K / 256)) splits (ceil(K / 128) when M, N <= 64).  The fp32 family drops to 64 x 64
# tiles while blocks x splits < 384; split-bf16 keeps tm = (M > 64) + 1, tn = (N > 64) + 1.
#            M    N    K   splits reduce  fp32 (tm, tn)  bf16x3 (tm, tn)
_SPLITK = [(68, 72, 2052, 9, 4, (1, 1), (2, 2)),             # 2..63 splits: 4 lanes per quad
           (60, 64, 1028, 9, 4, (1, 1), (1, 1)),             # M, N <= 64: 4 slabs per split, 64 x 64 tiles in both families
           (68, 64, 2052, 9, 4, (1, 1), (2, 1)),             # split-K on a non-square split-bf16 tile: 128 x 64 ...
           (64, 72, 2052, 9, 4, (1, 1), (1, 2)),             # ... and 64 x 128
           (68, 72, 17924, 71, 8, (1, 1), (2, 2)),           # 64..127 splits: 8 lanes
           (260, 132, 17924, 71, 8, (2, 2), (2, 2)),         # 6 tiles x 71 splits >= 384 blocks: fp32 keeps 128 x 128
           (68, 72, 33284, 131, 16, (1, 1), (2, 2)),         # >= 128 splits: 16 lanes
           (68, 66, 2052, 9, 1, (1, 1), (2, 2))]             # N % 4 != 0 (b_t = 1 only): scalar sum
SPLITK_CASES = []
for _prec, _fam in (("fp32", TILE_F32), ("bf16x3", TILE_X3)):
    for (_M, _N, _K, _s, _red, _t32, _tx3), _b_t, _c_form in ((r, b, c) for r in _SPLITK for b in (0, 1) for c in ("pad", "half")):
        _tm, _tn = _t32 if _fam == TILE_F32 else _tx3
        if _N % 4 == 0 or _b_t:
            SPLITK_CASES.append(Case(_id("splitk", _prec, f"{_M}x{_N}x{_K}", f"bt{_b_t}", _c_form), _prec, None, 1, _b_t, _N, _K,
                                     [(_M, False, False), (_M, False, True)], "pad", _c_form, (_fam, _tm, _tn, _s, _red, 0, 0, 0)))

# ---- 3. weight-stationary kernels --------------------------------------------------------------------------------------------------------
WS_GRID_N = (32, 64, 128, 256, 512, 1024)
WS_GRID_K = (64, 128, 256, 512)
WS_ROWS = (8192, 8193, 8192 + 31)                     # the threshold, one row into a new 32-row tile, one row short of a full tile
WS_UNEVEN_ROWS = 32 * 1027 + 5                        # 1028 tiles on a 256- or 512-workgroup grid: 4 workgroups get one tile more
# (N, K) -> (NB, KR) of k_gemm_ws: NB = min(N, 256) / 32 column blocks, KS = 8 / NB k-splits, KR = K / KS / 2 in {16, 32, 64, 128}, and
# the k-split exchange (KS - 1) NB 1024 floats must fit one A buffer of 32 (K + 4)
WS_F32_GEOMETRY = {(32, 256): (1, 16), (32, 512): (1, 32), (64, 256): (2, 32), (64, 512): (2, 64),
                   (128, 128): (4, 32), (128, 256): (4, 64), (128, 512): (4, 128)}
# (N, K) -> (NB, KSTEPS) of k_gemm_ws_x3: KSTEPS = K / KS / 16 in {2, 4, 8}, exchange (KS - 1) NB 4096 bytes <= 64 (2 K + 16)
WS_X3_GEOMETRY = {(32, 256): (1, 2), (32, 512): (1, 4), (64, 256): (2, 4), (64, 512): (2, 8), (128, 128): (4, 4), (128, 256): (4, 8)}
for _N in (256, 512, 1024):                           # N >= 256: 8 column blocks, no k-split, wider outputs as 256-column chunks
    for _K, _kr, _st in ((64, 32, 4), (128, 64, 8), (256, 128, None)):
        WS_F32_GEOMETRY[(_N, _K)] = (8, _kr)
        if _st:
            WS_X3_GEOMETRY[(_N, _K)] = (8, _st)
WS_UNEVEN = (128, 128)                                # the geometry that also runs WS_UNEVEN_ROWS (4 column blocks x 2 k-splits), b_t = 1

WS_CASES = []
for _prec, _fam, _geo in (("fp32", WS_F32, WS_F32_GEOMETRY), ("bf16x3", WS_X3, WS_X3_GEOMETRY)):
    for (_N, _K), (_nb, _kr) in sorted(_geo.items()):
        for _b_t in (1, 0):
            rows = list(WS_ROWS) + ([WS_UNEVEN_ROWS] if (_N, _K) == WS_UNEVEN and _b_t == 1 else [])
            # the flag alternates over the row counts: bias on the fp32 family, accumulate on the split family
            runs = [(m, _fam == WS_F32 and i % 2 == 1, _fam == WS_X3 and i % 2 == 1) for i, m in enumerate(rows)]
            WS_CASES.append(Case(_id("ws", _prec, f"{_N}x{_K}", f"bt{_b_t}"), _prec, None, 0, _b_t, _N, _K, runs,
                                 "half" if _b_t else "pad", "pad", (_fam, 0, 0, 1, 0, _nb, _kr, _K // 64)))

ALL_CASES = TILE_CASES + SPLITK_CASES + WS_CASES
