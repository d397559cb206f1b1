"""not gpu: gsat_gemm_pair_plan (host arithmetic) against the plans of the two calls it pairs: one launch exactly when gsat_gemm_bf16x3(a_t = 0,
b_t = 0) would take its weight-stationary split-bf16 kernel (gsat_gemm_plan family 3) AND gsat_gemm_wgrad_x3 its streaming kernel (AND two
workgroups of the pair fit the LDS of a CU, which excludes Cg = 512)."""
import ctypes

import pytest

WS_X3 = 3


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def pair_plan(R, Cg, Co, Cy):
    from dp_gsat_amd._lib import call
    out = (ctypes.c_int32 * 4)()
    call("gsat_gemm_pair_plan", R, Cg, Co, Cy, out)
    return tuple(out)                                  # (paired, weight-gradient workgroups, backward-data workgroups, LDS bytes)


def gemm_plan(M, N, K):
    from dp_gsat_amd._lib import call
    out = (ctypes.c_int32 * 8)()
    call("gsat_gemm_plan", 1, 0, 0, M, N, K, 0, 0, N, out)
    return tuple(out)


def wgrad_plan(Mo, No, K):
    from dp_gsat_amd._lib import call
    out = (ctypes.c_int32 * 4)()
    call("gsat_gemm_wgrad_plan", Mo, No, K, out)
    return tuple(out)


ROWS = [4, 1000, 8192, 30000, 32764, 32768, 32805, 51639, 65536, 111310, 500000]
CHANNELS = [64, 128, 192, 256, 512]


def test_pair_plan_is_the_conjunction_of_the_two_plans(monkeypatch):
    monkeypatch.delenv("GSAT_GEMM_PRECISION", raising=False)
    paired = 0
    for Cg in CHANNELS:
        for Co in CHANNELS:
            for Cy in (Co, 128):
                for R in ROWS:
                    g, w, p = gemm_plan(R, Co, Cg), wgrad_plan(Cg, Cy, R), pair_plan(R, Cg, Co, Cy)
                    lds = max(65536, 4 * 32 * (2 * Cg + 16))                              # the larger of the two bodies' LDS
                    fits = 2 * lds <= 160 * 1024                                          # a workgroup of each kind on one CU
                    assert p[0] == int(g[0] == WS_X3 and w[0] == 1 and fits), (R, Cg, Co, Cy, g, w, p)
                    if not p[0]:
                        assert p == (0, 0, 0, 0)
                        continue
                    paired += 1
                    assert p[1] == (Cg // 128) * (Cy // 128) * w[1]                       # the weight gradient's grid, unchanged
                    chunks = (Co + 255) // 256
                    assert p[2] % chunks == 0 and 0 < p[2] // chunks <= (R + 31) // 32      # at most one workgroup per row tile
                    # two 32 KB operand images (weight gradient), or two buffers of two bf16 planes of 32 rows x (2 Cg + 16) bytes
                    assert p[3] == lds
    assert paired >= 20
    # the extractor's two pairs at the benchmark size: dh2 -> (da1, dW2) and dh1 -> (demb, dW1)
    assert pair_plan(51639, 128, 256, 256)[0] == 1 and pair_plan(51639, 256, 128, 128)[0] == 1
    # below either threshold the two calls stay separate
    assert pair_plan(4096, 128, 256, 256)[0] == 0 and pair_plan(400, 256, 128, 128)[0] == 0


def test_pair_plan_follows_the_split_setting(monkeypatch):
    monkeypatch.setenv("GSAT_GEMM_PRECISION", "fp32")                               # split-bf16 not wanted: neither kernel runs
    assert pair_plan(51639, 128, 256, 256)[0] == 0 and pair_plan(51639, 256, 128, 128)[0] == 0
    monkeypatch.delenv("GSAT_GEMM_PRECISION", raising=False)
    assert pair_plan(51639, 128, 256, 256)[0] == 1


def test_pair_plan_rejects_bad_extents():
    from dp_gsat_amd._lib import GsatHipError
    with pytest.raises(GsatHipError):
        pair_plan(0, 128, 256, 256)
