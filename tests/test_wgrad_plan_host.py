"""not gpu: gsat_gemm_wgrad_plan (host arithmetic) and the workspace of gsat_attn_bwd that is sized by it."""
import ctypes

import pytest


def plan(Mo, No, K):
    from dp_gsat_amd._lib import call
    out = (ctypes.c_int32 * 4)()
    call("gsat_gemm_wgrad_plan", Mo, No, K, out)
    return tuple(out)                                  # (eligible, S, rows per range, workspace floats)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def test_plan_workspace_is_s_tiles_and_ranges_cover_k(monkeypatch):
    from dp_gsat_amd._lib import load
    monkeypatch.delenv("GSAT_GEMM_PRECISION", raising=False)
    seen = 0
    for Mo, No in [(128, 128), (128, 256), (256, 128), (256, 256), (384, 128)]:
        for K in [4, 1000, 30000, 32764, 32768, 51639, 65532, 65536, 65573, 111310, 500000, 4000000]:
            el, S, rows, wsf = plan(Mo, No, K)
            if el:
                seen += 1
                assert wsf == S * Mo * No
                assert rows % 32 == 0 and rows >= 8 * 32 and S >= 2
                assert (S - 1) * rows < K <= S * rows              # every range holds rows, the last one at least one
            else:                                                  # the tile kernel's split, as gsat_gemm_bf16x3(a_t = 1) sizes it
                assert wsf == load().gsat_gemm_workspace_floats(1, Mo, No, K)
    assert seen >= 20
    assert plan(128, 256, 51639)[0] == 1 and plan(256, 128, 51639)[0] == 1          # the extractor's weight gradients at the benchmark size
    for Mo, No, K in [(64, 128, 100000), (128, 192, 100000), (100, 128, 100000)]:   # no whole 128 x 128 tiles
        assert plan(Mo, No, K)[0] == 0
    monkeypatch.setenv("GSAT_GEMM_PRECISION", "fp32")                               # split-bf16 not wanted
    assert plan(128, 256, 51639)[0] == 0


@pytest.mark.parametrize("edge_mode", [0, 1])
def test_attn_bwd_workspace_grows_by_at_most_the_plan(monkeypatch, edge_mode):
    """With GSAT_GEMM_PRECISION=fp32 no product is eligible and the workspace is the tile kernel's alone."""
    from dp_gsat_amd._lib import AttnArgs, load
    lib = load()
    H = 128
    for rows in [1000, 40000, 51639, 111310, 700000]:
        a = AttnArgs()
        a.M, a.N, a.G, a.H, a.edge_mode = rows, rows // 2 if edge_mode else rows, 64, H, edge_mode
        a.C1, a.C2 = (4 * H, H) if edge_mode else (2 * H, H)
        monkeypatch.delenv("GSAT_GEMM_PRECISION", raising=False)
        new = lib.gsat_attn_bwd_workspace_bytes(ctypes.byref(a))
        plans = [plan(a.C2, a.C1, a.M)] + [plan(a.C1, H, a.N)] * (2 if edge_mode else 1)
        monkeypatch.setenv("GSAT_GEMM_PRECISION", "fp32")
        old = lib.gsat_attn_bwd_workspace_bytes(ctypes.byref(a))
        assert old <= new <= old + 4 * sum(p[3] for p in plans if p[0])
