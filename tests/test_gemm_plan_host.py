"""not gpu: gsat_gemm_plan (the dispatcher's own decision function, host arithmetic only) against the case list of the GPU test.

The GPU test can only cover what its cases name.  Here the query is enumerated over the whole grid the cases were drawn from, and the set of
distinct plans it reaches must EQUAL the set the cases name: a new reachable instantiation without a case, or a case whose plan is no
longer reached, fails on a machine without a GPU."""
import ctypes

import pytest

from tests import gemm_path_cases as gc


def query(precision, a_t, b_t, M, N, K, bias=False, accumulate=False, ldb=None):
    from dp_gsat_amd._lib import call
    plan = (ctypes.c_int32 * 8)()
    call("gsat_gemm_plan", int(precision == "bf16x3"), int(a_t), int(b_t), M, N, K, int(bias), int(accumulate),
         (K if b_t else N) if ldb is None else ldb, plan)
    return tuple(plan)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture
def env(monkeypatch):
    def set_(precision, tile):
        monkeypatch.setenv("GSAT_GEMM_PRECISION", precision)
        if tile is None:
            monkeypatch.delenv("GSAT_GEMM_TILE", raising=False)
        else:
            monkeypatch.setenv("GSAT_GEMM_TILE", tile)
    return set_


def test_every_case_reports_its_plan(env):
    assert len({c.name for c in gc.ALL_CASES}) == len(gc.ALL_CASES)
    for c in gc.ALL_CASES:
        env(c.precision, c.tile)
        for M, bias, acc in c.runs:
            assert query(c.precision, c.a_t, c.b_t, M, c.N, c.K, bias, acc) == c.plan, (c.name, M, bias, acc)


def test_weight_stationary_grid_is_covered(env):
    """Every weight-stationary plan reachable for N in {32..1024}, K in {64..512}, either B layout, has a GPU case, and no case names
    an unreachable one."""
    for precision, fams in (("fp32", (gc.WS_F32,)), ("bf16x3", (gc.WS_X3,))):
        env(precision, None)
        reached = set()
        for N in gc.WS_GRID_N:
            for K in gc.WS_GRID_K:
                for b_t in (0, 1):
                    for M in gc.WS_ROWS + (gc.WS_UNEVEN_ROWS,):
                        p = query(precision, 0, b_t, M, N, K)
                        if p[0] in (gc.WS_F32, gc.WS_X3):
                            reached.add((b_t, N, K) + p)
        named = {(c.b_t, c.N, c.K) + c.plan for c in gc.WS_CASES if c.precision == precision}
        assert reached == named, sorted(reached ^ named)
        # entries are (b_t, N, K, family, TM, TN, splits, reduce, NB, KR | KSTEPS, NQ)
        assert {e[3] for e in reached} == set(fams)


def test_weight_stationary_threshold_and_exclusions(env):
    for precision, tile_family in (("fp32", gc.TILE_F32), ("bf16x3", gc.TILE_X3)):
        env(precision, None)
        for c in gc.WS_CASES:
            if c.precision == precision:
                assert query(precision, 0, c.b_t, 8191, c.N, c.K)[0] == tile_family, c.name          # one row below the threshold
        # the shapes the geometry functions reject stay on the tile kernel at any row count
        for N, K in ((32, 64), (32, 128), (64, 64), (64, 128), (128, 64), (256, 512), (96, 128)):
            assert query(precision, 0, 1, 20000, N, K)[0] == tile_family, (N, K)
    env("bf16x3", None)
    assert query("bf16x3", 0, 1, 20000, 256, 512) == (gc.TILE_X3, 2, 2, 1, 0, 0, 0, 0)            # 32 fragment steps: not weight-stationary
    assert query("bf16x3", 0, 1, 20000, 128, 512)[0] == gc.TILE_X3
    # what moves a weight-stationary shape onto the tile kernel: accumulate (fp32), a bias (split-bf16), a transposed A
    env("fp32", None)
    assert query("fp32", 0, 1, 8192, 128, 128, accumulate=True)[0] == gc.TILE_F32
    assert query("fp32", 1, 0, 8192, 128, 128)[0] == gc.TILE_F32
    env("bf16x3", None)
    assert query("bf16x3", 0, 1, 8192, 128, 128, bias=True)[0] == gc.TILE_X3


def test_tile_and_splitk_plans_are_covered(env):
    """Over the tile and split-K shapes of the case list, in every layout, tile override and precision: the set of distinct
    (family, a_t, b_t, TM, TN, split?, reduce) the query reaches equals the set the cases name."""
    def key(a_t, b_t, p):
        return (p[0], a_t, b_t, p[1], p[2], p[3] > 1, p[4])
    reached, named = set(), set()
    for c in gc.TILE_CASES + gc.SPLITK_CASES:
        named.add(key(c.a_t, c.b_t, c.plan))
    shapes = {(c.runs[0][0], c.N, c.K) for c in gc.TILE_CASES + gc.SPLITK_CASES}
    for precision in ("fp32", "bf16x3"):
        for tile in (None, "11", "12", "21", "22"):
            env(precision, tile)
            for M, N, K in sorted(shapes):
                for a_t, b_t in gc.LAYOUTS:
                    if (a_t and M % 4) or (not b_t and N % 4):
                        continue
                    p = query(precision, a_t, b_t, M, N, K)
                    if tile is not None and p[3] > 1:
                        continue                          # split-K under a tile override: a tuning combination, not a dispatch path
                    reached.add(key(a_t, b_t, p))
    assert reached == named, sorted(reached ^ named)


def test_plan_splits_agree_with_the_workspace_query(env):
    from dp_gsat_amd._lib import load
    for c in gc.ALL_CASES:
        env(c.precision, c.tile)
        for M, bias, acc in c.runs:
            wsf = int(load().gsat_gemm_workspace_floats(c.a_t, M, c.N, c.K))
            assert wsf == (c.plan[3] * M * c.N if c.plan[3] > 1 else 0), c.name


def test_plan_rejects_what_the_dispatcher_rejects():
    from dp_gsat_amd._lib import GsatHipError
    with pytest.raises(GsatHipError):
        query("fp32", 0, 0, 128, 66, 36)                  # b_t = 0 needs N % 4 == 0
    with pytest.raises(GsatHipError):
        query("fp32", 1, 0, 130, 64, 36)                  # a_t = 1 needs M % 4 == 0
    with pytest.raises(GsatHipError):
        query("fp32", 1, 0, 68, 72, 2052, bias=True)      # bias with split-K
    with pytest.raises(GsatHipError):
        query("fp32", 0, 1, 0, 64, 36)
