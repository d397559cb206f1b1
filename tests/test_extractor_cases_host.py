"""not gpu: the inputs of the extractor path tests are what tests/test_gpu_extractor_paths.py takes them to be.  For every case of both
tables at every width and mode used there: the fp32 reference sits within the case's cap of the fp64 one (so no GPU comparison can pass on
the slack term), no pre-activation sits on the kink of ReLU, the regular table has no graph under 4 rows, every boundary size is present;
and the tables of expected kernel choices agree with what gsat_attn_paths reports (host arithmetic: no GPU needed)."""
import pytest
import torch

from tests import extractor_cases as ec
from tests import extractor_oracle as eo
from tests.extractor_driver import shape_args

SWITCHES = ("GSAT_ATTN_FUSED", "GSAT_ATTN_FUSED_X6", "GSAT_ATTN_FUSED_PQG", "GSAT_ATTN_BWD_FUSED", "GSAT_ATTN_BWD_SPLIT",
            "GSAT_ATTN_BWD_MERGED", "GSAT_DUAL_GEMM")


def _check_reference(case, refs, family, gradients, margin):
    r32, r64 = refs
    worst = {}
    for k in ec.FWD_TENSORS + (ec.GRAD_TENSORS if gradients else ()):
        if r64[k] is None:
            continue
        g, scale = eo.gap(r32[k], r64[k])
        cap = ec.cap_for(family, k)
        assert 4.0 * g <= cap * scale, f"{k}: 4 * |r32 - r64| = {4 * g:.3e} > cap {cap:.1e} * scale {scale:.3e}"
        worst[k] = g / scale
    if gradients:
        assert r64["relu_margin"] >= margin, f"a pre-activation lies {r64['relu_margin']:.2e} from the kink of ReLU (< {margin:.1e})"
        assert bool(((r32["a1"] > 0) == (r64["a1"] > 0)).all()), "the fp32 and fp64 references disagree on a ReLU sign"
    return worst


@pytest.mark.parametrize("family", list(ec.FAMILIES))
def test_oracle_alone_meets_the_caps(family):
    worst = {}
    n = 0
    for key in ec.all_cases():
        if key[0] != family:
            continue
        case = ec.make_case(*key)
        H = key[3]
        w = _check_reference(case, eo.references(case), family, H in ec.BWD_STAGED_WIDTHS or family == "tiny", ec.RELU_MARGIN)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        n += 1
    print(f"\n{family}: {n} cases, worst |r32 - r64|max / scale per tensor: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    if family == "tiny":        # the caps were taken from this measurement: 8 x the recorded value, so the value itself leaves a factor 2
        for k, v in ec.TINY_GAP_MEASURED.items():       # (where 8 x the value is under the regular cap, that cap holds instead)
            assert worst[k] <= max(2.0 * v, ec.CAP_REGULAR / 4.0), f"{k}: measured gap {worst[k]:.3e} is more than twice the recorded {v:.3e}"


@pytest.mark.parametrize("H", ec.LARGE_WIDTHS)
def test_oracle_alone_meets_the_caps_on_the_large_batch(H):
    case = ec.make_large_case(H)
    assert not case["edge_mode"] and case["M"] >= ec.LARGE_ROWS and case["training"]
    assert int(case["rows"].min()) >= 16 and int(case["rows"].max()) <= 40
    _check_reference(case, eo.references(case, key=("large", H)), "regular", True, ec.LARGE_RELU_MARGIN[H])


def test_regular_table_sits_on_the_boundaries_and_has_no_small_graph():
    for name, sizes in ec.REGULAR.items():
        assert set(ec.BOUNDARY_ROWS) <= set(sizes), set(ec.BOUNDARY_ROWS) - set(sizes)
        small = [s for s in sizes if 0 < s < 32]
        assert len(small) >= 3 and sum(small) <= 32, "several small graphs must fit one tile"
        for edge_mode in (False, True):
            for sorted_edges in ((False, True) if edge_mode else (False,)):
                case = ec.make_case("regular", name, edge_mode, 16, True, sorted_edges)
                rows = case["rows"].tolist()
                assert rows == list(sizes), "the rows per graph are the table's sizes in the mode under test"
                assert all(r == 0 or r >= ec.MIN_ROWS for r in rows)
                assert case["M"] == sum(sizes) < 2500 and case["ei"].shape[1] < 2500
                if edge_mode:
                    seg = case["batch"][case["ei"][0]]
                    assert bool((seg[1:] >= seg[:-1]).all()) == sorted_edges
                    assert bool((case["batch"][case["ei"][0]] == case["batch"][case["ei"][1]]).all())


def test_tiny_table_holds_graphs_of_zero_to_three_rows():
    seen = set()
    for name in ec.TINY:
        for edge_mode in (False, True):
            case = ec.make_case("tiny", name, edge_mode, 16, True)
            seen |= {(edge_mode, int(r)) for r in case["rows"].tolist() if r < 4}
            assert 0 < case["M"] < 2500
    assert {(False, r) for r in (0, 1, 2, 3)} <= seen and {(True, 0), (True, 2)} <= seen


def _paths(monkeypatch, case, fused, env, with_order=None):
    from dp_gsat_amd._lib import attn_paths
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return attn_paths(shape_args(case, fused, case["edge_mode"] if with_order is None else with_order))


def test_expected_forward_shapes_match_the_path_query(monkeypatch):
    import __graft_entry__ as ge
    ge.build()
    for (edge_mode, H), e in ec.FUSED_FWD_EXPECT.items():
        case = ec.make_case("regular", "boundaries", edge_mode, H, True)
        for x6 in ("1", "0"):
            for pqg in ("1", "0"):
                p = _paths(monkeypatch, case, 1, {"GSAT_ATTN_FUSED_X6": x6, "GSAT_ATTN_FUSED_PQG": pqg})
                want = dict(fwd_kind=2 if (x6 == "1" and e["x6"]) else 1, fwd_pqg=int(pqg == "1" and e["pqg"]), fwd_nrb=e["nrb"], fwd_ncbw=e["ncbw"])
                assert {k: p[k] for k in want} == want, (edge_mode, H, x6, pqg, p)
        p = _paths(monkeypatch, case, -1, {"GSAT_ATTN_FUSED": "1"})            # args.fused = -1 wins over the environment
        assert (p["fwd_kind"], p["fwd_pqg"], p["fwd_nrb"], p["fwd_ncbw"], p["slices"]) == (0, 0, 0, 0, 1)
        p = _paths(monkeypatch, case, 0, {})                                    # automatic: small batches stay staged
        assert p["fwd_kind"] == 0
        assert _paths(monkeypatch, case, 0, {"GSAT_ATTN_FUSED": "1"})["fwd_kind"] >= 1
    node = ec.make_case("regular", "boundaries", False, 64, True)
    assert _paths(monkeypatch, node, 1, {}, with_order=True)["fwd_kind"] == 0, "node mode with a row order has no one-launch forward"
    assert _paths(monkeypatch, ec.make_large_case(64), 0, {})["fwd_kind"] == 2


def test_expected_backward_paths_match_the_path_query(monkeypatch):
    import __graft_entry__ as ge
    ge.build()
    bwd = lambda p: {k[4:]: v for k, v in p.items() if k.startswith("bwd_")}
    for edge_mode in (False, True):
        for H in ec.BWD_STAGED_WIDTHS:
            case = ec.make_case("regular", "boundaries", edge_mode, H, True)
            base = dict(fused=0, ncht=0, dual_l2=0, dual_l1=0, pair_l2=0, pair_l1=0, split=1, merged=1)      # 769 rows: too few to pair
            assert bwd(_paths(monkeypatch, case, -1, {})) == base
            assert bwd(_paths(monkeypatch, case, -1, {"GSAT_ATTN_BWD_SPLIT": "0"})) == dict(base, split=0)
            assert bwd(_paths(monkeypatch, case, -1, {"GSAT_ATTN_BWD_MERGED": "0"})) == dict(base, merged=0)
            ncht = ec.FUSED_BWD_NCHT.get((edge_mode, H))
            want = dict(base, fused=1, ncht=ncht, merged=0) if ncht else base
            assert bwd(_paths(monkeypatch, case, -1, {"GSAT_ATTN_BWD_FUSED": "1"})) == want
            d = int(H <= ec.DUAL_GEMM_MAX_H)
            assert bwd(_paths(monkeypatch, case, -1, {"GSAT_DUAL_GEMM": "1"})) == dict(base, dual_l2=d, dual_l1=d)
    assert set(ec.FUSED_BWD_NCHT.values()) == {2, 4, 8}
    node = ec.make_case("regular", "boundaries", False, 64, True)
    assert bwd(_paths(monkeypatch, node, -1, {"GSAT_ATTN_BWD_FUSED": "1"}, with_order=True))["fused"] == 0


def test_path_query_rejects_a_short_buffer():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from dp_gsat_amd import _lib
    a = shape_args(ec.make_case("regular", "boundaries", False, 16, True), 0, False)
    out = (ctypes.c_int32 * len(_lib.ATTN_PATH_FIELDS))()
    assert _lib.load().gsat_attn_paths(ctypes.byref(a), out, len(out) - 1) != 0
    assert _lib.load().gsat_attn_paths(None, out, len(out)) != 0
    assert _lib.load().gsat_attn_paths(ctypes.byref(a), out, len(out)) == 0
