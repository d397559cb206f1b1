"""-m gpu: every dispatch path of the attention extractor (csrc/attn.hip, attn_fused.hip, attn_fused_bwd.hip, dual_gemm.hip) against the
fp64 reference of tests/extractor_oracle.py, on the seeded cases of tests/extractor_cases.py.

Every test sets all seven switches itself, asks gsat_attn_paths what the library will run for exactly the arguments of the call and asserts
that it is the path the test names; a parametrisation outside a path's reach asserts that the query says so and checks the fallback just
the same.  Comparisons go through close64: |actual - r64|max <= TOL * scale + 4 * |r32 - r64|max, with the slack term capped per family
(tests/test_extractor_cases_host.py asserts the caps on the reference alone)."""
import pytest
import torch

from tests import extractor_cases as ec
from tests import extractor_oracle as eo
from tests.extractor_driver import run

pytestmark = pytest.mark.gpu

SWITCHES = ("GSAT_ATTN_FUSED", "GSAT_ATTN_FUSED_X6", "GSAT_ATTN_FUSED_PQG", "GSAT_ATTN_BWD_FUSED", "GSAT_ATTN_BWD_SPLIT",
            "GSAT_ATTN_BWD_MERGED", "GSAT_DUAL_GEMM")
WORST = {}          # path label -> worst err / allowed seen, printed when the module is done (pytest -s)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst error against fp64 as a multiple of the allowed error, per path:")
    for k in sorted(WORST):
        print(f"  {k:<44s} {WORST[k][0]:.3f}  ({WORST[k][1]})")


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _compare(label, out, refs, family, tensors, what):
    r32, r64 = refs
    for k in tensors:
        if r64.get(k) is None:
            continue
        if k in ("var1", "var2"):          # the library saves 1/sigma, which amplifies the rounding of a nearly constant channel: compare var + eps
            a, b32, b64 = out["rstd" + k[-1]].double() ** -2, r32[k] + eo.EPS, r64[k] + eo.EPS
        else:
            a, b32, b64 = out[k], r32[k], r64[k]
        ratio = eo.close64(a.reshape(b64.shape), b32, b64, f"{what}: {k}", ec.cap_for(family, k))
        if ratio > WORST.get(label, (0.0, ""))[0]:
            WORST[label] = (ratio, f"{k}, {what}")


# ---- forward ------------------------------------------------------------------------------------------------------------------------
# name -> (args.fused, environment, seg_order)
FWD_PATHS = {
    "staged": (-1, {}, "auto"),
    "staged_no_order": (-1, {}, "none"),                   # edge mode: edges grouped by graph, no row order
    "staged_identity_order": (1, {}, "identity"),          # node mode with a row order: the one-launch forward is asked for and out of reach
    "fused_x6": (1, {}, "auto"),
    "fused_fp32": (1, {"GSAT_ATTN_FUSED_X6": "0"}, "auto"),
    "fused_x6_in_tile": (1, {"GSAT_ATTN_FUSED_PQG": "0"}, "auto"),
    "fused_fp32_in_tile": (1, {"GSAT_ATTN_FUSED_X6": "0", "GSAT_ATTN_FUSED_PQG": "0"}, "auto"),
}
NODE_FWD = ("staged", "staged_identity_order", "fused_x6", "fused_fp32")
EDGE_FWD = ("staged", "staged_no_order", "fused_x6", "fused_fp32", "fused_x6_in_tile", "fused_fp32_in_tile")


def _expected_forward(path, edge_mode, H):
    """What gsat_attn_paths must report for the forward of ``path`` at this width, from the tables of extractor_cases."""
    fused, env, order = FWD_PATHS[path]
    if fused < 0 or (not edge_mode and order == "identity"):
        return dict(fwd_kind=0, fwd_pqg=0, fwd_nrb=0, fwd_ncbw=0)
    e = ec.FUSED_FWD_EXPECT[(edge_mode, H)]
    x6 = env.get("GSAT_ATTN_FUSED_X6") != "0" and e["x6"]
    pqg = env.get("GSAT_ATTN_FUSED_PQG") != "0" and e["pqg"]
    return dict(fwd_kind=2 if x6 else 1, fwd_pqg=int(bool(pqg)), fwd_nrb=e["nrb"], fwd_ncbw=e["ncbw"])


def _forward_case(dev, monkeypatch, family, name, edge_mode, H, training, path):
    fused, env, order = FWD_PATHS[path]
    case = ec.make_case(family, name, edge_mode, H, training, sorted_edges=(order == "none"))
    _env(monkeypatch, env)
    out = run(dev, case, fused=fused, order=order, backward=False)
    want = _expected_forward(path, edge_mode, H)
    assert {k: out["paths"][k] for k in want} == want, out["paths"]
    assert out["paths"]["slices"] == 1
    for k in ("logits", "att", "P", "Q", "a1", "h2", "stats"):
        assert out[k] is None or not torch.isnan(out[k]).any(), f"{k}: the forward left entries unwritten"
    kind = ("staged", "fused fp32", "fused x6")[want["fwd_kind"]] + (" P|Q in tile" if edge_mode and want["fwd_kind"] and not want["fwd_pqg"] else "")
    label = f"fwd {'edge' if edge_mode else 'node'} {kind}" + (f" nrb{want['fwd_nrb']} ncbw{want['fwd_ncbw']}" if want["fwd_kind"] else "") + f" [{family}]"
    _compare(label, out, eo.references(case), family, ec.FWD_TENSORS, f"{path} {name} H={H} train={training}")


def _fwd_params():
    ps = []
    for edge_mode, paths in ((False, NODE_FWD), (True, EDGE_FWD)):
        for path in paths:
            hs = ec.FWD_WIDTHS + (ec.FUSED_EXTRA_WIDTHS if path.startswith("fused") else ())
            ps += [(edge_mode, path, H) for H in hs]
    return ps


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("edge_mode,path,H", _fwd_params())
def test_forward_path_regular(dev, monkeypatch, edge_mode, path, H, training):
    _forward_case(dev, monkeypatch, "regular", "boundaries", edge_mode, H, training, path)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", list(ec.TINY))
@pytest.mark.parametrize("edge_mode,path,H", [p for p in _fwd_params() if p[2] in ec.TINY_WIDTHS and p[1] != "staged_no_order"])
def test_forward_path_tiny(dev, monkeypatch, edge_mode, path, H, name, training):
    _forward_case(dev, monkeypatch, "tiny", name, edge_mode, H, training, path)


# ---- backward -----------------------------------------------------------------------------------------------------------------------
BWD_PATHS = {
    "staged": {},                                          # split-bf16 GEMMs, paired where gsat_gemm_pair_plan pairs them (large batches)
    "staged_fp32": {"GSAT_ATTN_BWD_SPLIT": "0"},
    "staged_unmerged": {"GSAT_ATTN_BWD_MERGED": "0"},
    "fused": {"GSAT_ATTN_BWD_FUSED": "1"},
    "dual": {"GSAT_DUAL_GEMM": "1"},
}


def _pair_plan(R, Cg, Co, Cy):
    import ctypes
    from dp_gsat_amd._lib import call
    plan = (ctypes.c_int32 * 4)()
    call("gsat_gemm_pair_plan", R, Cg, Co, Cy, plan)
    return int(plan[0])


def _expected_backward(path, case):
    """What gsat_attn_paths must report for the backward of ``path`` on ``case``."""
    edge_mode, H, M, N = case["edge_mode"], case["H"], case["M"], case["N"]
    _, C1, C2 = ec.widths(edge_mode, H)
    env = BWD_PATHS[path]
    split = env.get("GSAT_ATTN_BWD_SPLIT") != "0"
    ncht = ec.FUSED_BWD_NCHT.get((edge_mode, H), 0) if path == "fused" else 0
    dual = int(path == "dual" and H <= ec.DUAL_GEMM_MAX_H)
    want = dict(bwd_fused=int(ncht > 0), bwd_ncht=ncht, bwd_dual_l2=dual, bwd_dual_l1=dual, bwd_split=int(split),
                bwd_merged=int(not ncht and env.get("GSAT_ATTN_BWD_MERGED") != "0"))
    want["bwd_pair_l2"] = int(split and not ncht and not dual and _pair_plan(M, C2, C1, C1))
    want["bwd_pair_l1"] = int(split and not dual and not edge_mode and _pair_plan(N, C1, H, H))
    return want


def _bwd_label(case, want):
    p = want
    how = f"fused ncht{p['bwd_ncht']}" if p["bwd_fused"] else "staged" + ("" if p["bwd_merged"] else " unmerged")
    l2 = "" if p["bwd_fused"] else (" l2:dual" if p["bwd_dual_l2"] else " l2:pair" if p["bwd_pair_l2"] else "")
    l1 = " l1:dual" if p["bwd_dual_l1"] else " l1:pair" if p["bwd_pair_l1"] else ""
    return f"bwd {'edge' if case['edge_mode'] else 'node'} {how}{l2}{l1} {'split-bf16' if p['bwd_split'] else 'fp32'} [{case['family']}]"


def _backward_case(dev, monkeypatch, case, refs, path, fwd=(-1, {}), dlogits=True, datt=True, what=""):
    _env(monkeypatch, dict(fwd[1], **BWD_PATHS[path]))
    out = run(dev, case, fused=fwd[0], backward=True, dlogits=dlogits, datt=datt)
    want = _expected_backward(path, case)
    assert {k: out["paths"][k] for k in want} == want, out["paths"]
    assert out["paths"]["slices"] == 1
    what = f"{path} {case['name']} H={case['H']} train={case['training']} {what}"
    _compare(_bwd_label(case, want), out, refs, case["family"], ec.GRAD_TENSORS, what)
    assert not bool(out["db1"].any()) and not bool(out["db2"].any()), "a bias in front of an InstanceNorm has an exactly zero gradient"
    return out, want


def _bwd_params(tiny):
    ps = []
    for path in BWD_PATHS:
        hs = ec.TINY_WIDTHS if tiny else (ec.BWD_STAGED_WIDTHS if path.startswith("staged") else ec.BWD_WIDTHS + (256,))
        ps += [(path, H) for H in hs]          # H = 256 on "fused" / "dual": beyond both, falls back to the staged kernels
    return ps


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("edge_mode", [False, True])
@pytest.mark.parametrize("path,H", _bwd_params(False))
def test_backward_path_regular(dev, monkeypatch, path, H, edge_mode, training):
    case = ec.make_case("regular", "boundaries", edge_mode, H, training)
    _backward_case(dev, monkeypatch, case, eo.references(case), path)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("edge_mode", [False, True])
@pytest.mark.parametrize("name", list(ec.TINY))
@pytest.mark.parametrize("path,H", _bwd_params(True))
def test_backward_path_tiny(dev, monkeypatch, path, H, name, edge_mode, training):
    case = ec.make_case("tiny", name, edge_mode, H, training)
    _backward_case(dev, monkeypatch, case, eo.references(case), path)


@pytest.mark.parametrize("given", ["datt_only", "dlogits_only"])
@pytest.mark.parametrize("edge_mode", [False, True])
@pytest.mark.parametrize("path", ["staged", "fused"])
def test_backward_with_one_upstream_gradient(dev, monkeypatch, path, edge_mode, given):
    base = ec.make_case("regular", "boundaries", edge_mode, 64, True)
    zeroed = "dlogits" if given == "datt_only" else "datt"
    case = dict(base, **{zeroed: torch.zeros_like(base[zeroed])})          # the reference sees a zero where the library sees NULL
    refs = eo.references(case, key=("one_gradient", edge_mode, given))
    _backward_case(dev, monkeypatch, case, refs, path, dlogits=(given == "dlogits_only"), datt=(given == "datt_only"), what=given)


FWD_KINDS = {0: (-1, {}), 1: (1, {"GSAT_ATTN_FUSED_X6": "0"}), 2: (1, {})}


@pytest.mark.parametrize("edge_mode", [False, True])
@pytest.mark.parametrize("path", list(BWD_PATHS))
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_backward_after_each_forward_kind(dev, monkeypatch, kind, path, edge_mode):
    """The one-launch forward writes the buffers every backward reads (P | Q, a1, h2, statistics, att)."""
    case = ec.make_case("regular", "boundaries", edge_mode, 64, True)
    out, _ = _backward_case(dev, monkeypatch, case, eo.references(case), path, fwd=FWD_KINDS[kind], what=f"after forward kind {kind}")
    assert out["paths"]["fwd_kind"] == kind


@pytest.mark.parametrize("H", ec.LARGE_WIDTHS)
def test_large_batch_takes_the_automatic_paths(dev, monkeypatch, H):
    """The default large-batch step of node mode, nothing forced: the split-bf16 one-launch forward, then the staged backward -- with its
    GEMM pairs as one launch each where the widths allow whole 128 x 128 tiles of the weight gradient (H = 128: da1 | dW2 and demb | dW1;
    at H = 64 neither dW2 [64, 128] nor dW1 [128, 64] qualifies, and the query says so)."""
    case = ec.make_large_case(H)
    refs = eo.references(case, key=("large", H))
    _env(monkeypatch, {})
    out = run(dev, case, fused=0, order="auto")
    p = out["paths"]
    want = _expected_backward("staged", case)
    assert {k: p[k] for k in want} == want, p
    assert (p["fwd_kind"], p["fwd_nrb"], p["fwd_ncbw"], p["slices"]) == (2, 2, 1, 1), p
    assert (p["bwd_pair_l2"], p["bwd_pair_l1"]) == ((1, 1) if H == 128 else (0, 0)), p
    label = f"large node H={H}: fwd fused x6, {_bwd_label(case, want)}"
    _compare(label, out, refs, "regular", ec.FWD_TENSORS + ec.GRAD_TENSORS, f"large H={H}")
