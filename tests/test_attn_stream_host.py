"""not gpu: the host side of the memory-bounded extractor.  gsat_attn_stream_plan (pure host code) over hand-written and random edge
pointers; the new symbols declared, exported and bound with the ABI still at 4; and the inputs that tests/test_gpu_attn_stream.py adds to
the table of tests/extractor_cases.py held to the same conditions on the reference alone as tests/test_extractor_cases_host.py holds
that table to."""
import os
import re

import numpy as np
import pytest
import torch

from tests import attn_stream_cases as sc
from tests import extractor_cases as ec
from tests import extractor_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsat_attn_stream_plan", "gsat_attn_stream_check", "gsat_attn_stream_fwd_workspace_bytes", "gsat_attn_stream_fwd",
           "gsat_attn_stream_bwd_workspace_bytes", "gsat_attn_stream_bwd")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _ptr(rows):
    return [0] + np.cumsum(rows).tolist()


def _plan(rows, budget):
    from tests.attn_stream_driver import host_plan
    return host_plan(_ptr(rows), budget)


def _check_rule(rows, budget):
    """The properties of the greedy rule, from the row counts alone."""
    G = len(rows)
    gp, scratch = _plan(rows, budget)
    if G == 0:
        assert gp == [0] and scratch == 1
        return gp, scratch
    assert gp[0] == 0 and gp[-1] == G and all(a < b for a, b in zip(gp, gp[1:])), f"{gp}: not a partition of [0, {G}) into runs"
    sums = [sum(rows[a:b]) for a, b in zip(gp, gp[1:])]
    for k, (a, b) in enumerate(zip(gp, gp[1:])):
        busy = [g for g in range(a, b) if rows[g] > 0]
        assert sums[k] <= budget or len(busy) == 1, f"group {k} = graphs [{a}, {b}) has {sums[k]} rows > {budget} and is not one graph"
        if k > 0:
            assert rows[a] > 0, f"group {k} opens with the empty graph {a}"
        if b < G:          # the group could not have taken the next non-empty graph (the one that opens the next group)
            assert sums[k] + rows[b] > budget, f"group {k} ({sums[k]} rows) had room for graph {b} ({rows[b]} rows) within {budget}"
    assert scratch == max(max(sums), 1)
    return gp, scratch


def test_plan_hand_written():
    assert _check_rule([4, 5, 32, 33, 64, 65, 128, 129, 257, 0, 12, 40], 64) == ([0, 3, 4, 5, 6, 7, 8, 10, 12], 257)
    assert _check_rule([3, 3, 3], 1) == ([0, 1, 2, 3], 3)                          # budget 1: every graph alone
    assert _check_rule([3, 3, 3], 6) == ([0, 2, 3], 6)                             # an exact fit closes the group
    assert _check_rule([3, 3, 3], 9) == ([0, 3], 9)
    assert _check_rule([3, 3, 3], 10 ** 6) == ([0, 3], 9)
    assert _check_rule([10, 2, 2, 10, 2], 4) == ([0, 1, 3, 4, 5], 10)              # oversize graphs are groups of their own
    assert _check_rule([0, 0, 5, 5], 5) == ([0, 3, 4], 5)                          # empties at the start join the first group
    assert _check_rule([5, 0, 0, 5], 5) == ([0, 3, 4], 5)                          # in the middle: the group before them
    assert _check_rule([5, 5, 0, 0], 5) == ([0, 1, 4], 5)                          # at the end likewise
    assert _check_rule([7, 0, 7], 5) == ([0, 2, 3], 7)                             # also behind an oversize graph
    assert _check_rule([0, 0, 0], 5) == ([0, 3], 1)                                # all empty: one group, scratch of one row
    assert _check_rule([], 5) == ([0], 1)                                          # G = 0: no group
    assert _check_rule([0], 1) == ([0, 1], 1)


def test_plan_random():
    rng = np.random.RandomState(5)
    for _ in range(300):
        G = int(rng.randint(0, 40))
        rows = [int(r) if rng.rand() > 0.25 else 0 for r in rng.randint(1, 50, size=G)]
        for budget in (1, 7, 49, 50, 120, 10 ** 6, int(rng.randint(1, 200))):
            _check_rule(rows, budget)


def test_plan_rejects_bad_arguments():
    import ctypes
    from dp_gsat_amd import _lib
    lib = _lib.load()
    seg = (ctypes.c_int32 * 3)(0, 4, 2)                                            # not monotone
    gp = (ctypes.c_int32 * 3)()
    n, r = ctypes.c_int64(), ctypes.c_int64()
    assert lib.gsat_attn_stream_plan(seg, 2, 8, gp, ctypes.byref(n), ctypes.byref(r)) != 0
    seg = (ctypes.c_int32 * 3)(0, 2, 4)
    assert lib.gsat_attn_stream_plan(seg, 2, 0, gp, ctypes.byref(n), ctypes.byref(r)) != 0, "budget 0"
    assert lib.gsat_attn_stream_plan(seg, 2, 8, None, ctypes.byref(n), ctypes.byref(r)) != 0
    assert lib.gsat_attn_stream_plan(seg, 2, 8, gp, ctypes.byref(n), ctypes.byref(r)) == 0 and (n.value, r.value) == (1, 4)


def test_symbols_are_declared_exported_and_bound():
    from dp_gsat_amd import _lib
    header = open(os.path.join(ROOT, "include", "gsat_hip.h")).read()
    assert re.search(r"#define\s+GSAT_ABI_VERSION\s+4\b", header)
    lib = _lib.load()
    assert lib.gsat_abi_version() == 4
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/gsat_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from dp_gsat_amd._lib.SIGNATURES"
        assert getattr(lib, name) is not None
    assert _lib.SIGNATURES["gsat_attn_stream_fwd_workspace_bytes"][0] is _lib.SZ and _lib.SIGNATURES["gsat_attn_stream_bwd_workspace_bytes"][0] is _lib.SZ


def test_workspace_queries_are_host_arithmetic_and_smaller_than_one_activation():
    """The shape of the memory test of tests/test_gpu_attn_stream_module.py: 8 graphs of 2560 rows on 160 nodes each, H = 64."""
    from tests.attn_stream_driver import workspace_bytes
    M, C1, C2 = 8 * 2560, 256, 64
    fwd, bwd, gp, scratch = workspace_bytes([2560] * 8, [160] * 8, 64, 2560)
    assert (gp, scratch) == (list(range(9)), 2560)
    act = M * C1 * 4
    assert scratch * C1 * 4 <= fwd < act / 4, (fwd, act)
    assert 2 * scratch * C1 * 4 + M * C2 * 4 <= bwd < act, (bwd, act)


@pytest.mark.parametrize("name", list(sc.BUILDERS))
def test_added_cases_meet_the_conditions_on_the_reference(name):
    """RELU_MARGIN and 4 * |r32 - r64| <= cap for every tensor the GPU tests compare, at the recorded draw -- and that draw is the first
    that passes."""
    def passes(case, refs):
        r32, r64 = refs
        for k in ec.FWD_TENSORS + ec.GRAD_TENSORS:
            if k in sc.NO_SLACK.get(name, ()):          # compared without the slack term: see attn_stream_cases.NO_SLACK
                if float(r64[k].abs().max()) > sc.EXACT_ZERO:
                    return f"{k}: the fp64 reference is not zero"
                continue
            g, scale = eo.gap(r32[k], r64[k])
            if 4.0 * g > ec.cap_for("regular", k) * scale:
                return f"{k}: 4 * |r32 - r64| = {4 * g:.3e} > cap {ec.cap_for('regular', k):.1e} * scale {scale:.3e}"
        if r64["relu_margin"] < ec.RELU_MARGIN:
            return f"a pre-activation lies {r64['relu_margin']:.2e} from the kink of ReLU"
        if not bool(((r32["a1"] > 0) == (r64["a1"] > 0)).all()):
            return "the fp32 and fp64 references disagree on a ReLU sign"
        return None
    case = sc.make_stream_case(name)
    assert case["edge_mode"] and case["training"] and case["H"] == sc.H
    assert all(r == 0 or r >= ec.MIN_ROWS for r in case["rows"].tolist())
    seg = case["batch"][case["ei"][0]]
    assert bool((seg[1:] >= seg[:-1]).all()) and bool((seg == case["batch"][case["ei"][1]]).all())
    why = passes(case, sc.stream_references(name))
    assert why is None, why
    for earlier in range(sc.REDRAW[name]):
        c = sc.make_stream_case(name, earlier)
        assert passes(c, (eo.reference_one(c, torch.float32), eo.reference_one(c, torch.float64))) is not None, f"draw {earlier} passes already"
    if name == "hub":
        deg = torch.bincount(case["ei"][0], minlength=case["N"])
        assert int(deg.max()) == sc.STAR_LEAVES > 256 and case["rows"].tolist() == [40, 600, 12]
