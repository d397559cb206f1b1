"""not gpu: the task-log oracle of tests/fidelity_tasks_oracle.py against tests/fidelity_curve_oracle.py at one task and column by column;
what the multi-task label fixtures of tests/multitask.py contain; the C ABI of the two task-log entry points."""
import ctypes
import os
import re

import numpy as np

from tests import evaluate_oracle as eo
from tests import fidelity_curve_oracle as fco
from tests import fidelity_tasks_oracle as fto
from tests import multitask as mt
from tests import padded_oracle as po
from tests import ragged_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gsat_fidelity_curve_append_tasks", "gsat_fidelity_curve_reduce_tasks")


def _case(seed, Gp, S, T):
    rng = np.random.RandomState(seed)
    V = 2 * S + 1
    z = (rng.randn(V * Gp, T) * 3).astype(np.float32)
    E = 300
    keep = np.sort(rng.randint(0, E + 1, size=S))
    return z, keep, E


def test_task_oracle_at_one_task_is_the_curve_oracle():
    for seed, (Gp, S) in enumerate([(1, 1), (9, 3), (33, 16)]):
        z, keep, E = _case(seed, Gp, S, 1)
        g = max(Gp - 2, 1)
        levels = list(range(1, S + 1))
        c1, p1 = fco.rows(z, Gp, S, g)
        ct, pt = fto.rows(z, Gp, S, g, 1)
        assert ct.shape == (g, 1, 2 * S + 1) and np.array_equal(ct[:, 0], c1) and np.array_equal(pt[:, 0], p1)
        want, got = fco.compute(c1, p1, S, keep, E, levels), fto.compute(ct, pt, S, keep, E, levels)
        for key, v in want.items():
            assert got[key] == v, key                                       # the mean over one task is that task's mean, bit for bit
        for key in fto.TASK_KEYS:
            assert [row[0] for row in got[key + "_tasks"]] == want[key], key
        assert got["p_full_tasks"] == [want["p_full"]]


def test_task_oracle_is_the_curve_oracle_column_by_column():
    Gp, S, T = 11, 3, 4
    z, keep, E = _case(7, Gp, S, T)
    cls, p = fto.rows(z, Gp, S, Gp, T)
    res = fto.compute(cls, p, S, keep, E, [1, 2, 3])
    for t in range(T):
        c1, p1 = fco.rows(z[:, t:t + 1], Gp, S, Gp)
        assert np.array_equal(cls[:, t], c1) and np.array_equal(p[:, t], p1)
        one = fco.compute(c1, p1, S, keep, E, [1, 2, 3])
        for key in fto.TASK_KEYS:
            assert [res[key + "_tasks"][s][t] for s in range(S)] == one[key], (t, key)
    for key in fto.TASK_KEYS:                                               # every graph counts for every task: the flat mean
        for s in range(S):
            assert res[key][s] == float(np.mean(np.array(res[key + "_tasks"][s])))
    flat = (p[:, :, :1] - p[:, :, 1 + S:]).reshape(-1, S).mean(axis=0)
    assert np.allclose(res["fidelity_plus"], flat, rtol=0, atol=1e-15)


def test_label_fixtures_hold_the_cases_the_gpu_tests_rely_on():
    """Under the numpy ROC oracle: at least two scorable tasks, exactly one task with a single class among its labelled rows, NaNs in
    every column, and one column that is NaN throughout one budget batch of range(48)."""
    graphs = po.mutag_graphs(**po.STEP_GRAPHS)
    y = mt.task_labels(graphs)
    assert y.shape == (48, mt.T) and y.dtype == np.float32
    frac = np.isnan(y).mean()
    assert 0.1 < frac < 0.4 and np.isnan(y).any(axis=0).all()
    counts = eo.task_counts_oracle(np.zeros_like(y), y)
    scorable = [int(P) > 0 and int(Nn) > 0 for _, P, Nn in counts]
    assert sum(scorable) >= 2 and scorable.count(False) == 1 and not scorable[mt.UNSCORABLE]
    assert int(counts[mt.UNSCORABLE][1]) > 0 and int(counts[mt.UNSCORABLE][2]) == 0          # labelled, and all of one class
    n, e = po.sizes(graphs)
    batches = ro.budget_batches(n, e, range(48), ro.RAGGED_CAPACITY, ro.RAGGED_SLOTS)
    assert [len(b) for b in batches] == ro.RAGGED_SIZES and batches[1] == list(mt.NAN_GRAPHS)
    assert np.isnan(y[batches[1], mt.NAN_TASK]).all() and not np.isnan(y[batches[1]]).all()
    per = mt.roc_tasks_oracle(np.random.RandomState(0).randn(*y.shape).astype(np.float32), y)
    assert np.isnan(per[mt.UNSCORABLE]) and np.isfinite(np.delete(per, mt.UNSCORABLE)).all()
    # the same holds for the 40 graphs the fixed-count evaluation tests use
    c40 = eo.task_counts_oracle(np.zeros((40, mt.T), np.float32), mt.task_labels(graphs[:40]))
    assert [int(P) > 0 and int(Nn) > 0 for _, P, Nn in c40] == scorable


def test_header_declares_the_task_log_symbols_and_signatures_match():
    import __graft_entry__ as ge
    ge.build()
    from dp_gsat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsat_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/gsat_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        args = [a.strip() for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        res, sig = _lib.SIGNATURES[name]
        assert len(sig) == len(args), (name, len(sig), args)
        for a, c in zip(args, sig):
            want = _lib.P if "*" in a else {"int64_t": _lib.I64, "size_t": _lib.SZ, "int": _lib.INT, "double": _lib.F64}[a.split()[0]]
            assert c is want, (name, a, c)
        assert res is _lib.INT, name
