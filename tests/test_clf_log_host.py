"""not gpu: the classifier-log oracle against brute force and tests/evaluate_oracle.py on the same rows, and the declarations of the new
entry points."""
import os
import re

import numpy as np
import pytest

from tests import clf_log_oracle as co
from tests import evaluate_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsat_clf_log_append", "gsat_clf_log_counts", "gsat_clf_log_counts_words")


def eighths(rng, shape):
    """Multiples of 1/8 in [-4, 4], exact 0 included: z > 0 and sigmoid(z) > 0.5 agree on all of them."""
    return (rng.randint(-32, 33, size=shape) / 8.0).astype(np.float32)


def _rows(mode, n, seed):
    rng = np.random.RandomState(seed)
    if mode == 0:
        return eighths(rng, (n, 1)), (rng.rand(n, 1) < 0.5).astype(np.float32)
    if mode == 1:
        z = eighths(rng, (n, 3))
        z[::4, 1] = z[::4, 0]                                               # tied maxima are common at this grid anyway
        return z, rng.randint(0, 3, size=(n, 1)).astype(np.float32)
    y = (rng.rand(n, 3) < 0.5).astype(np.float32)
    y[rng.rand(n, 3) < 0.25] = np.nan
    return eighths(rng, (n, 3)), y


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_oracle_equals_brute_force_on_the_concatenation(mode):
    multi, cols = mode == 2, (1, 3, 3)[mode]
    sizes = (5, 0, 300, 1)
    log = co.ClfLogOracle(sum(sizes) + 7, len(sizes) + 1, cols, 3 if multi else 1, multi)
    zs, ys, losses = [], [], []
    for i, n in enumerate(sizes):
        z, y = _rows(mode, n, 40 + i)
        loss = np.float32(0.25 * (i + 1))
        log.append(z, y, loss)
        zs.append(z); ys.append(y); losses.append(loss)
    z, y = np.concatenate(zs), np.concatenate(ys)
    assert log.state.tolist() == [sum(sizes), len(sizes), 0, 0]
    assert (log.logits[sum(sizes):].view(np.int32) == co.ClfLogOracle.SENTINEL).all()
    res = log.compute()
    assert res["n"] == sum(sizes) and res["loss"] == float(np.sum(np.float64(losses)) / len(sizes))
    # the accuracy of tests/evaluate_oracle.py (get_preds restated) and a brute-force confusion matrix
    assert res["clf_acc"] == eo.accuracy_oracle(z, y, multi)
    if multi:
        for t in range(3):
            have = ~np.isnan(y[:, t])
            p, lab = z[have, t] > 0, y[have, t] != 0
            want = [int((~p & ~lab).sum()), int((p & ~lab).sum()), int((~p & lab).sum()), int((p & lab).sum())]
            assert res["task_counts"][t].tolist() == want and res["unlabelled"][t] == int((~have).sum())
        assert res["clf_roc"] == eo.rocauc_oracle(z, y)
    else:
        C = 2 if mode == 0 else 3
        pred = (z[:, 0] > 0).astype(int) if mode == 0 else np.array([min(c for c in range(3) if r[c] == r.max()) for r in z])
        want = np.zeros((C, C), dtype=np.int64)
        np.add.at(want, (y[:, 0].astype(int), pred), 1)
        assert np.array_equal(res["confusion"], want) and res["bad"] == 0
        assert res["clf_roc"] == (eo.rocauc_oracle(z, y) if mode == 0 else 0.0)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_oracle_of_a_log_without_rows(mode):
    multi, cols = mode == 2, (1, 3, 3)[mode]
    log = co.ClfLogOracle(4, 2, cols, 3 if multi else 1, multi)
    z, y = _rows(mode, 0, 1)
    log.append(z, y, 0.5)
    res = log.compute()
    assert res["n"] == 0 and res["loss"] == 0.5 and np.isnan(res["clf_acc"]) and (mode == 1 or np.isnan(res["clf_roc"]))


def test_oracle_bad_rows_match_nothing():
    z = np.array([[1.0, 0.5, 0.0], [np.nan, 3.0, 0.0], [0.0, 0.0, 0.0], [2.0, 2.0, 2.5], [0.0, 1.0, 0.0]], dtype=np.float32)
    y = np.array([[0], [1], [3], [2], [1.5]], dtype=np.float32)             # a NaN logit, a label out of range, a label that is no integer
    c = co.counts_oracle(z, y, 1)
    assert c[9] == 3 and c[:9].reshape(3, 3).tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 1]]
    c = co.counts_oracle(np.array([[np.nan], [1.0], [-1.0], [0.0]], dtype=np.float32), np.array([[1], [1], [np.nan], [0]], dtype=np.float32), 0)
    assert c.tolist() == [1, 0, 0, 1, 2]


def test_oracle_flags_and_padded_counts():
    z, y = _rows(0, 6, 3)
    for caps in ((5, 2), (6, 0)):                                           # past max_graphs, past max_batches
        log = co.ClfLogOracle(caps[0], caps[1], 1)
        before = log.logits.copy()
        log.append(z, y, 1.0)
        assert log.state.tolist() == [0, 0, co.FLAG_FULL, 0] and log.loss_sum[0] == 0.0
        assert np.array_equal(log.logits.view(np.uint8), before.view(np.uint8))
        with pytest.raises(ValueError, match="flag bit 1"):
            log.compute()
    log = co.ClfLogOracle(12, 4, 1)
    with pytest.raises(ValueError, match="before any append"):
        log.compute()
    log.append(z, y, 1.0, valid=[0, 0, 3, 0])                               # a padded batch: 3 of 6 rows
    log.append(z, y, 2.0, valid=[0, 0, 0, 0])                               # a count of 0 is a batch with no rows
    assert log.state.tolist() == [3, 2, 0, 0] and log.loss_sum[0] == 3.0
    assert np.array_equal(log.logits[:3], z[:3]) and (log.logits[3:].view(np.int32) == co.ClfLogOracle.SENTINEL).all()
    log.append(z, y, 1.0, valid=[0, 0, 7, 0])                               # a count beyond the batch's own rows
    assert log.state.tolist() == [3, 2, co.FLAG_FULL, 0]
    log.reset()
    log.append(z, y, 1.0, valid=[0, 0, 6, 1])                               # the overflow word
    assert log.state.tolist() == [0, 0, co.FLAG_OVERFLOW, 0]
    with pytest.raises(ValueError, match="flag bit 0"):
        log.compute()
    log.reset()
    log.append(z, y)                                                        # no loss: the mean turns NaN
    assert np.isnan(log.compute()["loss"])


def test_header_and_signatures_list_the_new_entry_points():
    from dp_gsat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsat_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gsat_[a-z0-9_]+)\s*\(", txt))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/gsat_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
    assert re.search(r"#define\s+GSAT_ABI_VERSION\s+4\b", txt)
    res, args = _lib.SIGNATURES["gsat_clf_log_append"]
    assert res is _lib.INT and args[-1] is _lib.P and len(args) == 14          # an int status, the stream last
    res, args = _lib.SIGNATURES["gsat_clf_log_counts"]
    assert res is _lib.INT and args[-1] is _lib.P and len(args) == 9
    import dp_gsat_amd as G
    assert G.ClfLog.__module__ == "dp_gsat_amd.eval_log"
    assert G.ReplayedClfStep.__module__ == "dp_gsat_amd.replay" and G.ReplayedClfEval.__module__ == "dp_gsat_amd.replay"
    assert G.pretrain_clf.__module__ == "dp_gsat_amd.pretrain"
