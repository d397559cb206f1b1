"""-m gpu: the device classifier log (csrc/clf_log.hip, dp_gsat_amd.ClfLog) against tests/clf_log_oracle.py.  Counts are exact; the logged
arrays are compared word for word, NaN payloads included; everything an append must not touch is pre-filled with a NaN pattern and
checked afterwards.  The logits are multiples of 1/8 in [-4, 4] with exact zeros: on these ``z > 0`` and ``get_preds``'s ``sigmoid(z) >
0.5`` agree everywhere, so ``clf_acc`` must equal ``classifier_accuracy`` on the same rows exactly."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import clf_log_oracle as co
from tests.test_clf_log_host import _rows

pytestmark = pytest.mark.gpu
SENT = co.ClfLogOracle.SENTINEL
MODES = {0: (1, 1, False), 1: (3, 1, False), 2: (3, 3, True)}            # mode -> (logit_cols, y_cols, multi_label)


def _new(dev, mode, max_graphs, max_batches):
    import dp_gsat_amd as G
    cols, y_cols, multi = MODES[mode]
    log = G.ClfLog(max_graphs, max_batches, cols, y_cols, multi, dev)
    log.logits.view(torch.int32).fill_(SENT)
    log.y.view(torch.int32).fill_(SENT)
    return log, co.ClfLogOracle(max_graphs, max_batches, cols, y_cols, multi)


def _append(log, oracle, dev, z, y, loss=None, valid=None):
    zt, yt = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    data = NS(y=yt, num_graphs=z.shape[0])
    if valid is not None:
        data.valid = torch.tensor(valid, dtype=torch.int32, device=dev)
    log.append(data, zt, None if loss is None else torch.tensor(loss, dtype=torch.float32, device=dev))
    oracle.append(z, y, loss, valid)


def _words(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _assert_arrays(log, oracle, what):
    torch.cuda.synchronize()
    assert log.state.tolist() == oracle.state.tolist(), what
    assert np.array_equal(_words(log.logits), oracle.logits.view(np.int32)), what + ": logits"
    assert np.array_equal(_words(log.y), oracle.y.view(np.int32)), what + ": y"
    assert np.array_equal(_words(log.loss_sum), oracle.loss_sum.view(np.int32)), what + ": loss_sum"


def _same(got, want, what):
    assert set(got) == set(want), what
    for key, w in want.items():
        g = got[key]
        if isinstance(w, np.ndarray):
            assert np.array_equal(g, w, equal_nan=w.dtype.kind == "f"), f"{what}: {key}"
        elif key == "clf_roc" and "clf_roc_tasks" in want and np.isfinite(w):
            assert abs(g - w) <= 4 * 2.0 ** -53, f"{what}: {key}"          # a mean of at most three values in [0, 1], in either order
        elif key == "clf_acc" and np.isfinite(w):
            # the hits are in the counts, compared exactly above or below; the quotient in [0, 1] is formed on the device like
            # classifier_accuracy's (exact equality with it is asserted by the caller), where the division may round twice
            assert abs(g - w) <= 2 * 2.0 ** -53, f"{what}: {key}"
        else:
            assert g == w or (np.isnan(g) and np.isnan(w)), f"{what}: {key} {g!r} != {w!r}"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_appends_and_scores_equal_the_oracle(dev, mode):
    """Unpadded batches of 5, 0, 300 and 1 rows, a padded batch with 3 of 6 rows and a padded batch with none: the arrays word for word,
    compute() against the oracle and clf_acc against classifier_accuracy on the same rows; then reset, and the same again."""
    import dp_gsat_amd as G
    multi = MODES[mode][2]
    log, oracle = _new(dev, mode, 320, 8)
    with pytest.raises(ValueError, match="before any append"):
        log.compute()
    for round_ in range(2):
        for i, n in enumerate((5, 0, 300, 1)):
            z, y = _rows(mode, n, 40 + i + 10 * round_)
            _append(log, oracle, dev, z, y, 0.25 * (i + 1))
        z, y = _rows(mode, 6, 50)
        _append(log, oracle, dev, z, y, 1.5, valid=[11, 22, 3, 0])
        _append(log, oracle, dev, z, y, 0.125, valid=[0, 0, 0, 0])
        assert oracle.state.tolist() == [309, 6, 0, 0]
        _assert_arrays(log, oracle, f"mode {mode} round {round_}")
        got = log.compute()
        _same(got, oracle.compute(), f"mode {mode} round {round_}")
        again = log.compute()                                               # repeatable: the counters are integers, the sums ordered
        _same(again, got, f"mode {mode} round {round_}: a second compute")
        assert again["clf_acc"] == got["clf_acc"] and again["clf_roc"] == got["clf_roc"] and again["loss"] == got["loss"]      # bit for bit
        acc = float(G.classifier_accuracy(log.logits[:309], log.y[:309].reshape(309, -1) if multi else log.y[:309], multi))
        assert got["clf_acc"] == acc
        log.reset()
        oracle.reset()
        assert log.state.tolist() == [0, 0, 0, 0] and log.loss_sum.tolist() == [0.0]
        with pytest.raises(ValueError, match="before any append"):
            log.compute()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [0, 1, 5, 300])
def test_row_counts(dev, mode, n):
    """One batch of n rows alone: 300 crosses the 256-thread block, and with 3 columns the grid stride."""
    log, oracle = _new(dev, mode, 300, 1)
    z, y = _rows(mode, n, 7 + n)
    _append(log, oracle, dev, z, y, 0.5)
    _assert_arrays(log, oracle, f"mode {mode}, {n} rows")
    _same(log.compute(), oracle.compute(), f"mode {mode}, {n} rows")


def test_refused_appends_write_nothing_but_their_flag(dev):
    z, y = _rows(0, 6, 3)
    log, oracle = _new(dev, 0, 12, 2)
    _append(log, oracle, dev, z, y, 1.0, valid=[0, 0, 3, 0])
    _append(log, oracle, dev, z, y, 1.0, valid=[0, 0, 6, 1])               # the overflow word: flag bit 0, nothing else
    assert oracle.state.tolist() == [3, 1, 1, 0]
    _assert_arrays(log, oracle, "overflow word")
    with pytest.raises(ValueError, match="flag bit 0"):
        log.compute()
    log.reset(); oracle.reset()
    _append(log, oracle, dev, z, y, 1.0)
    _append(log, oracle, dev, z, y, 1.0)
    _append(log, oracle, dev, z, y, 1.0)                                    # past max_batches
    assert oracle.state.tolist() == [12, 2, 2, 0]
    _assert_arrays(log, oracle, "past max_batches")
    with pytest.raises(ValueError, match="flag bit 1"):
        log.compute()
    log, oracle = _new(dev, 0, 10, 4)
    _append(log, oracle, dev, z, y, 1.0)
    _append(log, oracle, dev, z, y, 1.0)                                    # past max_graphs: 12 > 10
    _append(log, oracle, dev, z, y, 1.0, valid=[0, 0, 7, 0])               # a count beyond the batch's own rows
    _append(log, oracle, dev, z, y, 1.0, valid=[0, 0, -1, 0])
    assert oracle.state.tolist() == [6, 1, 2, 0]
    _assert_arrays(log, oracle, "past max_graphs")
    log.reset(); oracle.reset()
    _append(log, oracle, dev, z, y)                                         # no loss: the mean turns NaN
    assert np.isnan(log.compute()["loss"])


def test_nan_logits_and_labels_that_are_no_class_are_bad(dev):
    z = np.array([[1.0, 0.5, 0.0], [np.nan, 3.0, 0.0], [0.0, 0.0, 0.0], [2.0, 2.0, 2.5], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]], dtype=np.float32)
    y = np.array([[0], [1], [3], [2], [1.5], [np.nan]], dtype=np.float32)
    log, oracle = _new(dev, 1, 6, 1)
    _append(log, oracle, dev, z, y, 1.0)
    got = log.compute()
    _same(got, oracle.compute(), "mode 1")
    assert got["bad"] == 4 and got["confusion"].tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 1]] and abs(got["clf_acc"] - 2 / 6) <= 2.0 ** -53
    log, oracle = _new(dev, 0, 4, 1)
    _append(log, oracle, dev, np.array([[np.nan], [1.0], [-1.0], [0.0]], dtype=np.float32), np.array([[1], [1], [2], [0]], dtype=np.float32), 1.0)
    got = log.compute()
    assert got["bad"] == 2 and got["confusion"].tolist() == [[1, 0], [0, 1]]


def test_constructor_refusals(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import _lib
    for args in ((4, 1, 33), (4, 1, 257, 257, True), (4, 1, 3, 2), (4, 1, 3, 2, True), (-1, 1, 1), (4, 1, 0)):
        with pytest.raises(ValueError):
            G.ClfLog(*args, device=dev)
    lib = _lib.load()
    assert lib.gsat_clf_log_counts_words(1, 1, 0) == 5 and lib.gsat_clf_log_counts_words(32, 1, 1) == 1025
    assert lib.gsat_clf_log_counts_words(256, 256, 2) == 1280 and lib.gsat_clf_log_counts_words(33, 1, 1) == -1
    out = torch.zeros(8, dtype=torch.int64, device=dev)
    state = torch.zeros(4, dtype=torch.int64, device=dev)
    status = lib.gsat_clf_log_counts(None, None, state.data_ptr(), 0, 33, 1, 1, out.data_ptr(), None)
    assert status == _lib.load().gsat_clf_log_counts(None, None, state.data_ptr(), 0, 257, 257, 2, out.data_ptr(), None) != 0


def test_one_captured_append_accumulates_over_replays(dev):
    """One append captured in a torch.cuda.graph and replayed three times on changed inputs logs three batches."""
    z0, y0 = _rows(2, 6, 60)
    log, oracle = _new(dev, 2, 20, 4)
    z, y = torch.from_numpy(z0).to(dev), torch.from_numpy(y0).to(dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    valid = torch.tensor([0, 0, 6, 0], dtype=torch.int32, device=dev)
    data = NS(y=y, num_graphs=6, valid=valid)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        log.append(data, z, loss)
    torch.cuda.current_stream().wait_stream(side)
    log.reset()
    log.logits.view(torch.int32).fill_(SENT)
    log.y.view(torch.int32).fill_(SENT)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        log.append(data, z, loss)
    assert log.state.tolist() == [0, 0, 0, 0]                              # capturing ran nothing
    for i, count in enumerate((6, 2, 5)):
        zi, yi = _rows(2, 6, 61 + i)
        z.copy_(torch.from_numpy(zi)); y.copy_(torch.from_numpy(yi)); loss.fill_(0.5 * (i + 1)); valid[2] = count
        graph.replay()
        oracle.append(zi, yi, 0.5 * (i + 1), [0, 0, count, 0])
    _assert_arrays(log, oracle, "three replays")
    assert oracle.state.tolist() == [13, 3, 0, 0]
    _same(log.compute(), oracle.compute(), "three replays")
