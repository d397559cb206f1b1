"""-m gpu: the end-to-end training example with --graph --ragged --train-scores prints, under every report line, the scores of the training
epoch from the training-pass log -- with no eager batch -- and still learns."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--graph", "--ragged", "--graphs", "600", "--epochs", "25"]      # the epoch count of tests/test_gpu_ragged_example.py


def _run(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ba2motifs.py"), *ARGS, *extra], capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines()


def test_train_scores_are_printed_for_every_report(dev):
    """Every report line is followed by the scores of that training epoch.  Its ``loss`` is the mean the report line prints as ``train
    loss`` (the same fp32 losses, summed on the device there and in fp64 by the log; both printed to four decimals: within 2e-4), ``pred
    + info`` is ``loss`` (three roundings: 2e-4), the other scores lie in [0, 1], and the run still passes the assertions of
    tests/test_gpu_ragged_example.py on its last test scores."""
    lines = _run("--train-scores")
    reports = [l for l in lines if l.startswith("epoch")]
    train = [l for l in lines if l.lstrip().startswith("train ")]
    assert len(reports) == 5 and len(train) == len(reports)
    assert [lines.index(t) - lines.index(r) for r, t in zip(reports, train)] == [1] * 5
    for rep, line in zip(reports, train):
        vals = {k: float(v) for k, v in re.findall(r"(loss|pred|info|acc|clf ROC-AUC|attention ROC-AUC|prec@5) ([0-9.]+)", line)}
        assert set(vals) == {"loss", "pred", "info", "acc", "clf ROC-AUC", "attention ROC-AUC", "prec@5"}, line
        assert abs(vals["loss"] - float(re.search(r"train loss ([0-9.]+)", rep).group(1))) <= 2e-4, (rep, line)
        assert abs(vals["pred"] + vals["info"] - vals["loss"]) <= 2e-4, line
        assert all(0.0 <= vals[k] <= 1.0 for k in vals if k not in ("loss", "pred", "info")), line
    last = reports[-1]
    acc = float(re.search(r"test acc ([0-9.]+)", last).group(1))
    auc = float(re.search(r"ROC-AUC vs motif edges ([0-9.]+)", last).group(1))
    assert acc >= 0.9 and auc >= 0.8, last
