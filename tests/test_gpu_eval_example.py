"""-m gpu: the training example with --graph evaluates through ReplayedEval (a full batch replayed, a tail run eagerly) and prints its
epoch lines in the format the other example tests read."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^epoch +(\d+)  train loss (-?[0-9.]+)  test acc ([0-9.]+)  attention ROC-AUC vs motif edges ([0-9.]+)  prec@5 ([0-9.]+)$")


def test_train_ba2motifs_example_evaluates_by_replay(dev):
    # 200 graphs: 160 for training (5 replayed steps per epoch), 40 for the test evaluation = one replayed batch of 32 and a tail of 8
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ba2motifs.py"), "--graph", "--graphs", "200", "--epochs", "6",
                          "--batch-size", "32", "--hidden", "32"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("epoch")]
    assert len(lines) == 2, out.stdout                                       # epochs 5 and 6
    for line, epoch in zip(lines, (5, 6)):
        m = LINE.match(line)
        assert m, line
        assert int(m.group(1)) == epoch
        acc, auc, prec = (float(m.group(i)) for i in (3, 4, 5))
        assert 0.0 <= acc <= 1.0 and 0.0 < auc <= 1.0 and 0.0 <= prec <= 1.0, line
        assert round(acc * 40) == pytest.approx(acc * 40, abs=0.021)         # an accuracy over the 40 test graphs
