"""-m gpu: the training example with --graph --ragged --fidelity 5 prints the fidelity of the test split under each report line, and
without the flag prints what it printed before."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^epoch +(\d+)  train loss (-?[0-9.]+)  test acc ([0-9.]+)  attention ROC-AUC vs motif edges ([0-9.]+)  prec@5 ([0-9.]+)$")
FIDELITY = re.compile(r"^      fidelity@5  fidelity_plus (-?[0-9.]+)  fidelity_minus (-?[0-9.]+)  flip_plus ([0-9.]+)  flip_minus ([0-9.]+)$")


def _run(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ba2motifs.py"), "--graph", "--ragged", "--graphs", "120",
                          "--epochs", "5", "--batch-size", "32", "--hidden", "32", *extra], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return [l for l in out.stdout.splitlines() if l.strip()]


def test_example_prints_the_fidelity_of_the_test_split(dev):
    plain, scored = _run(), _run("--fidelity", "5")
    assert len(plain) == 1 and LINE.match(plain[0]), plain                              # epoch 5, and nothing else: the output of before
    assert len(scored) == 2 and scored[0] == plain[0], (plain, scored)                  # the fidelity epoch changes neither training nor scores
    m = FIDELITY.match(scored[1])
    assert m, scored[1]
    plus, minus, flip_plus, flip_minus = (float(v) for v in m.groups())
    assert all(math.isfinite(v) for v in (plus, minus, flip_plus, flip_minus))
    assert -1.0 <= plus <= 1.0 and -1.0 <= minus <= 1.0 and 0.0 <= flip_plus <= 1.0 and 0.0 <= flip_minus <= 1.0
    assert round(flip_plus * 24) == pytest.approx(flip_plus * 24, abs=0.013)            # a rate over the 24 test graphs
