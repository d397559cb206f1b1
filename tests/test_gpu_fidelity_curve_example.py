"""-m gpu: the training example with --graph --ragged --fidelity-curve 0.2,0.5,0.8 prints one line per sparsity level under each report
line, and without the flag prints what it printed before."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^epoch +(\d+)  train loss (-?[0-9.]+)  test acc ([0-9.]+)  attention ROC-AUC vs motif edges ([0-9.]+)  prec@5 ([0-9.]+)$")
LEVEL = re.compile(r"^      fidelity@([0-9.]+)  kept ([0-9.]+)  fidelity_plus (-?[0-9.]+)  fidelity_minus (-?[0-9.]+)  flip_plus ([0-9.]+)  "
                   r"flip_minus ([0-9.]+)$")


def _run(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ba2motifs.py"), "--graph", "--ragged", "--graphs", "200",
                          "--epochs", "2", "--batch-size", "32", "--hidden", "32", *extra], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return [l for l in out.stdout.splitlines() if l.strip()]


def test_example_prints_three_level_lines_per_report(dev):
    plain, scored = _run(), _run("--fidelity-curve", "0.2,0.5,0.8")
    assert len(plain) == 1 and LINE.match(plain[0]), plain                              # epoch 2, and nothing else: the output of before
    assert len(scored) == 4 and scored[0] == plain[0], (plain, scored)                  # the curve epoch changes neither training nor scores
    for report in (scored[1:4],):
        kept_before = 0.0
        for line, ratio in zip(report, (0.2, 0.5, 0.8)):
            m = LEVEL.match(line)
            assert m, line
            level, kept, plus, minus, flip_plus, flip_minus = (float(v) for v in m.groups())
            assert level == ratio and all(math.isfinite(v) for v in (kept, plus, minus, flip_plus, flip_minus))
            assert ratio <= kept + 5e-4 and kept_before <= kept <= 1.0                   # ceil(ratio * E_g) edges of every graph: nested levels
            assert -1.0 <= plus <= 1.0 and -1.0 <= minus <= 1.0 and 0.0 <= flip_plus <= 1.0 and 0.0 <= flip_minus <= 1.0
            kept_before = kept
