"""-m gpu: examples/train_multitask.py --graph --ragged runs on a small graph count, prints the per-task scores and the per-task curve, and
two runs with one seed print the same lines.  No accuracy is asserted."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM = r"(-?[0-9.]+|nan)"
TASKS = r"\[" + NUM + ", " + NUM + ", " + NUM + r"\]"
LINE = re.compile(r"^epoch +(\d+)  train loss " + NUM + "  clf_roc " + NUM + r"  \|  test loss " + NUM + "  clf_acc " + NUM + "  clf_roc " + NUM +
                  "  clf_roc_tasks " + TASKS + r"  att_auroc 0\.0 \(no edge labels\)$")
LEVEL = re.compile(r"^      fidelity@([0-9.]+)  kept ([0-9.]+)  fidelity_plus " + NUM + "  fidelity_minus " + NUM + "  fidelity_plus_tasks " + TASKS +
                   "  fidelity_minus_tasks " + TASKS + "$")


def _run():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_multitask.py"), "--graph", "--ragged", "--graphs", "120",
                          "--epochs", "2", "--batch-size", "32", "--hidden", "32", "--fidelity-curve", "0.3,0.7"], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return [l for l in out.stdout.splitlines() if l.strip()]


def test_example_prints_per_task_scores_and_repeats_itself(dev):
    first, second = _run(), _run()
    assert first == second, (first, second)
    assert len(first) == 4 and LINE.match(first[0]) and LINE.match(first[1]), first
    for line, ratio in zip(first[2:], (0.3, 0.7)):
        m = LEVEL.match(line)
        assert m and float(m.group(1)) == ratio and ratio <= float(m.group(2)) + 5e-4, line
