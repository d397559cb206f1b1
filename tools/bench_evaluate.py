#!/usr/bin/env python3
"""Times the evaluation scores of dp_gsat_amd.evaluate against what a user can write with torch alone, and writes
profiles/evaluate_report.json:

  histogram   attention_histogram(att, labels, bins=64) at the C3 (molhiv, 2048 graphs) edge count, attention = sigmoid of a normal
              draw (piled up, as after the extractor), against torch.histc run twice, once per class (att[labels == c]: one host
              read each inside the boolean index)
  rocauc      classifier_rocauc(logits, labels) at R = 41127, T = 1 (molhiv) and R = 7831, T = 12 with ~20 % NaN labels (tox21),
              against a device-side torch restatement: per task a boolean index of the labelled rows, sort, unique_consecutive
              and cumsum

Every timed step is a child process of its own under a time limit; the first failure ends the run and nothing further starts.  Median
of 20 event-timed runs after 5 warm-up runs.  Each child first checks that the two sides agree.  The baselines live here, not in the
package: the package has no torch fallback.

  python tools/bench_evaluate.py [--out profiles/evaluate_report.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS = 64
STEP_TIMEOUT = 240
ROC_SHAPES = {"molhiv": (41127, 1), "tox21": (7831, 12)}
STEPS = ["histogram"] + [f"rocauc_{name}" for name in ROC_SHAPES]


def median_ms(fn, runs=20, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def torch_histc_twice(att, lab):
    import torch
    return torch.stack([torch.histc(att[lab == 0], bins=BINS, min=0.0, max=1.0), torch.histc(att[lab != 0], bins=BINS, min=0.0, max=1.0)])


def torch_rocauc(logits, labels):
    """The ogb rule with exact tie handling, one task at a time, on the device."""
    import torch
    per = []
    for t in range(logits.shape[1]):
        y = labels[:, t]
        have = ~y.isnan()
        s, pos = logits[have, t], y[have] != 0
        order = torch.sort(s).indices
        s, pos = s[order], pos[order]
        cneg = torch.cat([torch.zeros(1, dtype=torch.int64, device=s.device), torch.cumsum((~pos).to(torch.int64), 0)])
        _, group, size = torch.unique_consecutive(s, return_inverse=True, return_counts=True)
        end = torch.cumsum(size, 0)
        u2 = ((cneg[end - size][group] + cneg[end][group]) * pos).sum()
        per.append(torch.stack([u2, pos.sum(), (~pos).sum()]))
    c = torch.stack(per)
    den = 2 * c[:, 1] * c[:, 2]
    ok = den > 0
    return (torch.where(ok, c[:, 0].double() / den.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=c.device)).sum()
            / ok.sum().double())


def run_step(step):
    import numpy as np
    import torch
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)
    row = {"device": torch.cuda.get_device_name(0)}
    if step == "histogram":
        E = synth.molhiv_batch(2048, seed=0).num_edges
        att = torch.sigmoid(torch.from_numpy(rng.randn(E).astype(np.float32) * 3.0)).to(dev)
        lab = torch.from_numpy((rng.rand(E) < 0.25).astype(np.uint8)).to(dev)
        mine, base = G.attention_histogram(att, lab, bins=BINS), torch_histc_twice(att, lab)
        assert int(mine.counts.sum()) == E and int(base.sum().item()) == E
        out = G.attention_histogram(att, lab, bins=BINS)
        row.update(edges=E, bins=BINS, bins_equal_histc=bool(torch.equal(mine.counts, base.to(torch.int64))),
                   attention_histogram=median_ms(lambda: G.attention_histogram(att, lab, bins=BINS)),
                   attention_histogram_into_out=median_ms(lambda: G.attention_histogram(att, lab, out=out)),
                   torch_histc_twice=median_ms(lambda: torch_histc_twice(att, lab)))
        row["hip_faster_than_torch"] = row["attention_histogram"] < row["torch_histc_twice"]
    else:
        R, T = ROC_SHAPES[step[len("rocauc_"):]]
        logits = torch.from_numpy(rng.randn(R, T).astype(np.float32)).to(dev)
        y = (rng.rand(R, T) < 0.1).astype(np.float32)
        if T > 1:
            y[rng.rand(R, T) < 0.2] = np.nan
        labels = torch.from_numpy(y).to(dev)
        mine, base = G.classifier_rocauc(logits, labels).item(), torch_rocauc(logits, labels).item()
        assert abs(mine - base) <= 1e-12, (mine, base)
        row.update(rows=R, tasks=T, rocauc=mine, classifier_rocauc=median_ms(lambda: G.classifier_rocauc(logits, labels)),
                   torch_sort_cumsum=median_ms(lambda: torch_rocauc(logits, labels)))
        row["hip_faster_than_torch"] = row["classifier_rocauc"] < row["torch_sort_cumsum"]
    print("RESULT " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=STEPS, help="(child mode) run one timed step and print its result line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_report.json"))
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return 0
    report = {"runs": 20, "warmup": 5, "unit": "ms (median)", "steps": {}}
    for step in STEPS:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {STEP_TIMEOUT} s; stopping, no report written", flush=True)
            return 1
        lines = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
        if res.returncode != 0 or not lines:
            print(f"{step}: failed with exit status {res.returncode}; stopping, no report written\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}", flush=True)
            return 1
        row = json.loads(lines[-1][len("RESULT "):])
        report["device"] = row.pop("device")
        report["steps"][step] = row
        print(step, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
