#!/usr/bin/env python3
"""Times what the scores of a training epoch cost, three ways, and writes profiles/train_log_report.json.

Per Mutagenicity epoch (one fixed shuffle, 128 graph slots, ReplayedStep(ragged=True) at the capacity near the mean batch -- the c_mean
configuration of tools/bench_ragged_replay.py), by that tool's method:
  a -- replayed training without a log: the epoch returns a loss and nothing else;
  b -- ReplayedStep(..., log_k=5): begin_epoch(), the same replays, epoch_scores() -- the training pass logs itself;
  c -- (a) and then ReplayedEval(ragged=True).run over the same ids: the way to train scores without the training-pass log (a second,
       eval-mode pass: other numbers, too).
The configurations alternate in one process: all are warmed, then ``--rounds`` rounds of one window each, every window whole epochs for at
least ``--window`` seconds and ending in a synchronise.  Reported per configuration: the median ms/epoch of the windows and their min /
max; and the two costs of the scores, (b) - (a) and (c) - (a), from the medians.  No threshold is set: the report is the claim.

Shapes: tools/bench_padded.py's Mutagenicity (the 4337 topologies of tests/golden/mutag_full.npz, GIN, H 64, edge attention), with
pseudo-random edge labels -- the log and the evaluator need some, and their cost does not depend on the values.

  python tools/bench_train_log.py [--out profiles/train_log_report.json] [--window 1.0] [--rounds 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from bench_padded import BATCH, HIDDEN, build, mutag_graphs
from bench_ragged_replay import summary, timed

K = 5


def labelled_mutag_graphs():
    graphs, x_dim = mutag_graphs()
    rng = np.random.RandomState(3)
    for g in graphs:
        g.edge_label = torch.from_numpy((rng.rand(g.edge_index.shape[1]) < 0.3).astype(np.float32))
    return graphs, x_dim


def measure(graphs, x_dim, dev, seconds, rounds):
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    perm = np.random.RandomState(1).permutation(len(graphs))
    capacity = (max(int(np.ceil(n_all.mean() * BATCH)), int(n_all.max())) + 2, max(int(np.ceil(e_all.mean() * BATCH)), int(e_all.max())))
    runs, steppers, scores = {}, [], {}

    def trainer(**kw):
        gsat = build(graphs, x_dim, dev, True)
        rs = G.ReplayedStep(gsat, ds, BATCH, capacity=capacity, ragged=True, **kw)
        steppers.append(rs)
        return gsat, rs, rs.batches(perm)

    _, rs_a, rows = trainer()

    def epoch_a():
        for row in rows:
            rs_a.step(row, 0)

    _, rs_b, rows_b = trainer(log_k=K)

    def epoch_b():
        rs_b.begin_epoch()
        for row in rows_b:
            rs_b.step(row, 0)
        scores["b"] = rs_b.epoch_scores()

    gsat_c, rs_c, rows_c = trainer()
    ev = G.ReplayedEval(gsat_c, ds, BATCH, K, capacity=capacity, ragged=True)

    def epoch_c():
        for row in rows_c:
            rs_c.step(row, 0)
        scores["c"] = ev.run(perm, 0)

    runs = dict(a=epoch_a, b=epoch_b, c=epoch_c)
    for _ in range(2):                                      # warm every configuration
        for epoch in runs.values():
            epoch()
    times = {key: [] for key in runs}
    for _ in range(rounds):
        for key, epoch in runs.items():
            times[key].append(timed(epoch, seconds))
    for rs in steppers:
        assert not rs.overflowed(), "a timed batch did not fit its capacity"
    assert all(np.isfinite(scores[key]["loss"]) and 0.0 <= scores[key]["clf_acc"] <= 1.0 for key in ("b", "c"))
    out = dict(shape="mutag", graphs=len(graphs), slots=BATCH, hidden=HIDDEN, k=K, capacity=dict(nodes=capacity[0], edges=capacity[1]),
               batches_per_epoch=int(rows.shape[0]),
               configurations={key: dict(ms_per_epoch=summary(times[key])) for key in runs})
    med = {key: out["configurations"][key]["ms_per_epoch"]["median"] for key in runs}
    out["log_cost_ms_per_epoch"] = med["b"] - med["a"]                       # the training pass logs itself
    out["second_pass_cost_ms_per_epoch"] = med["c"] - med["a"]               # an evaluation pass over the training ids
    out["log_cost_per_step_ms"] = out["log_cost_ms_per_epoch"] / out["batches_per_epoch"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_log_report.json"))
    ap.add_argument("--window", type=float, default=1.0, help="least length of a timed window, seconds")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    graphs, x_dim = labelled_mutag_graphs()
    res = measure(graphs, x_dim, dev, args.window, args.rounds)
    report = dict(device=torch.cuda.get_device_name(0), window_seconds=args.window, rounds=args.rounds, epochs=[res])
    for key, c in res["configurations"].items():
        t = c["ms_per_epoch"]
        print(f"mutag {key}: {res['batches_per_epoch']} batches  {t['median']:.2f} ms/epoch [{t['min']:.2f}, {t['max']:.2f}]", flush=True)
    print(f"mutag: the log costs {res['log_cost_ms_per_epoch']:.2f} ms/epoch, the second pass {res['second_pass_cost_ms_per_epoch']:.2f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
