#!/usr/bin/env python3
"""Times a multi-task training epoch and a multi-task evaluation epoch, eager against replayed, and writes
profiles/multitask_replay_report.json.

Workload: the 4337 Mutagenicity topologies of tests/golden/mutag_full.npz with 12 pseudo-random label columns of which about 20 % of the
entries are NaN (the shape of ogbg-moltox21) and a zero-filled ``edge_label``; GIN, H 64, edge attention, a 12-column multi-label head and
``Criterion(12, True, capturable=True)``; 128 graph slots at a capacity near the mean batch (tools/bench_ragged_replay.py's ``c_mean``).

  train_eager     -- per batch of 128 in a fixed shuffle: ``collate``, ``forward_pass`` (the capturable criterion), zero_grad, backward, Adam;
  train_replayed  -- ``ReplayedStep(ragged=True, log_k=5)`` over ``batches(perm)`` and ``epoch_scores()``: every batch a replay, the epoch scored;
  eval_eager      -- per batch: ``collate``, the eval-mode ``forward_pass``, ``EvaluationMeter(multi_label=True).update``; ``compute()`` at the end;
  eval_replayed   -- ``ReplayedEval(ragged=True).run``.

The method is tools/bench_ragged_replay.py's: everything is warmed, then ``--rounds`` rounds in which the configurations alternate, one
window each -- whole epochs for at least ``--window`` seconds, ending in a synchronise -- in ONE process.  Reported: median, min and max
of the windows' ms/epoch.

  python tools/bench_multitask_replay.py [--out profiles/multitask_replay_report.json] [--window 1.0] [--rounds 5]
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

from bench_padded import BATCH, HIDDEN, mutag_graphs
from bench_ragged_replay import summary, timed

TASKS = 12


def multitask_graphs():
    graphs, x_dim = mutag_graphs()
    rng = np.random.RandomState(3)
    for g in graphs:
        y = (rng.rand(TASKS) < 0.5).astype(np.float32)
        y[rng.rand(TASKS) < 0.2] = np.nan
        g.y = torch.from_numpy(y).view(1, TASKS)
        g.edge_label = torch.zeros(g.edge_index.shape[1])           # an OGB-style set has no ground-truth explanation
    return graphs, x_dim


def build(graphs, x_dim, dev):
    import dp_gsat_amd as G
    torch.manual_seed(0)
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=HIDDEN, dropout_p=0.3, use_edge_attr=False, deg=deg)
    clf = G.get_model(x_dim, 0, TASKS, True, cfg, dev)
    ext = G.ExtractorMLP(HIDDEN, True).to(dev)
    opt = torch.optim.Adam(list(clf.parameters()) + list(ext.parameters()), lr=1e-3, weight_decay=3e-6, capturable=True, fused=True)
    return G.GSAT(clf, ext, G.Criterion(TASKS, True, capturable=True), opt, learn_edge_att=True).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multitask_replay_report.json"))
    ap.add_argument("--window", type=float, default=1.0, help="least length of a timed window, seconds")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import dp_gsat_amd as G
    dev = torch.device("cuda:0")
    graphs, x_dim = multitask_graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    capacity = (max(int(np.ceil(n_all.mean() * BATCH)), int(n_all.max())) + 2, max(int(np.ceil(e_all.mean() * BATCH)), int(e_all.max())))
    perm = np.random.RandomState(1).permutation(len(graphs))
    chunks = [torch.as_tensor(perm[s:s + BATCH], device=dev) for s in range(0, len(perm), BATCH)]
    eager, replayed = build(graphs, x_dim, dev), build(graphs, x_dim, dev)
    step = G.ReplayedStep(replayed, ds, BATCH, capacity=capacity, ragged=True, log_k=5)
    evaluator = G.ReplayedEval(replayed, ds, BATCH, 5, capacity=capacity, ragged=True)
    rows = step.batches(perm)

    def train_eager():
        for ids in chunks:
            _, loss, _, _ = eager.forward_pass(ds.collate(ids), 0, True)
            eager.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            eager.optimizer.step()

    def train_replayed():
        step.begin_epoch()
        for row in rows:
            step.step(row, 0)
        step.epoch_scores()

    def eval_eager():
        meter = G.EvaluationMeter(5, multi_label=True)
        eager.eval()
        with torch.no_grad():
            for ids in chunks:
                b = ds.collate(ids)
                att, _, _, logits = eager.forward_pass(b, 0, False)
                meter.update(att, b, logits)
        eager.train()
        meter.compute()

    def eval_replayed():
        evaluator.run(perm, 0)

    runs = dict(train_eager=train_eager, train_replayed=train_replayed, eval_eager=eval_eager, eval_replayed=eval_replayed)
    for _ in range(2):
        for fn in runs.values():
            fn()
    times = {key: [] for key in runs}
    for _ in range(args.rounds):
        for key, fn in runs.items():
            times[key].append(timed(fn, args.window))
    assert not step.overflowed()
    report = dict(device=torch.cuda.get_device_name(0), window_seconds=args.window, rounds=args.rounds, shape="mutag", graphs=len(graphs),
                  tasks=TASKS, slots=BATCH, hidden=HIDDEN, capacity=dict(nodes=capacity[0], edges=capacity[1]),
                  batches_per_epoch=dict(eager=len(chunks), replayed=int(rows.shape[0])),
                  ms_per_epoch={key: summary(t) for key, t in times.items()})
    for kind in ("train", "eval"):
        report[f"{kind}_replayed_over_eager"] = (report["ms_per_epoch"][f"{kind}_replayed"]["median"] /
                                                 report["ms_per_epoch"][f"{kind}_eager"]["median"])
    for key, t in report["ms_per_epoch"].items():
        print(f"{key}: {t['median']:.2f} ms/epoch [{t['min']:.2f}, {t['max']:.2f}]", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    G.clear_cache()


if __name__ == "__main__":
    main()
