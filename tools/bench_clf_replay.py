#!/usr/bin/env python3
"""Times an ERM (classifier-only) training EPOCH two ways on the same ragged budget batches and writes profiles/clf_replay_report.json.

  eager    -- per batch: PackedDataset.collate, forward, torch criterion, zero_grad, backward, fused Adam, and the epoch's accuracy from
              integer hit counts kept on the device (no EvaluationMeter, one host read at the end of the epoch): what a user wrote
              before the classifier classes existed;
  replayed -- ReplayedClfStep(ragged=True, log=True): every batch one replay, the epoch scored by epoch_scores() (two host reads).
Both visit the rows of PackedDataset.budget_batches for one fixed shuffle, at a capacity near the mean batch (128 graphs of the mean
size).  Method of tools/bench_padded.py: both are warmed, then ``--rounds`` rounds of one window each, alternating in one process, every
window whole epochs for at least ``--window`` seconds and ending in a synchronise.  Reported: the median ms/epoch of the windows, their
min / max and the ratio of the medians.

Shapes: tools/bench_padded.py's (800 BA-2motifs graphs; the 4337 Mutagenicity topologies of tests/golden/mutag_full.npz), GIN, H 64.

  python tools/bench_clf_replay.py [--out profiles/clf_replay_report.json] [--window 1.0] [--rounds 5]
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

from bench_padded import BATCH, HIDDEN, example_graphs, mutag_graphs
from bench_ragged_replay import summary, timed


def build_clf(graphs, x_dim, dev):
    import dp_gsat_amd as G
    torch.manual_seed(0)
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=HIDDEN, dropout_p=0.3, use_edge_attr=False, deg=deg)
    clf = G.get_model(x_dim, 0, 2, False, cfg, dev).train()
    opt = torch.optim.Adam(clf.parameters(), lr=1e-3, weight_decay=3e-6, capturable=True, fused=True)
    return clf, G.Criterion(2, False), opt


def measure(name, graphs, x_dim, dev, seconds, rounds):
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    perm = np.random.RandomState(1).permutation(len(graphs))
    capacity = (max(int(np.ceil(n_all.mean() * BATCH)), int(n_all.max())) + 2, max(int(np.ceil(e_all.mean() * BATCH)), int(e_all.max())))
    model, crit, opt = build_clf(graphs, x_dim, dev)
    rs = G.ReplayedClfStep(model, crit, opt, ds, BATCH, capacity=capacity, ragged=True, log=True)
    rows = rs.batches(perm)
    lists = [row[row >= 0] for row in rows]                    # the eager epoch's ids, on the device already

    def replayed():
        rs.begin_epoch()
        for row in rows:
            rs.step(row)
        return rs.epoch_scores()["clf_acc"]

    emodel, ecrit, eopt = build_clf(graphs, x_dim, dev)
    hits = torch.zeros((), dtype=torch.int64, device=dev)

    def eager():
        hits.zero_()
        for ids in lists:
            b = ds.collate(ids)
            logits = emodel(b.x, b.edge_index, b.batch, edge_attr=b.edge_attr)
            loss = ecrit(logits, b.y)
            eopt.zero_grad(set_to_none=True)
            loss.backward()
            eopt.step()
            hits.add_(((logits.detach() > 0).float() == b.y).sum())
        return int(hits) / len(graphs)

    runs = {"eager": eager, "replayed": replayed}
    for _ in range(2):                                      # warm both
        for fn in runs.values():
            fn()
    times = {key: [] for key in runs}
    for _ in range(rounds):
        for key, fn in runs.items():
            times[key].append(timed(fn, seconds))
    assert not rs.overflowed(), f"{name}: a timed batch did not fit its capacity"
    out = dict(shape=name, graphs=len(graphs), slots=BATCH, hidden=HIDDEN, capacity=dict(nodes=capacity[0], edges=capacity[1]),
               batches_per_epoch=int(rows.shape[0]), ms_per_epoch={key: summary(t) for key, t in times.items()})
    out["eager_over_replayed"] = out["ms_per_epoch"]["eager"]["median"] / out["ms_per_epoch"]["replayed"]["median"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clf_replay_report.json"))
    ap.add_argument("--window", type=float, default=1.0, help="least length of a timed window, seconds")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    report = dict(device=torch.cuda.get_device_name(0), window_seconds=args.window, rounds=args.rounds, epochs=[])
    for name, make in (("ba2motifs_example", example_graphs), ("mutag", mutag_graphs)):
        graphs, x_dim = make()
        res = measure(name, graphs, x_dim, dev, args.window, args.rounds)
        report["epochs"].append(res)
        e, r = res["ms_per_epoch"]["eager"], res["ms_per_epoch"]["replayed"]
        print(f"{name}: {res['batches_per_epoch']} batches  eager {e['median']:.2f} ms/epoch [{e['min']:.2f}, {e['max']:.2f}]  "
              f"replayed {r['median']:.2f} [{r['min']:.2f}, {r['max']:.2f}]  eager / replayed {res['eager_over_replayed']:.2f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
