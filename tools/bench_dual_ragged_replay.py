#!/usr/bin/env python3
"""Times a dual/primal (DualGSAT) training EPOCH and an evaluation EPOCH over ragged batches four ways and writes
profiles/dual_ragged_replay_report.json.

Per epoch (one fixed shuffle of the dataset, batch / slot count 128), by the alternating-window method of tools/bench_dual_replay.py:
  a       -- ReplayedDualStep / ReplayedDualEval at PackedDataset.pair_capacity_for(dual, 128), the bound over every possible batch; the
             tail batch runs eagerly;
  b       -- the same at the tightest capacity that holds this shuffle's full batches (and graphs 0 .. 127, on which the fixed-count
             classes capture); the tail batch runs eagerly;
  c_tight -- ReplayedDualStep / ReplayedDualEval(ragged=True) over the three-budget batches (PackedDataset.budget_batches(..., dual=)) at
             capacity (b): every batch is a replay;
  c_mean  -- the same at a capacity near the mean batch (128 graphs of the mean size, at least the largest graph, in nodes, edges and
             dual edges).
(a) and (b) are the paths as they were before the pair took a ragged graph count: the baseline.  The configurations alternate in one
process: all are warmed, then ``--rounds`` rounds of one window each, every window whole epochs for at least ``--window`` seconds and
ending in a synchronise.  Reported per configuration and per kind of epoch: the median ms/epoch of the windows, their min / max, ms per
graph, and the batches per epoch.  An evaluation epoch is ``run(perm, 0)`` with its two host reads.

Shape: the topology of all 4337 Mutagenicity graphs (tests/golden/mutag_full.npz; labels drawn at random) and its dual dataset, GIN, H 64,
2 layers, node attention on both sides.  Epoch 0 throughout: the unmixed graphs.

  python tools/bench_dual_ragged_replay.py [--out profiles/dual_ragged_replay_report.json] [--window 1.0] [--rounds 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from bench_dual_replay import build
from bench_padded import BATCH, HIDDEN, mutag_graphs
from bench_ragged_replay import summary, timed

K = 5
KEYS = ("nodes", "edges", "dual_edges")


def measure(name, ds, dual, dev, seconds, rounds):
    import dp_gsat_amd as G
    counts = [c.cpu().numpy() for c in (ds.node_counts, ds.edge_counts, dual.edge_counts)]
    perm = np.random.RandomState(1).permutation(ds.num_graphs)
    full = [perm[s:s + BATCH] for s in range(0, len(perm) - BATCH + 1, BATCH)]
    tail = perm[len(full) * BATCH:]
    bound = ds.pair_capacity_for(dual, BATCH)
    pad = (2, 0, 0)
    # the fixed-count classes warm up and capture on graphs 0 .. 127, which (b) therefore has to hold next to the shuffle's batches
    tight = tuple(max(int(c[u].sum()) for u in full + [np.arange(BATCH)]) + p for c, p in zip(counts, pad))
    mean = tuple(max(int(np.ceil(c.mean() * BATCH)), int(c.max())) + p for c, p in zip(counts, pad))
    configs, runs = {}, {}

    def make(capacity, ragged):
        m = build(dev, True)
        rs = G.ReplayedDualStep(m, ds, dual, BATCH, capacity=capacity, ragged=ragged)
        ev = G.ReplayedDualEval(m, ds, dual, BATCH, K, capacity=capacity, ragged=ragged)
        if ragged:
            rows = rs.batches(perm)

            def train():
                for row in rows:
                    rs.step(row, 0)
            return rs, train, lambda: ev.run(perm, 0), int(rows.shape[0]), 0
        rs.check_epoch(perm)
        tail_ids = torch.as_tensor(tail, device=dev)

        def train():
            for ids in full:
                rs.step(ids, 0)
            if len(tail):                                   # the eager tail: both collates, the step, the one host read of the loss dict
                _, loss, ld, _ = m.dual_forward_pass(ds.collate(tail_ids), dual.collate(tail_ids), 0, True)
                m.primal_optimizer.zero_grad(set_to_none=True)
                m.dual_optimizer.zero_grad(set_to_none=True)
                loss.backward()
                m.primal_optimizer.step()
                m.dual_optimizer.step()
        return rs, train, lambda: ev.run(perm, 0), len(full) + (1 if len(tail) else 0), 1 if len(tail) else 0

    for key, capacity, ragged in (("a", bound, False), ("b", tight, False), ("c_tight", tight, True), ("c_mean", mean, True)):
        rs, train, evaluate, batches, eager_batches = make(capacity, ragged)
        runs[key] = (rs, train, evaluate)
        configs[key] = dict(capacity=dict(zip(KEYS, capacity)), ragged=ragged, batches_per_epoch=batches,
                            eager_batches_per_epoch=eager_batches)
    for _ in range(2):                                      # warm every configuration
        for rs, train, evaluate in runs.values():
            train()
            evaluate()
    times = {key: dict(train=[], eval=[]) for key in runs}
    for _ in range(rounds):
        for key, (rs, train, evaluate) in runs.items():
            times[key]["train"].append(timed(train, seconds))
            times[key]["eval"].append(timed(evaluate, seconds))
    for key, (rs, _, _) in runs.items():
        assert not rs.overflowed(), f"{name} {key}: a timed batch did not fit its capacity"
        for kind in ("train", "eval"):
            configs[key][f"{kind}_ms_per_epoch"] = summary(times[key][kind])
            configs[key][f"{kind}_ms_per_graph"] = configs[key][f"{kind}_ms_per_epoch"]["median"] / ds.num_graphs
    G.clear_cache()
    med = lambda key, kind: configs[key][f"{kind}_ms_per_epoch"]["median"]
    return dict(shape=name, graphs=ds.num_graphs, slots=BATCH, hidden=HIDDEN,
                mean_batch={k: float(c.mean() * BATCH) for k, c in zip(KEYS, counts)}, configurations=configs,
                train_c_mean_over_b=med("c_mean", "train") / med("b", "train"), train_c_mean_over_a=med("c_mean", "train") / med("a", "train"),
                eval_c_mean_over_b=med("c_mean", "eval") / med("b", "eval"), eval_c_mean_over_a=med("c_mean", "eval") / med("a", "eval"))


def main():
    import dp_gsat_amd as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_ragged_replay_report.json"))
    ap.add_argument("--window", type=float, default=1.0, help="least length of a timed window, seconds")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    graphs, _ = mutag_graphs()
    gen = torch.Generator().manual_seed(0)
    for g in graphs:
        g.edge_label = (torch.rand(g.edge_index.shape[1], generator=gen) > 0.67).float()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    dual = ds.line_graph_dataset()
    G.clear_cache()
    props = torch.cuda.get_device_properties(0)
    report = dict(device=torch.cuda.get_device_name(0), arch=props.gcnArchName, compute_units=props.multi_processor_count,
                  window_seconds=args.window, rounds=args.rounds, dual_edges_total=int(dual.edge_local_all.shape[1]), epochs=[])
    res = measure("mutag_dual_slots128", ds, dual, dev, args.window, args.rounds)
    report["epochs"].append(res)
    for key, c in res["configurations"].items():
        t, e = c["train_ms_per_epoch"], c["eval_ms_per_epoch"]
        print(f"{key}: capacity {c['capacity']}  {c['batches_per_epoch']} batches  train {t['median']:.2f} ms/epoch [{t['min']:.2f}, "
              f"{t['max']:.2f}]  eval {e['median']:.2f} ms/epoch [{e['min']:.2f}, {e['max']:.2f}]", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
