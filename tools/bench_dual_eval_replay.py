#!/usr/bin/env python3
"""Times one dual/primal (DualGSAT) evaluation epoch two ways and writes profiles/dual_eval_replay_report.json:

  eager    -- per batch two PackedDataset.collate calls (primal and dual dataset), the eval-mode dual_forward_pass under no_grad (the dual
              Gumbel noise from torch's generator, the one host read of the loss dict) and EvaluationMeter.update; at the end
              EvaluationMeter.compute();
  replayed -- dp_gsat_amd.ReplayedDualEval.run: every full batch is a replay of ONE captured hipGraph (collate_padded_pair to a fixed
              capacity, one seed word, the eval-mode forward with the noise drawn inside the sampler kernel, EpochLog.append), the tail
              batch runs eagerly, and EpochLog.compute() scores the device log once.

Shape (that of tools/bench_dual_replay.py): the topology of all 4337 Mutagenicity graphs (tests/golden/mutag_full.npz; node labels, graph
labels and edge labels are drawn at random) and its dual dataset, batches of 128 graphs, GIN, H 64, 2 layers, node attention on both sides.
An epoch visits every graph once, in a fixed random order: 33 full batches and a tail of 113.  The two modes alternate in one process:
both are warmed, then 5 rounds of one eager and one replayed window, each of whole epochs, at least 1 s long and ending in a synchronise.
Reported per mode: the median ms/epoch of the 5 windows and their min / max.  Timed at the bound capacity
(PackedDataset.pair_capacity_for(dual, 128)) and again at the tightest capacity that holds the epoch's batches and the evaluator's warm-up batch, graphs 0..127 (vetted with
check_epoch).
Epoch 0 throughout: the unmixed graph.  The eager figure is host-bound and moves with the load of the host.  No ratio is expected in
advance.

  python tools/bench_dual_eval_replay.py [--out profiles/dual_eval_replay_report.json] [--window 1.0] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from bench_dual_replay import build
from bench_eval_replay import BATCH, HIDDEN, K, window
from bench_padded import mutag_graphs


def measure(name, ds, dual, dev, seconds, rounds, tight):
    import dp_gsat_amd as G
    model = build(dev, False)
    n_graphs = ds.num_graphs
    perm = np.random.RandomState(2).permutation(n_graphs)
    full = [perm[s:s + BATCH] for s in range(0, n_graphs - BATCH + 1, BATCH)]
    counts = [c.cpu().numpy() for c in (ds.node_counts, ds.edge_counts, dual.edge_counts)]
    capacity = None
    if tight:
        warm = [np.arange(BATCH)]                          # the evaluator's warm-up runs collate graphs 0 .. BATCH-1
        n, e, ed = (max(int(c[u].sum()) for u in full + warm) for c in counts)
        capacity = (n + 2, e, ed)
    replayed = G.ReplayedDualEval(model, ds, dual, BATCH, K, capacity=capacity)
    replayed.check_epoch(perm)
    meter = G.EvaluationMeter(K)
    batches = [torch.as_tensor(perm[s:s + BATCH], device=dev) for s in range(0, n_graphs, BATCH)]
    results = {}

    def eager_epoch():
        meter.reset()
        model.eval()
        with torch.no_grad():
            for ids in batches:
                pb, db = ds.collate(ids), dual.collate(ids)
                att, _, _, logits = model.dual_forward_pass(pb, db, 0, False)
                meter.update(att, pb, logits)
        model.train()
        results["eager"] = meter.compute()

    def replayed_epoch():
        results["replayed"] = replayed.run(perm, 0)

    for _ in range(3):                                     # warm both modes
        eager_epoch()
        replayed_epoch()
    # the two modes draw different (identically distributed) Gumbel noise: the scores agree loosely, not bit for bit
    for key in ("att_auroc", "clf_acc"):
        assert abs(results["eager"][key] - results["replayed"][key]) <= 5e-2, (key, results["eager"][key], results["replayed"][key])
    times = {"eager": [], "replayed": []}
    for _ in range(rounds):
        for mode, fn in (("eager", eager_epoch), ("replayed", replayed_epoch)):
            times[mode].append(window(fn, seconds))
    keys = ("nodes", "edges", "dual_edges")
    mean = [float(np.mean([c[u].sum() for u in full])) for c in counts]
    out = dict(shape=name, graphs=n_graphs, batch=BATCH, hidden=HIDDEN, full_batches=len(full), tail_graphs=n_graphs % BATCH,
               capacity_rule="epoch and warm-up maximum" if tight else "pair_capacity_for", capacity=dict(zip(keys, replayed.capacity)),
               mean_real=dict(zip(keys, mean)), padding_share={k: (c - m) / c for k, c, m in zip(keys, replayed.capacity, mean)})
    for mode, t in times.items():
        out[mode] = dict(ms_per_epoch_median=statistics.median(t), ms_per_epoch_min=min(t), ms_per_epoch_max=max(t), windows=t)
    out["replayed_over_eager"] = out["replayed"]["ms_per_epoch_median"] / out["eager"]["ms_per_epoch_median"]
    G.clear_cache()
    return out


def main():
    import dp_gsat_amd as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_eval_replay_report.json"))
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
    report = dict(device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                  compute_units=torch.cuda.get_device_properties(0).multi_processor_count, window_seconds=args.window, rounds=args.rounds,
                  dual_edges_total=int(dual.edge_local_all.shape[1]), shapes=[])
    for name, tight in (("mutag_dual_eval_batch128", False), ("mutag_dual_eval_batch128_tight_capacity", True)):
        res = measure(name, ds, dual, dev, args.window, args.rounds, tight)
        report["shapes"].append(res)
        print(json.dumps({k: res[k] for k in ("shape", "capacity", "full_batches", "replayed_over_eager")}), flush=True)
        print(f"  eager {res['eager']['ms_per_epoch_median']:.3f} ms/epoch  replayed {res['replayed']['ms_per_epoch_median']:.3f} ms/epoch", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
