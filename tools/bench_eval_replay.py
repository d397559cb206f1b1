#!/usr/bin/env python3
"""Times one evaluation epoch two ways and writes profiles/eval_replay_report.json:

  eager    -- per batch PackedDataset.collate(ids), the eval-mode forward_pass under no_grad and EvaluationMeter.update; at the end
              EvaluationMeter.compute();
  replayed -- dp_gsat_amd.ReplayedEval.run: every full batch is a replay of ONE captured hipGraph (collate_padded to a fixed capacity,
              the eval-mode forward, EpochLog.append), the tail batch runs eagerly, and EpochLog.compute() scores the device log once.

Shapes (those of tools/bench_padded.py): the example's 1000 BA-2motifs graphs (GIN, H 64, edge attention, batch 128) and the 4337
Mutagenicity topologies of tests/golden/mutag_full.npz with random node labels, graph labels and edge labels, batch 128; the second also
with the tightest capacity that holds the epoch's batches.  An epoch visits every graph once, in a fixed random order.  For each shape
the two modes alternate in one process: both are warmed, then 5 rounds of one eager and one replayed window, each of whole epochs, at
least 1 s long and ending in a synchronise (compute() reads the results back anyway).  Reported per mode: the median ms/epoch of the 5
windows and their min / max.  No ratio is expected in advance.

  python tools/bench_eval_replay.py [--out profiles/eval_replay_report.json] [--window 1.0] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

BATCH, HIDDEN, K = 128, 64, 5


def example_graphs():
    from train_ba2motifs import make_graphs
    return make_graphs(1000, 0), 10


def mutag_graphs():
    import bench_padded
    graphs, x_dim = bench_padded.mutag_graphs()
    rng = np.random.RandomState(1)
    for g in graphs:
        g.edge_label = torch.from_numpy((rng.rand(g.edge_index.shape[1]) < 0.3).astype(np.float32))
    return graphs, x_dim


def window(epoch_fn, seconds):
    """ms/epoch of a window of whole epochs, at least ``seconds`` long, ending in a synchronise."""
    n = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while True:
        epoch_fn()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def measure(name, graphs, x_dim, dev, seconds, rounds, tight):
    import bench_padded
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = bench_padded.build(graphs, x_dim, dev, False)
    perm = np.random.RandomState(2).permutation(len(graphs))
    full = [perm[s:s + BATCH] for s in range(0, len(graphs) - BATCH + 1, BATCH)]
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    capacity = (max(int(n_all[u].sum()) for u in full) + 2, max(int(e_all[u].sum()) for u in full)) if tight else None
    replayed = G.ReplayedEval(gsat, ds, BATCH, K, capacity=capacity)
    meter = G.EvaluationMeter(K)
    batches = [torch.as_tensor(perm[s:s + BATCH], device=dev) for s in range(0, len(graphs), BATCH)]
    results = {}

    def eager_epoch():
        meter.reset()
        gsat.eval()
        with torch.no_grad():
            for ids in batches:
                b = ds.collate(ids)
                att, _, _, logits = gsat.forward_pass(b, 0, False)
                meter.update(att, b, logits)
        gsat.train()
        results["eager"] = meter.compute()

    def replayed_epoch():
        results["replayed"] = replayed.run(perm, 0)

    for _ in range(3):                                     # warm both modes
        eager_epoch()
        replayed_epoch()
    for key in ("att_auroc", "clf_acc"):                   # both modes scored the same epoch
        assert abs(results["eager"][key] - results["replayed"][key]) <= 5e-3, (key, results["eager"][key], results["replayed"][key])
    times = {"eager": [], "replayed": []}
    for _ in range(rounds):
        for mode, fn in (("eager", eager_epoch), ("replayed", replayed_epoch)):
            times[mode].append(window(fn, seconds))
    N_cap, E_cap = replayed.capacity
    out = dict(shape=name, graphs=len(graphs), batch=BATCH, hidden=HIDDEN, full_batches=len(full), tail_graphs=len(graphs) % BATCH,
               edges=int(e_all.sum()), capacity_rule="epoch maximum" if tight else "capacity_for", capacity=dict(nodes=N_cap, edges=E_cap))
    for mode, t in times.items():
        out[mode] = dict(ms_per_epoch_median=statistics.median(t), ms_per_epoch_min=min(t), ms_per_epoch_max=max(t), windows=t)
    out["replayed_over_eager"] = out["replayed"]["ms_per_epoch_median"] / out["eager"]["ms_per_epoch_median"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_replay_report.json"))
    ap.add_argument("--window", type=float, default=1.0, help="least length of a timed window, seconds")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    report = dict(device=torch.cuda.get_device_name(0), window_seconds=args.window, rounds=args.rounds, shapes=[])
    for name, make, tight in (("ba2motifs_example", example_graphs, False), ("mutag_batch128", mutag_graphs, False),
                              ("mutag_batch128_tight_capacity", mutag_graphs, True)):
        graphs, x_dim = make()
        res = measure(name, graphs, x_dim, dev, args.window, args.rounds, tight)
        report["shapes"].append(res)
        print(json.dumps({k: res[k] for k in ("shape", "capacity", "full_batches", "replayed_over_eager")}), flush=True)
        print(f"  eager {res['eager']['ms_per_epoch_median']:.3f} ms/epoch  replayed {res['replayed']['ms_per_epoch_median']:.3f} ms/epoch", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
