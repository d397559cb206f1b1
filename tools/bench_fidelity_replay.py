#!/usr/bin/env python3
"""Times one explanation-fidelity epoch two ways and writes profiles/fidelity_replay_report.json:

  eager    -- per batch PackedDataset.collate(ids), the eval-mode forward_pass under no_grad and dp_gsat_amd.explanation_fidelity (two
              extractions that read their sizes back, three backbone forwards); the per-batch means are read back at the end;
  replayed -- dp_gsat_amd.ReplayedFidelity.run on ragged budget batches: every batch is a replay of ONE captured hipGraph (collate_padded,
              the eval-mode attention, the fused top-k, two padded extractions, three backbone forwards, FidelityLog.append), and
              FidelityLog.compute() reads the device log once.

Workloads: the example's 1000 BA-2motifs graphs and the 4337 Mutagenicity topologies of tests/golden/mutag_full.npz with random node
labels, each with GIN (edge attention) and PNA (node attention), H 64, top-5 explanations, at most 128 graphs per batch and a capacity
near the mean batch (the mean graph times 128).  An epoch visits every graph once, in a fixed random order.  For each workload the two
modes alternate in one process: both are warmed, then 5 rounds of one eager and one replayed window, each of whole epochs, at least 1 s
long and ending in a synchronise.  Reported per mode: the median ms/epoch of the 5 windows and their min / max.  No ratio is expected in
advance.

  python tools/bench_fidelity_replay.py [--out profiles/fidelity_replay_report.json] [--window 1.0] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from bench_eval_replay import example_graphs, window

BATCH, HIDDEN, K = 128, 64, 5


def mutag_graphs():
    import bench_padded
    return bench_padded.mutag_graphs()


def build(graphs, x_dim, dev, backbone):
    import dp_gsat_amd as G
    torch.manual_seed(0)
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=HIDDEN, dropout_p=0.3, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=deg)
    edge = backbone == "GIN"
    clf = G.get_model(x_dim, 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(HIDDEN, edge).to(dev)
    return G.GSAT(clf, ext, G.Criterion(2, False), None, learn_edge_att=edge).train()


def measure(name, graphs, x_dim, backbone, dev, seconds, rounds):
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = build(graphs, x_dim, dev, backbone)
    perm = np.random.RandomState(2).permutation(len(graphs))
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    capacity = (max(int(np.ceil(n_all.mean() * BATCH)), int(n_all.max())) + 2, max(int(np.ceil(e_all.mean() * BATCH)), int(e_all.max())))
    replayed = G.ReplayedFidelity(gsat, ds, BATCH, k=K, capacity=capacity, ragged=True)
    rows = replayed.batches(perm)
    batches = [row[row >= 0] for row in rows]                # the eager epoch takes the same batches
    results = {}

    def eager_epoch():
        plus, minus, count = [], [], []
        gsat.eval()
        with torch.no_grad():
            for ids in batches:
                b = ds.collate(ids)
                att = gsat.forward_pass(b, 0, False)[0]
                res = G.explanation_fidelity(gsat.clf, b, att, k=K)
                plus.append(res["fidelity_plus"]); minus.append(res["fidelity_minus"]); count.append(int(ids.numel()))
        gsat.train()
        w = torch.tensor(count, dtype=torch.float64, device=dev)
        both = torch.stack([(torch.stack(plus).double() * w).sum(), (torch.stack(minus).double() * w).sum()]) / w.sum()
        results["eager"] = dict(zip(("fidelity_plus", "fidelity_minus"), both.tolist()))      # the one read of the epoch's result

    def replayed_epoch():
        results["replayed"] = replayed.run(perm)

    for _ in range(3):                                        # warm both modes
        eager_epoch()
        replayed_epoch()
    for key in ("fidelity_plus", "fidelity_minus"):           # both modes scored the same epoch
        assert abs(results["eager"][key] - results["replayed"][key]) <= 5e-3, (key, results["eager"][key], results["replayed"][key])
    times = {"eager": [], "replayed": []}
    for _ in range(rounds):
        for mode, fn in (("eager", eager_epoch), ("replayed", replayed_epoch)):
            times[mode].append(window(fn, seconds))
    out = dict(shape=name, backbone=backbone, graphs=len(graphs), max_batch=BATCH, hidden=HIDDEN, k=K, batches=len(batches),
               edges=int(e_all.sum()), capacity=dict(nodes=capacity[0], edges=capacity[1], keep_edges=replayed.keep_capacity[1]),
               fidelity_plus=results["replayed"]["fidelity_plus"], fidelity_minus=results["replayed"]["fidelity_minus"])
    for mode, t in times.items():
        out[mode] = dict(ms_per_epoch_median=statistics.median(t), ms_per_epoch_min=min(t), ms_per_epoch_max=max(t), windows=t)
    out["replayed_over_eager"] = out["replayed"]["ms_per_epoch_median"] / out["eager"]["ms_per_epoch_median"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fidelity_replay_report.json"))
    ap.add_argument("--window", type=float, default=1.0, help="least length of a timed window, seconds")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    report = dict(device=torch.cuda.get_device_name(0), window_seconds=args.window, rounds=args.rounds, shapes=[])
    for name, make in (("ba2motifs_example", example_graphs), ("mutag", mutag_graphs)):
        graphs, x_dim = make()
        for backbone in ("GIN", "PNA"):
            res = measure(name, graphs, x_dim, backbone, dev, args.window, args.rounds)
            report["shapes"].append(res)
            print(json.dumps({k: res[k] for k in ("shape", "backbone", "capacity", "batches", "replayed_over_eager")}), flush=True)
            print(f"  eager {res['eager']['ms_per_epoch_median']:.3f} ms/epoch  replayed {res['replayed']['ms_per_epoch_median']:.3f} ms/epoch", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
