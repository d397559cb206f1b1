#!/usr/bin/env python3
"""Times a training EPOCH over ragged batches four ways and one step two ways, and writes profiles/ragged_replay_report.json.

Per epoch (one fixed shuffle of the dataset, batch / slot count 128), by the method of tools/bench_padded.py:
  a       -- ReplayedStep at PackedDataset.capacity_for(128), the bound over every possible batch; the tail batch runs eagerly;
  b       -- ReplayedStep at the tightest capacity that holds this shuffle's full batches; the tail batch runs eagerly;
  c_tight -- ReplayedStep(ragged=True) over PackedDataset.budget_batches at capacity (b): every batch is a replay;
  c_mean  -- the same at a capacity near the mean batch (128 graphs of the mean size, at least the largest graph).
The configurations alternate in one process: all are warmed, then ``--rounds`` rounds of one window each, every window whole epochs for at
least ``--window`` seconds and ending in a synchronise.  Reported per configuration: the median ms/epoch of the windows, their min / max,
ms per graph, and the batches per epoch.

Per step: ReplayedStep(ragged=True) on FULL batches of 16 and of 128 graphs against ReplayedStep without ``ragged`` -- the step as it was
before the graph count became ragged: the same collation kernel, torch's criterion on a host slice -- at the same capacity
(capacity_for), in alternating windows.

Shapes: tools/bench_padded.py's (800 BA-2motifs graphs; the 4337 Mutagenicity topologies of tests/golden/mutag_full.npz), GIN, H 64, edge
attention.

  python tools/bench_ragged_replay.py [--out profiles/ragged_replay_report.json] [--window 1.0] [--rounds 5]
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

from bench_padded import BATCH, HIDDEN, build, example_graphs, mutag_graphs


def summary(times):
    return dict(median=statistics.median(times), min=min(times), max=max(times), windows=times)


def timed(fn, seconds):
    """ms per call of ``fn`` over a window of whole calls lasting at least ``seconds`` and ending in a synchronise."""
    calls = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while True:
        fn()
        calls += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def eager_step(gsat, ds, ids, dev):
    b = ds.collate(torch.as_tensor(ids, device=dev))
    _, loss, ld, _ = gsat.forward_pass(b, 0, True)
    gsat.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    gsat.optimizer.step()
    return ld["loss"]


def measure_epochs(name, graphs, x_dim, dev, seconds, rounds):
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    perm = np.random.RandomState(1).permutation(len(graphs))
    full = [perm[s:s + BATCH] for s in range(0, len(perm) - BATCH + 1, BATCH)]
    tail = perm[len(full) * BATCH:]
    bound = ds.capacity_for(BATCH)
    tight = (max(int(n_all[u].sum()) for u in full) + 2, max(int(e_all[u].sum()) for u in full))
    mean = (max(int(np.ceil(n_all.mean() * BATCH)), int(n_all.max())) + 2, max(int(np.ceil(e_all.mean() * BATCH)), int(e_all.max())))
    configs, runs = {}, {}

    def fixed(capacity):
        gsat = build(graphs, x_dim, dev, True)
        rs = G.ReplayedStep(gsat, ds, BATCH, capacity=capacity)
        rs.check_epoch(perm)

        def epoch():
            for ids in full:
                rs.step(ids, 0)
            if len(tail):
                eager_step(gsat, ds, tail, dev)
        return rs, epoch, len(full) + (1 if len(tail) else 0), 1 if len(tail) else 0

    def ragged(capacity):
        gsat = build(graphs, x_dim, dev, True)
        rs = G.ReplayedStep(gsat, ds, BATCH, capacity=capacity, ragged=True)
        rows = rs.batches(perm)

        def epoch():
            for row in rows:
                rs.step(row, 0)
        return rs, epoch, int(rows.shape[0]), 0

    for key, make, capacity in (("a", fixed, bound), ("b", fixed, tight), ("c_tight", ragged, tight), ("c_mean", ragged, mean)):
        rs, epoch, batches, eager_batches = make(capacity)
        runs[key] = (rs, epoch)
        configs[key] = dict(capacity=dict(nodes=capacity[0], edges=capacity[1]), batches_per_epoch=batches, eager_batches_per_epoch=eager_batches)
    for _ in range(2):                                      # warm every configuration
        for rs, epoch in runs.values():
            epoch()
    times = {key: [] for key in runs}
    for _ in range(rounds):
        for key, (rs, epoch) in runs.items():
            times[key].append(timed(epoch, seconds))
    for key, (rs, _) in runs.items():
        assert not rs.overflowed(), f"{name} {key}: a timed batch did not fit its capacity"
        configs[key]["ms_per_epoch"] = summary(times[key])
        configs[key]["ms_per_graph"] = configs[key]["ms_per_epoch"]["median"] / len(graphs)
    G.clear_cache()
    return dict(shape=name, graphs=len(graphs), slots=BATCH, hidden=HIDDEN,
                mean_batch=dict(nodes=float(n_all.mean() * BATCH), edges=float(e_all.mean() * BATCH)), configurations=configs,
                c_mean_over_b=configs["c_mean"]["ms_per_epoch"]["median"] / configs["b"]["ms_per_epoch"]["median"])


def measure_step(name, graphs, x_dim, dev, slots, seconds, rounds):
    """A FULL batch of ``slots`` graphs: ReplayedStep with and without ``ragged`` at capacity_for(slots), ms per step."""
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gen = np.random.RandomState(2)
    pool = [gen.permutation(len(graphs))[:slots] for _ in range(64)]
    runs = {}
    for key, is_ragged in (("fixed_count", False), ("ragged", True)):
        rs = G.ReplayedStep(build(graphs, x_dim, dev, True), ds, slots, ragged=is_ragged)

        def sweep(rs=rs):
            for ids in pool:
                rs.step(ids, 0)
        runs[key] = (rs, sweep)
    for rs, sweep in runs.values():
        sweep()
    times = {key: [] for key in runs}
    for _ in range(rounds):
        for key, (rs, sweep) in runs.items():
            times[key].append(timed(sweep, seconds) / len(pool))
    out = dict(shape=name, slots=slots, capacity=dict(zip(("nodes", "edges"), runs["ragged"][0].capacity)))
    for key, (rs, _) in runs.items():
        assert not rs.overflowed() and int(rs.batch.valid[2]) == slots
        out[key] = dict(ms_per_step=summary(times[key]))
    med = out["ragged"]["ms_per_step"]["median"]
    out["ragged_within_fixed_count_spread"] = bool(out["fixed_count"]["ms_per_step"]["min"] <= med <= out["fixed_count"]["ms_per_step"]["max"])
    out["ragged_over_fixed_count"] = med / out["fixed_count"]["ms_per_step"]["median"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_replay_report.json"))
    ap.add_argument("--window", type=float, default=1.0, help="least length of a timed window, seconds")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    report = dict(device=torch.cuda.get_device_name(0), window_seconds=args.window, rounds=args.rounds, epochs=[], steps=[])
    for name, make in (("ba2motifs_example", example_graphs), ("mutag", mutag_graphs)):
        graphs, x_dim = make()
        res = measure_epochs(name, graphs, x_dim, dev, args.window, args.rounds)
        report["epochs"].append(res)
        for key, c in res["configurations"].items():
            print(f"{name} {key}: capacity {c['capacity']}  {c['batches_per_epoch']} batches  {c['ms_per_epoch']['median']:.2f} ms/epoch "
                  f"[{c['ms_per_epoch']['min']:.2f}, {c['ms_per_epoch']['max']:.2f}]  {c['ms_per_graph']:.5f} ms/graph", flush=True)
        for slots in (16, BATCH):
            res = measure_step(name, graphs, x_dim, dev, slots, args.window, args.rounds)
            report["steps"].append(res)
            f, r = res["fixed_count"]["ms_per_step"], res["ragged"]["ms_per_step"]
            print(f"{name} full batch of {slots}: fixed count {f['median']:.4f} ms/step [{f['min']:.4f}, {f['max']:.4f}]  "
                  f"ragged {r['median']:.4f} [{r['min']:.4f}, {r['max']:.4f}]", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
