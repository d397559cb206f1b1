#!/usr/bin/env python3
"""Times one fidelity-curve epoch over S sparsity levels two ways and writes profiles/fidelity_curve_report.json:

  per_level -- the path as it was: S dp_gsat_amd.ReplayedFidelity instances, one per ratio, each .run over the epoch (every batch a replay
               of that instance's captured hipGraph: collate_padded, the eval-mode attention, the fused top-ratio mask, two padded
               extractions, three backbone forwards, FidelityLog.append);
  stacked   -- ONE dp_gsat_amd.ReplayedFidelityCurve.run: per batch one replay that ranks once, stacks the 2 S + 1 variants into one batch
               (a launch count that does not depend on S) and runs the backbone once; FidelityCurveLog.compute() reads the log once.

Both run on the same ragged budget batches.  Workloads and method are those of tools/bench_fidelity_replay.py: the example's 1000
BA-2motifs graphs and the 4337 Mutagenicity topologies, GIN (edge attention) and PNA (node attention), H 64, at most 128 graphs per batch
and a capacity near the mean batch; ratios 0.1 ... 0.9.  For each workload the two modes alternate in one process: both are warmed, then
5 rounds of one per_level and one stacked window, each of whole epochs, at least 1 s long and ending in a synchronise.  Reported per
mode: the median ms/epoch of the 5 windows, their min / max, and the kernel nodes of the captured graphs (per_level: of one instance,
and times S).  No ratio is expected in advance, and none is asserted.

  python tools/bench_fidelity_curve.py [--out profiles/fidelity_curve_report.json] [--window 1.0] [--rounds 5]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from bench_eval_replay import example_graphs, window
from bench_fidelity_replay import BATCH, HIDDEN, build, mutag_graphs

RATIOS = [round(0.1 * i, 1) for i in range(1, 10)]


def kept_graph():
    """A CUDAGraph that keeps its hipGraph for ``debug_dump``; None where torch cannot."""
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        return None
    graph.enable_debug_mode()
    return graph


def kernel_nodes(graph):
    """The number of kernel nodes of a kept graph, from hipGraphDebugDotPrint's dump; None without one."""
    if graph is None:
        return None
    try:
        path = os.path.join(tempfile.mkdtemp(), "graph.dot")
        graph.debug_dump(path)
        return len(re.findall(r"\{ID \| (\d+) \| (.*?)\\<\\<\\<", open(path, errors="replace").read())) or None
    except Exception:
        return None


def measure(name, graphs, x_dim, backbone, dev, seconds, rounds):
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = build(graphs, x_dim, dev, backbone)
    perm = np.random.RandomState(2).permutation(len(graphs))
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    capacity = (max(int(np.ceil(n_all.mean() * BATCH)), int(n_all.max())) + 2, max(int(np.ceil(e_all.mean() * BATCH)), int(e_all.max())))
    first = kept_graph()
    singles = [G.ReplayedFidelity(gsat, ds, BATCH, ratio=r, capacity=capacity, ragged=True, graph=first if i == 0 else None)
               for i, r in enumerate(RATIOS)]
    curve_graph = kept_graph()
    curve = G.ReplayedFidelityCurve(gsat, ds, BATCH, ratios=RATIOS, capacity=capacity, ragged=True, graph=curve_graph)
    nodes = dict(per_level_one_instance=kernel_nodes(first), stacked=kernel_nodes(curve_graph))
    results = {}

    def per_level_epoch():
        results["per_level"] = [rf.run(perm) for rf in singles]

    def stacked_epoch():
        results["stacked"] = curve.run(perm)

    for _ in range(3):                                        # warm both modes
        per_level_epoch()
        stacked_epoch()
    for s, single in enumerate(results["per_level"]):         # both modes scored the same epoch
        for key in ("p_keep", "p_drop"):
            assert abs(single[key] - results["stacked"][key][s]) <= 5e-3, (RATIOS[s], key, single[key], results["stacked"][key][s])
    times = {"per_level": [], "stacked": []}
    for _ in range(rounds):
        for mode, fn in (("per_level", per_level_epoch), ("stacked", stacked_epoch)):
            times[mode].append(window(fn, seconds))
    res = results["stacked"]
    out = dict(shape=name, backbone=backbone, graphs=len(graphs), max_batch=BATCH, hidden=HIDDEN, ratios=RATIOS,
               batches=int(len(curve.batches(perm))), edges=int(e_all.sum()), capacity=dict(nodes=capacity[0], edges=capacity[1]),
               stacked_edge_slots=int(curve.stack.segment_offsets[-1]), kernel_nodes=nodes,
               fidelity_plus=res["fidelity_plus"], fidelity_minus=res["fidelity_minus"], kept_fraction=res["kept_fraction"])
    for mode, t in times.items():
        out[mode] = dict(ms_per_epoch_median=statistics.median(t), ms_per_epoch_min=min(t), ms_per_epoch_max=max(t), windows=t)
    out["stacked_over_per_level"] = out["stacked"]["ms_per_epoch_median"] / out["per_level"]["ms_per_epoch_median"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fidelity_curve_report.json"))
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
            print(json.dumps({k: res[k] for k in ("shape", "backbone", "capacity", "batches", "kernel_nodes", "stacked_over_per_level")}), flush=True)
            print(f"  per_level {res['per_level']['ms_per_epoch_median']:.3f} ms/epoch  stacked {res['stacked']['ms_per_epoch_median']:.3f} ms/epoch",
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
