#!/usr/bin/env python3
"""Times the connectivity of explanations two ways and writes profiles/components_report.json:

  (a) scores -- per batch of 128 graphs with a pseudo-random attention and nine ratios,
        device -- dp_gsat_amd.explanation_connectivity: one ranking, the levels, ONE gsat_level_components launch, one host read of 72 counts;
        host   -- the same ranking and levels on the device, then ``level`` / ``edge_index`` / ``batch`` moved to the host and
                  scipy.sparse.csgraph.connected_components per graph and level, summed into the same counts (what a user does today);
      both build the batch index afresh per batch (clear_cache), and the warm-up asserts that they return the same dict;
  (b) epoch  -- one dp_gsat_amd.ReplayedFidelityCurve epoch over the same ragged budget batches with and without ``connectivity=True``.

Workloads and method are those of tools/bench_fidelity_curve.py: the example's 1000 BA-2motifs graphs and the 4337 Mutagenicity
topologies, GIN H 64, ratios 0.1 ... 0.9; (a) runs the first 8 full batches of a fixed permutation.  The two modes alternate in one
process: both are warmed, then 5 rounds of one window each, of whole epochs, at least 1 s long and ending in a synchronise.  Reported per
mode: the median ms/epoch of the 5 windows and their min / max.  No ratio is expected in advance, and none is asserted.

  python tools/bench_components.py [--out profiles/components_report.json] [--window 1.0] [--rounds 5]
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
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from bench_eval_replay import example_graphs, window
from bench_fidelity_curve import RATIOS
from bench_fidelity_replay import BATCH, HIDDEN, build, mutag_graphs

SCORE_BATCHES = 8


def host_counts(edge_index, batch, level, G, S):
    """int64[S][8] of gsat_level_components from scipy, graph by graph and level by level, on host arrays."""
    acc = np.zeros((S, 8), np.int64)
    eg = batch[edge_index[0]]
    order = np.argsort(eg, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(eg, minlength=G))])
    nptr = np.concatenate([[0], np.cumsum(np.bincount(batch, minlength=G))])
    for g in range(G):
        ids = order[ptr[g]:ptr[g + 1]]
        n = int(nptr[g + 1] - nptr[g])
        u, v, lv = edge_index[0, ids] - nptr[g], edge_index[1, ids] - nptr[g], level[ids]
        for s in range(S):
            keep = lv <= s
            acc[s, 0] += 1
            if not keep.any():
                continue
            a, b = u[keep], v[keep]
            _, lab = connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(n, n)), directed=False)
            touched = np.zeros(n, bool)
            touched[a] = touched[b] = True
            sizes = np.bincount(lab[touched])
            comps = int((sizes > 0).sum())
            acc[s, 1:7] += [comps, len(a), np.bincount(lab[a]).max(), int(touched.sum()), sizes.max(), int(comps == 1)]
    return acc


def measure_scores(name, graphs, dev, seconds, rounds):
    import dp_gsat_amd as G
    from dp_gsat_amd.explain import connectivity_scores
    ds = G.PackedDataset.from_data_list(graphs, dev)
    perm = np.random.RandomState(2).permutation(len(graphs))
    S = len(RATIOS)
    batches = [ds.collate(torch.as_tensor(perm[i * BATCH:(i + 1) * BATCH], device=dev)) for i in range(min(SCORE_BATCHES, len(graphs) // BATCH))]
    gen = torch.Generator().manual_seed(3)
    atts = [torch.rand(int(b.edge_index.shape[1]), generator=gen).to(dev) for b in batches]
    results = {}

    def device_epoch():
        out = []
        for b, att in zip(batches, atts):
            G.clear_cache()
            out.append(G.explanation_connectivity(b, att, ratios=RATIOS))
        results["device"] = out

    def host_epoch():
        out = []
        for b, att in zip(batches, atts):
            G.clear_cache()
            level = G.explanation_levels(att, b.edge_index, b.batch, ratios=RATIOS, num_graphs=b.num_graphs)
            acc = host_counts(b.edge_index.cpu().numpy(), b.batch.cpu().numpy(), level.cpu().numpy(), int(b.num_graphs), S)
            out.append(dict(connectivity_scores(acc.tolist()), levels=list(RATIOS)))
        results["host"] = out

    for _ in range(2):                                        # warm both modes
        device_epoch()
        host_epoch()
    assert results["device"] == results["host"], "the kernel and scipy disagree"
    times = {"device": [], "host": []}
    for _ in range(rounds):
        for mode, fn in (("device", device_epoch), ("host", host_epoch)):
            times[mode].append(window(fn, seconds))
    out = dict(shape=name, part="scores", batches=len(batches), graphs_per_batch=BATCH, ratios=RATIOS,
               edges=int(sum(int(b.edge_index.shape[1]) for b in batches)), first_batch=results["device"][0])
    for mode, t in times.items():
        out[mode] = dict(ms_per_epoch_median=statistics.median(t), ms_per_epoch_min=min(t), ms_per_epoch_max=max(t), windows=t)
    out["device_over_host"] = out["device"]["ms_per_epoch_median"] / out["host"]["ms_per_epoch_median"]
    G.clear_cache()
    return out


def measure_epoch(name, graphs, x_dim, dev, seconds, rounds):
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = build(graphs, x_dim, dev, "GIN")
    perm = np.random.RandomState(2).permutation(len(graphs))
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    capacity = (max(int(np.ceil(n_all.mean() * BATCH)), int(n_all.max())) + 2, max(int(np.ceil(e_all.mean() * BATCH)), int(e_all.max())))
    curves = {mode: G.ReplayedFidelityCurve(gsat, ds, BATCH, ratios=RATIOS, capacity=capacity, ragged=True, connectivity=mode == "with")
              for mode in ("without", "with")}
    results = {}

    def epoch(mode):
        results[mode] = curves[mode].run(perm)

    for _ in range(3):
        for mode in curves:
            epoch(mode)
    assert all(results["with"][k] == v for k, v in results["without"].items()), "connectivity=True changed the curve"
    times = {mode: [] for mode in curves}
    for _ in range(rounds):
        for mode in curves:
            times[mode].append(window(lambda: epoch(mode), seconds))
    res = results["with"]
    out = dict(shape=name, part="epoch", backbone="GIN", graphs=len(graphs), max_batch=BATCH, hidden=HIDDEN, ratios=RATIOS,
               batches=int(len(curves["with"].batches(perm))), capacity=dict(nodes=capacity[0], edges=capacity[1]),
               **{key: res[key] for key in ("components", "largest_edge_share", "largest_node_share", "connected_fraction")})
    for mode, t in times.items():
        out[mode] = dict(ms_per_epoch_median=statistics.median(t), ms_per_epoch_min=min(t), ms_per_epoch_max=max(t), windows=t)
    out["with_over_without"] = out["with"]["ms_per_epoch_median"] / out["without"]["ms_per_epoch_median"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_report.json"))
    ap.add_argument("--window", type=float, default=1.0, help="least length of a timed window, seconds")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    report = dict(device=torch.cuda.get_device_name(0), window_seconds=args.window, rounds=args.rounds, shapes=[])
    for name, make in (("mutag", mutag_graphs), ("ba2motifs_example", example_graphs)):
        graphs, x_dim = make()
        for res in (measure_scores(name, graphs, dev, args.window, args.rounds), measure_epoch(name, graphs, x_dim, dev, args.window, args.rounds)):
            report["shapes"].append(res)
            modes = [m for m in ("device", "host", "without", "with") if m in res]
            print(json.dumps({k: res[k] for k in ("shape", "part", "batches")}), flush=True)
            print("  " + "  ".join(f"{m} {res[m]['ms_per_epoch_median']:.3f} ms/epoch" for m in modes), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
