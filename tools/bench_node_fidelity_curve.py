#!/usr/bin/env python3
"""Times one NODE-fidelity-curve epoch over S sparsity levels two ways and writes profiles/node_fidelity_curve_report.json:

  per_level -- what a user could build before: ONE captured hipGraph per batch that collates, takes the eval-mode node attention, ranks
               the nodes once (node_levels) and then, level by level, runs two dp_gsat_amd.node_subgraph_padded extractions (5 launches
               each) and a backbone forward inside ``padded()`` on each -- 2 S extractions and 2 S + 1 forwards -- and appends the
               concatenated logits to a FidelityCurveLog;
  stacked   -- dp_gsat_amd.ReplayedFidelityCurve(unit="node"): per batch one replay that ranks once, stacks the 2 S + 1 node-induced
               variants into one batch (gsat_fidelity_stack_nodes: 5 launches whatever S is) and runs the backbone once.

Both run on the same ragged budget batches and fill the same log, so their scores are compared before anything is timed.  Workloads and
method are those of tools/bench_fidelity_curve.py: the example's 1000 BA-2motifs graphs and the 4337 Mutagenicity topologies, GIN and PNA
with NODE attention, H 64, at most 128 graphs per batch and a capacity near the mean batch; ratios 0.1 ... 0.9.  For each workload the two
modes alternate in one process: both are warmed, then 5 rounds of one per_level and one stacked window, each of whole epochs, at least
1 s long and ending in a synchronise.  Reported per mode: the median ms/epoch of the 5 windows, their min / max, and the kernel nodes of
the captured graph.  No ratio is expected in advance, and none is asserted.

  python tools/bench_node_fidelity_curve.py [--out profiles/node_fidelity_curve_report.json] [--window 1.0] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from bench_eval_replay import example_graphs, window
from bench_fidelity_curve import RATIOS, kept_graph, kernel_nodes
from bench_fidelity_replay import BATCH, HIDDEN, mutag_graphs


def build(graphs, x_dim, dev, backbone):
    """bench_fidelity_replay.build with node attention for both backbones."""
    import dp_gsat_amd as G
    torch.manual_seed(0)
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=HIDDEN, dropout_p=0.3, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=deg)
    clf = G.get_model(x_dim, 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(HIDDEN, False).to(dev)
    return G.GSAT(clf, ext, G.Criterion(2, False), None, learn_edge_att=False).train()


def per_level_class():
    import dp_gsat_amd as G

    class PerLevelNodeCurve(G.ReplayedFidelityCurve):
        """The captured body of the class with the stack taken out: per level two padded node extractions and their forwards."""

        def _forward(self, b, epoch=0):
            clf = self.gsat.clf
            with torch.no_grad():
                att = self.gsat.forward_pass(b, epoch, False)[0].node_att.detach()
                real = int(b.num_graphs) - 1
                level = G.node_levels(att, b.batch, ks=self.ks, ratios=self.ratios, num_graphs=int(b.num_graphs),
                                      max_seg_nodes=self.max_seg_nodes, ranked_graphs=real)
                S = len(self.ks if self.ks is not None else self.ratios)
                masks = [None] + [level <= s for s in range(S)] + [level > s for s in range(S)]
                logits, valids = [], []
                for mask in masks:
                    d = b if mask is None else G.node_subgraph_padded(b, mask, self.capacity)
                    G.get_index(d.edge_index, int(d.x.shape[0])).graphs(d.batch, int(d.num_graphs))
                    with G.padded(d.valid, d.capacity):
                        logits.append(clf(d.x, d.edge_index, d.batch, getattr(d, "edge_attr", None)))
                    valids.append(d.valid)
                logits, stack_valid = torch.cat(logits), torch.stack(valids)
                self.log.append(logits, stack_valid, b.valid)
            return att, SimpleNamespace(node_level=level, valid=stack_valid), logits

    return PerLevelNodeCurve


def measure(name, graphs, x_dim, backbone, dev, seconds, rounds):
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = build(graphs, x_dim, dev, backbone)
    perm = np.random.RandomState(2).permutation(len(graphs))
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    capacity = (max(int(np.ceil(n_all.mean() * BATCH)), int(n_all.max())) + 2, max(int(np.ceil(e_all.mean() * BATCH)), int(e_all.max())))
    graphs_kept = {"per_level": kept_graph(), "stacked": kept_graph()}
    kw = dict(ratios=RATIOS, capacity=capacity, ragged=True, unit="node")
    runs = {"per_level": per_level_class()(gsat, ds, BATCH, graph=graphs_kept["per_level"], **kw),
            "stacked": G.ReplayedFidelityCurve(gsat, ds, BATCH, graph=graphs_kept["stacked"], **kw)}
    nodes = {mode: kernel_nodes(g) for mode, g in graphs_kept.items()}
    results = {}

    def epoch(mode):
        def run():
            results[mode] = runs[mode].run(perm)
        return run

    for _ in range(3):                                        # warm both modes
        for mode in runs:
            epoch(mode)()
    a, b = results["per_level"], results["stacked"]           # both modes scored the same epoch from the same ranking
    assert a["kept_fraction"] == b["kept_fraction"] and a["kept_node_fraction"] == b["kept_node_fraction"] and a["n"] == b["n"]
    for key in ("p_keep", "p_drop"):
        assert max(abs(x - y) for x, y in zip(a[key], b[key])) <= 5e-3, (key, a[key], b[key])
    times = {mode: [] for mode in runs}
    for _ in range(rounds):
        for mode in runs:
            times[mode].append(window(epoch(mode), seconds))
    out = dict(shape=name, backbone=backbone, graphs=len(graphs), max_batch=BATCH, hidden=HIDDEN, ratios=RATIOS,
               batches=int(len(runs["stacked"].batches(perm))), nodes=int(n_all.sum()), edges=int(e_all.sum()),
               capacity=dict(nodes=capacity[0], edges=capacity[1]), stacked_edge_slots=int(runs["stacked"].stack.segment_offsets[-1]),
               stacked_node_rows=int(runs["stacked"].stack.x.shape[0]), kernel_nodes=nodes, fidelity_plus=b["fidelity_plus"],
               fidelity_minus=b["fidelity_minus"], kept_fraction=b["kept_fraction"], kept_node_fraction=b["kept_node_fraction"])
    for mode, t in times.items():
        out[mode] = dict(ms_per_epoch_median=statistics.median(t), ms_per_epoch_min=min(t), ms_per_epoch_max=max(t), windows=t)
    out["stacked_over_per_level"] = out["stacked"]["ms_per_epoch_median"] / out["per_level"]["ms_per_epoch_median"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_fidelity_curve_report.json"))
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
