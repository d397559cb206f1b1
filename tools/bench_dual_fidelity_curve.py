#!/usr/bin/env python3
"""Times one fidelity-curve epoch of the dual/primal pair's TWO explanations two ways and writes
profiles/dual_fidelity_curve_report.json:

  two_stacks  -- the captured body of dp_gsat_amd.ReplayedDualFidelityCurve with the scoring as it would be without the multi-ranking
                 stack: two ``explanation_stack`` calls (the full variant laid out twice), two ``primal_clf`` forwards, two
                 FidelityCurveLog appends, and the level overlap;
  multi_stack -- dp_gsat_amd.ReplayedDualFidelityCurve itself: ONE ``explanation_stack_multi`` of 1 + 4 S variants, ONE forward, one append.

Everything before the scoring -- collate_padded_pair, the seed word, the eval-mode dual_forward_pass -- is the same code in both.  The
method is that of tools/bench_fidelity_curve.py: Mutagenicity (4337 topologies, random edge labels) and its dual, GIN H 64 on both sides,
128 graph slots per ragged batch under a near-mean three-budget capacity, ratios 0.2 ... 0.8; both modes are warmed, then 5 rounds of
one two_stacks and one multi_stack window, each of whole epochs, at least 1 s long and ending in a synchronise.  Reported per mode: the
median ms/epoch of the 5 windows, their min / max, and the kernel nodes of a captured graph.  No ratio is expected in advance, and none
is asserted.

  python tools/bench_dual_fidelity_curve.py [--out profiles/dual_fidelity_curve_report.json] [--window 1.0] [--rounds 5]
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
from bench_eval_replay import BATCH, HIDDEN, window
from bench_fidelity_curve import kept_graph, kernel_nodes
from bench_padded import mutag_graphs

RATIOS = [0.2, 0.4, 0.6, 0.8]


def two_stacks_class():
    import dp_gsat_amd as G
    from dp_gsat_amd.subgraph import explanation_stack

    class TwoStacks(G.ReplayedDualFidelityCurve):
        """The same captured body, scored ranking by ranking: what the pair would cost without gsat_fidelity_stack_multi."""

        def _make_log(self):
            super()._make_log()
            self.logs = [G.FidelityCurveLog(self._max_graphs, self.log.classes, self.ks, self.ratios, self.primal_ds.x_all.device)
                         for _ in range(2)]

        def _reset(self):
            super()._reset()
            for log in getattr(self, "logs", ()):
                log.reset()

        def _score(self, pb, att, dual_att):
            valid = getattr(pb, "valid", None)
            stacks = []
            for a, log in zip((att, dual_att), self.logs):
                stack = explanation_stack(pb, a, ks=self.ks, ratios=self.ratios, batch_size=self.batch_size, max_seg_edges=self.max_seg_edges)
                logits = self.model.primal_clf(stack.x, stack.edge_index, stack.batch, stack.edge_attr)
                over = stack.valid[:, 3].amax().view(1)
                self._overflow.bitwise_or_(over if valid is None else over | valid[3:4])
                log.append(logits, stack.valid, valid)
                stacks.append((stack, logits))
            G.level_overlap(stacks[0][0].edge_level, stacks[1][0].edge_level, len(self.levels), valid=valid, out=self.overlap)
            stack, logits = stacks[0]
            stack.edge_level = torch.stack([s.edge_level for s, _ in stacks])
            return stack, logits

        def run_two(self, perm, epoch=0):
            """One epoch; the two curves come from the two logs."""
            self._set_seed_state(int(epoch) << 32)
            self._reset()
            for row in self.batches(torch.as_tensor(perm)):
                self.step(row, epoch)
            return [log.compute() for log in self.logs], self.overlap.tolist()

    return TwoStacks


def measure(ds, dual, dev, seconds, rounds):
    import dp_gsat_amd as G
    model = build(dev, False)
    perm = np.random.RandomState(2).permutation(ds.num_graphs)
    counts = [c.cpu().numpy() for c in (ds.node_counts, ds.edge_counts, dual.edge_counts)]
    capacity = tuple(max(int(np.ceil(c.mean() * BATCH)), int(c.max())) + (2 if i == 0 else 0) for i, c in enumerate(counts))
    graphs = {name: (kept_graph(), torch.cuda.CUDAGraph()) for name in ("two_stacks", "multi_stack")}
    pair = None if graphs["two_stacks"][0] is None else graphs["two_stacks"]
    two = two_stacks_class()(model, ds, dual, BATCH, ratios=RATIOS, capacity=capacity, seed=1, ragged=True, graphs=pair)
    pair = None if graphs["multi_stack"][0] is None else graphs["multi_stack"]
    multi = G.ReplayedDualFidelityCurve(model, ds, dual, BATCH, ratios=RATIOS, capacity=capacity, seed=1, ragged=True, graphs=pair)
    nodes = dict(two_stacks=kernel_nodes(graphs["two_stacks"][0]), multi_stack=kernel_nodes(graphs["multi_stack"][0]))
    results = {}

    def two_epoch():
        results["two_stacks"] = two.run_two(perm)

    def multi_epoch():
        results["multi_stack"] = multi.run(perm, 0)

    for _ in range(3):                                        # warm both modes
        two_epoch()
        multi_epoch()
    res = results["multi_stack"]
    (first, second), overlap = results["two_stacks"]          # both modes scored the same epoch with the same seed words
    for name, single in (("primal", first), ("dual", second)):
        for key in ("p_keep", "p_drop", "kept_fraction"):
            assert np.max(np.abs(np.asarray(single[key]) - np.asarray(res[name][key]))) <= 5e-3, (name, key, single[key], res[name][key])
    assert overlap == multi.overlap.tolist()
    times = {"two_stacks": [], "multi_stack": []}
    for _ in range(rounds):
        for mode, fn in (("two_stacks", two_epoch), ("multi_stack", multi_epoch)):
            times[mode].append(window(fn, seconds))
    out = dict(shape="mutag_dual_fidelity_curve", graphs=ds.num_graphs, max_batch=BATCH, hidden=HIDDEN, ratios=RATIOS,
               batches=int(len(multi.batches(torch.as_tensor(perm)))), capacity=dict(zip(("nodes", "edges", "dual_edges"), capacity)),
               stacked_edge_slots=dict(two_stacks=2 * int(two.stack.segment_offsets[-1]), multi_stack=int(multi.stack.segment_offsets[-1])),
               kernel_nodes_unmixed_graph=nodes, primal=res["primal"], dual=res["dual"], jaccard=res["jaccard"], overlap=res["overlap"])
    for mode, t in times.items():
        out[mode] = dict(ms_per_epoch_median=statistics.median(t), ms_per_epoch_min=min(t), ms_per_epoch_max=max(t), windows=t)
    out["multi_over_two"] = out["multi_stack"]["ms_per_epoch_median"] / out["two_stacks"]["ms_per_epoch_median"]
    G.clear_cache()
    return out


def main():
    import dp_gsat_amd as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_fidelity_curve_report.json"))
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
                  window_seconds=args.window, rounds=args.rounds, shapes=[])
    res = measure(ds, dual, dev, args.window, args.rounds)
    report["shapes"].append(res)
    print(json.dumps({k: res[k] for k in ("shape", "capacity", "batches", "kernel_nodes_unmixed_graph", "multi_over_two")}), flush=True)
    print(f"  two_stacks {res['two_stacks']['ms_per_epoch_median']:.3f} ms/epoch  multi_stack {res['multi_stack']['ms_per_epoch_median']:.3f} ms/epoch",
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
