#!/usr/bin/env python3
"""GSAT on a synthetic MULTI-TASK dataset (the shape of ogbg-moltox21 / molsider / molclintox) with every batch a hipGraph replay.

Every graph is a 20-node Barabasi-Albert tree plus a 5-node motif (house or cycle) attached by one edge, as in
examples/train_ba2motifs.py.  Each graph carries T = 3 binary labels derived from its structure -- the motif is a house; the motif hangs
on a node of the tree's first half; the tree's root has degree >= 4 -- and about 20 % of the label entries are NaN (unlabelled), the way
the OGB multi-task sets come.  Such a dataset has NO ground-truth explanation: ``edge_label`` is zero-filled, as the reference does
(src/utils/utils.py:31-32), and the attention scores against it are then 0 by the one-class rule (``att_auroc``, ``precision@k``).

The multi-label criterion boolean-indexes the labelled entries, which no captured graph can hold; constructed as
``Criterion(T, True, capturable=True)`` it runs as HIP kernels that count the labelled entries on the device instead, and the replay
classes take it:
  * dp_gsat_amd.ReplayedStep(..., ragged=True, log_k=5) trains every budget batch as a replay and logs the training pass;
  * dp_gsat_amd.ReplayedEval(..., ragged=True) scores the test split: ``clf_roc`` is the ogb mean over the scorable tasks and
    ``clf_roc_tasks`` the per-task ROC-AUCs (NaN for a task without both classes among its labelled rows);
  * ``--fidelity-curve 0.2,0.5,0.8``: dp_gsat_amd.ReplayedFidelityCurve reports the fidelity of the top-ratio explanation per level
    and per task (every (graph, task) is a binary decision of its own).

  python examples/train_multitask.py --graphs 600 --epochs 10 --graph --ragged --fidelity-curve 0.2,0.5,0.8
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.train_ba2motifs import make_graphs  # noqa: E402

T = 3


def make_multitask_graphs(num_graphs, seed):
    """``make_graphs`` with y [1, T] derived from the structure, about 20 % of the entries NaN, and a zero-filled ``edge_label``."""
    graphs = make_graphs(num_graphs, seed)
    rng = np.random.RandomState(seed + 1)
    for g in graphs:
        ei = g.edge_index.numpy()
        half = ei.shape[1] // 2                                   # the undirected edges come first, then their reverses
        attach = int(ei[0, half - 1])                             # the tree node the motif hangs on
        root_degree = int((ei[0, :half] == 0).sum() + (ei[1, :half] == 0).sum())
        y = np.array([float(g.y), float(attach < 10), float(root_degree >= 4)], dtype=np.float32)
        y[rng.rand(T) < 0.2] = np.nan
        g.y = torch.from_numpy(y).view(1, T)
        g.edge_label = torch.zeros(ei.shape[1])                   # no ground-truth explanation: zero-filled, as the reference does
    return graphs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=64, help="graph slots per batch")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--backbone", default="GIN", choices=["GIN", "PNA"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graph", action="store_true", help="train and evaluate as replays of captured hipGraphs")
    ap.add_argument("--ragged", action="store_true", help="with --graph: budget batches of a ragged graph count, every batch a replay")
    ap.add_argument("--fidelity-curve", type=lambda s: [float(v) for v in s.split(",")], default=None, metavar="R1,R2,...",
                    help="print the per-task fidelity of the top-ratio explanation on the test split at every ratio (increasing, in (0, 1])")
    args = ap.parse_args()
    if not (args.graph and args.ragged):
        ap.error("this example shows the replayed multi-task path: run it with --graph --ragged")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import dp_gsat_amd as G

    torch.manual_seed(args.seed)
    graphs = make_multitask_graphs(args.graphs, args.seed)
    n_train = int(0.8 * len(graphs))
    ds = G.PackedDataset.from_data_list(graphs, dev)
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=25) for g in graphs]), minlength=10)
    cfg = dict(model_name=args.backbone, n_layers=2, hidden_size=args.hidden, dropout_p=0.3, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std", "sum"], scalers=False, deg=deg)
    clf = G.get_model(10, 0, T, True, cfg, dev)
    ext = G.ExtractorMLP(args.hidden, True).to(dev)
    opt = torch.optim.Adam(list(clf.parameters()) + list(ext.parameters()), lr=1e-3, weight_decay=3e-6, capturable=True, fused=True)
    gsat = G.GSAT(clf, ext, G.Criterion(T, True, capturable=True), opt, learn_edge_att=True)      # the opt-in: capturable=True

    slots = min(args.batch_size, len(graphs))
    n_mean, e_mean, n_max, e_max = torch.stack([ds.node_counts.double().mean(), ds.edge_counts.double().mean(),
                                                ds.node_counts.max().double(), ds.edge_counts.max().double()]).tolist()
    capacity = (max(int(np.ceil(n_mean * slots)), int(n_max)) + 2, max(int(np.ceil(e_mean * slots)), int(e_max)))
    step = G.ReplayedStep(gsat, ds, slots, capacity=capacity, ragged=True, log_k=5)
    evaluator = G.ReplayedEval(gsat, ds, slots, 5, capacity=capacity, ragged=True)
    curve = None
    if args.fidelity_curve is not None:
        curve = G.ReplayedFidelityCurve(gsat, ds, slots, ratios=args.fidelity_curve, capacity=capacity, ragged=True)

    fmt = lambda values: "[" + ", ".join(f"{v:.3f}" for v in values) + "]"
    gen = np.random.RandomState(args.seed)
    test_ids = np.arange(n_train, len(graphs))
    for epoch in range(args.epochs):
        step.begin_epoch()
        for row in step.batches(gen.permutation(n_train)):
            step.step(row, epoch)
        if step.overflowed():
            raise RuntimeError("a budget batch overflowed its capacity")
        train, test = step.epoch_scores(), evaluator.run(test_ids, epoch)
        print(f"epoch {epoch + 1:3d}  train loss {train['loss']:.4f}  clf_roc {train['clf_roc']:.3f}  |  test loss {test['loss']:.4f}  "
              f"clf_acc {test['clf_acc']:.3f}  clf_roc {test['clf_roc']:.3f}  clf_roc_tasks {fmt(test['clf_roc_tasks'])}  "
              f"att_auroc {test['att_auroc']:.1f} (no edge labels)", flush=True)
        if curve is not None and (epoch % 5 == 4 or epoch == args.epochs - 1):
            res = curve.run(test_ids)
            for s, ratio in enumerate(res["levels"]):
                print(f"      fidelity@{ratio:g}  kept {res['kept_fraction'][s]:.3f}  fidelity_plus {res['fidelity_plus'][s]:.4f}  "
                      f"fidelity_minus {res['fidelity_minus'][s]:.4f}  fidelity_plus_tasks {fmt(res['fidelity_plus_tasks'][s])}  "
                      f"fidelity_minus_tasks {fmt(res['fidelity_minus_tasks'][s])}", flush=True)


if __name__ == "__main__":
    main()
