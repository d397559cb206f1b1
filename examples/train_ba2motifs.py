#!/usr/bin/env python3
"""End-to-end GSAT training on a synthetic BA-2motifs-style dataset with the MI355X hot path.

Every graph is a 20-node Barabasi-Albert tree plus a 5-node motif (house -> label 1, cycle -> label 0) attached by one edge
(the construction of src/datasets/ba_2motifs.py); the motif's edges are the ground-truth explanation.  The script follows the
reference's training loop (example/trainer.py:28-60: forward_pass, zero_grad, backward, Adam; accuracy, and the ROC-AUC and precision@5 of the
learned edge attention against the motif edges, scored on the device by dp_gsat_amd.explain) on top of:
  * dp_gsat_amd.PackedDataset -- the dataset lives in HBM, every batch is collated on the device from graph ids;
  * dp_gsat_amd.get_model / ExtractorMLP / GSAT -- the reference's module protocol over the HIP kernels;
  * data parallelism (optional): `python -m torch.distributed.run --nproc-per-node N examples/train_ba2motifs.py` shards every
    global batch over the ranks by edge count (LPT), re-weights the local losses and all-reduces one flat gradient buffer.

  * dp_gsat_amd.ReplayedStep (``--graph``, single process) -- every full batch is collated to a fixed capacity and trained by replaying
    ONE captured hipGraph (collation, forward, backward, fused Adam); the tail batch of an epoch runs eagerly.
  * dp_gsat_amd.ReplayedEval (``--graph``) -- the periodic test evaluation replays a second captured graph (collation, eval-mode forward,
    append to a device log) batch by batch and scores the log once: two host reads per evaluation.

  * ``--graph --ragged`` -- no eager batch at all: both captured graphs take a ragged graph count (``ragged=True``), an epoch is cut
    into batches that fill a node / edge budget (PackedDataset.budget_batches, at most ``--batch-size`` graphs each) and the capacity
    is sized from the data (the mean graph times the batch size) instead of from the worst batch.

  * ``--graph --ragged --train-scores`` -- the training pass logs itself (``ReplayedStep(..., log_k=5)``): every replay appends its
    training-mode attention, logits and losses to a device log inside the captured graph, and each report line is followed by the
    scores of the training epoch (``epoch_scores()``: two host reads, no second pass over the training ids).

  * ``--graph [--ragged] --fidelity K`` -- each report line is followed by the fidelity of the top-K explanation on the test split
    (``dp_gsat_amd.ReplayedFidelity``): a third captured graph cuts the K best edges of every graph out on the device, runs the backbone
    on the full batch, on the explanation alone and on the batch without it, and logs the probabilities; one host read per epoch.

  * ``--graph [--ragged] --fidelity-curve 0.1,0.2,...`` -- each report line is followed by one line per sparsity level: the fidelity of
    the top-ratio explanation on the test split at every ratio (``dp_gsat_amd.ReplayedFidelityCurve``).  One captured graph ranks the
    edges once, stacks the batch, every explanation and every complement into ONE batch and runs the backbone once.
    ``--connectivity`` adds four lines under the curve: per level the mean number of connected components of the kept edges per graph,
    the share of kept edges and of touched nodes inside the largest component, and the fraction of graphs whose explanation is ONE
    piece (``connectivity=True``: one more kernel per batch in the same captured graph, one more host read per epoch).

  * ``--node-attention`` -- the extractor scores nodes (``learn_edge_att=False``); the edge attention is the lifted product.  With it,
    ``--fidelity-curve ... --fidelity-unit node`` ranks the NODES: every level keeps (or removes) the top-ratio nodes of each graph and
    the edges among them, and each level line also shows the fraction of nodes kept.  The class refuses ``--fidelity-unit node`` for a
    model that learns edge attention, and the example passes that refusal through.

  * ``--graph [--ragged] --pretrain N`` -- ``from_scratch: false`` of the reference (src/run_gsat.py:984-1007): the backbone is first
    trained alone for N epochs by ``dp_gsat_amd.pretrain_clf`` (ERM, every batch a replay, the training scores from a device log), one
    line per epoch; GSAT then starts from that backbone with a fresh optimizer over extractor + backbone.

  python examples/train_ba2motifs.py --graphs 1000 --epochs 20
  python examples/train_ba2motifs.py --graphs 1000 --epochs 20 --graph
  python examples/train_ba2motifs.py --graphs 1000 --epochs 20 --graph --ragged
  python examples/train_ba2motifs.py --graphs 1000 --epochs 20 --graph --ragged --train-scores
  python examples/train_ba2motifs.py --graphs 1000 --epochs 20 --graph --ragged --pretrain 10
  python examples/train_ba2motifs.py --graphs 1000 --epochs 20 --graph --pretrain 10 --baseline gnnexplainer,saliency
  python examples/train_ba2motifs.py --graphs 1000 --epochs 20 --graph --ragged --fidelity 5
  python examples/train_ba2motifs.py --graphs 1000 --epochs 20 --graph --ragged --fidelity-curve 0.2,0.5,0.8
  python examples/train_ba2motifs.py --graphs 1000 --epochs 20 --graph --ragged --node-attention --fidelity-curve 0.2,0.5,0.8 --fidelity-unit node
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_graphs(num_graphs, seed):
    rng = np.random.RandomState(seed)
    graphs = []
    for _ in range(num_graphs):
        edges, deg = [(0, 1)], np.zeros(20)
        deg[0] = deg[1] = 1
        for v in range(2, 20):
            u = int(rng.choice(v, p=deg[:v] / deg[:v].sum()))
            edges.append((u, v)); deg[u] += 1; deg[v] += 1
        n_base = len(edges)
        house = rng.rand() < 0.5
        m = 20
        if house:
            edges += [(m, m + 1), (m + 1, m + 2), (m + 2, m + 3), (m + 3, m), (m + 4, m), (m + 4, m + 1)]
        else:
            edges += [(m + i, m + (i + 1) % 5) for i in range(5)]
        n_motif = len(edges) - n_base
        edges.append((int(rng.randint(0, 20)), m))
        und = np.asarray(edges, dtype=np.int64)
        ei = np.concatenate([und, und[:, ::-1]], axis=0).T                      # both directions
        lab = np.zeros(len(edges), dtype=np.float32)
        lab[n_base:n_base + n_motif] = 1.0
        graphs.append(SimpleNamespace(x=torch.full((25, 10), 0.1), edge_index=torch.from_numpy(np.ascontiguousarray(ei)),
                                      y=torch.tensor([[float(house)]]), edge_label=torch.from_numpy(np.concatenate([lab, lab])),
                                      edge_attr=None))
    return graphs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1000)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=128, help="GLOBAL batch size")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--backbone", default="GIN", choices=["GIN", "PNA"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--backend", default="nccl", help="nccl (= RCCL, one GPU per rank) or gloo (to rehearse N ranks on one GPU)")
    ap.add_argument("--graph", action="store_true", help="train full batches as replays of one captured hipGraph (single process)")
    ap.add_argument("--ragged", action="store_true", help="with --graph: budget batches of a ragged graph count, every batch a replay")
    ap.add_argument("--train-scores", action="store_true", help="with --graph --ragged: log the training pass and print its scores")
    ap.add_argument("--fidelity", type=int, default=None, metavar="K", help="with --graph: print the fidelity of the top-K explanation on the test split")
    ap.add_argument("--fidelity-curve", type=lambda s: [float(v) for v in s.split(",")], default=None, metavar="R1,R2,...",
                    help="with --graph: print the fidelity of the top-ratio explanation on the test split at every ratio (increasing, in (0, 1])")
    ap.add_argument("--fidelity-unit", default="edge", choices=["edge", "node"],
                    help="with --fidelity-curve: rank and remove edges, or the nodes of a --node-attention model")
    ap.add_argument("--connectivity", action="store_true",
                    help="with --fidelity-curve (edges): print how connected the kept edges are at every ratio")
    ap.add_argument("--pretrain", type=int, default=0, metavar="N",
                    help="with --graph: pre-train the backbone alone for N epochs (pretrain_clf) and start GSAT from it")
    ap.add_argument("--node-attention", action="store_true", help="learn node attention (learn_edge_att=False) instead of edge attention")
    ap.add_argument("--baseline", type=lambda s: [v.strip() for v in s.split(",") if v.strip()], default=None, metavar="gnnexplainer,saliency",
                    help="with --pretrain: after training, score post-hoc explanations of the pre-trained (ERM) backbone next to GSAT's attention")
    args = ap.parse_args()

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if args.graph and world > 1:
        ap.error("--graph is single-process: it replays one captured step and cannot shard a batch over ranks")
    if args.ragged and not args.graph:
        ap.error("--ragged batches are replays: it needs --graph")
    if args.train_scores and not args.ragged:
        ap.error("--train-scores logs replays of every batch: it needs --graph --ragged")
    if args.fidelity is not None and not args.graph:
        ap.error("--fidelity replays a captured fidelity batch: it needs --graph")
    if args.fidelity_curve is not None and not args.graph:
        ap.error("--fidelity-curve replays a captured stacked batch: it needs --graph")
    if args.connectivity and (args.fidelity_curve is None or args.fidelity_unit != "edge"):
        ap.error("--connectivity scores the kept edges of --fidelity-curve: it needs it, with --fidelity-unit edge")
    if args.pretrain and not args.graph:
        ap.error("--pretrain replays the classifier step: it needs --graph")
    if args.baseline is not None:
        if not args.pretrain:
            ap.error("--baseline explains the ERM backbone that --pretrain trains: it needs --pretrain N")
        if not args.baseline or any(b not in ("gnnexplainer", "saliency") for b in args.baseline):
            ap.error("--baseline takes a comma-separated list of gnnexplainer and saliency")
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    import dp_gsat_amd as G
    from dp_gsat_amd.dist import FlatGradAllReduce, global_loss_weights, shard_graphs_lpt

    torch.manual_seed(args.seed)                                  # same initial weights on every rank
    graphs = make_graphs(args.graphs, args.seed)
    n_train = int(0.8 * len(graphs))
    ds = G.PackedDataset.from_data_list(graphs, dev)
    edge_counts = ds.edge_counts.cpu().numpy()
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=25) for g in graphs]), minlength=10)
    cfg = dict(model_name=args.backbone, n_layers=2, hidden_size=args.hidden, dropout_p=0.3, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std", "sum"], scalers=False, deg=deg)
    clf = G.get_model(10, 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(args.hidden, not args.node_attention).to(dev)
    erm_clf = None
    if args.pretrain > 0:
        # from_scratch: false -- ERM on the backbone alone, then the GSAT optimizer below over extractor + backbone (run_gsat.py:1005-1007)
        n_valid = max(1, (len(graphs) - n_train) // 2)
        splits = {"train": np.arange(n_train), "valid": np.arange(n_train, n_train + n_valid), "test": np.arange(n_train + n_valid, len(graphs))}
        slots = min(args.batch_size, n_train)
        pre_opt = torch.optim.Adam(clf.parameters(), lr=torch.tensor(1e-3, device=dev), weight_decay=3e-6, capturable=True, fused=True)
        best, history = G.pretrain_clf(clf, G.Criterion(2, False), pre_opt, ds, splits, args.pretrain, slots, ragged=args.ragged)
        for r in history:
            print(f"pretrain epoch {r['epoch'] + 1:3d}  train loss {r['train_loss']:.4f}  train acc {r['train']:.3f}  "
                  f"valid acc {r['valid']:.3f}  test acc {r['test']:.3f}", flush=True)
        print(f"pretrain best epoch {best['metric/best_clf_epoch'] + 1}  valid acc {best['metric/best_clf_valid']:.3f}  "
              f"test acc {best['metric/best_clf_test']:.3f}", flush=True)
        if args.baseline is not None:
            import copy
            erm_clf = copy.deepcopy(clf)                          # GSAT trains clf on from here; the baselines explain the ERM backbone
    params = list(clf.parameters()) + list(ext.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-6, **(dict(capturable=True, fused=True) if args.graph else {}))
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), opt, learn_edge_att=not args.node_attention)
    flat = FlatGradAllReduce(params) if world > 1 else None
    torch.manual_seed(args.seed + 1000 * rank)                    # independent noise / dropout per rank from here on

    def evaluate(ids):
        gsat.eval()
        with torch.no_grad():
            b = ds.collate(torch.as_tensor(ids, device=dev))
            att, _, _, logits = gsat.forward_pass(b, 0, False)
        gsat.train()
        acc = float(((logits > 0).float() == b.y).float().mean())
        # scored where the attention lives (no host copy of the [E] vector, no per-graph Python loop): one read of two scalars
        auc, prec = torch.stack([G.attention_auroc(att, b.edge_label),
                                 G.precision_at_k(att, b.edge_label, 5, b.batch, b.edge_index, b.num_graphs).double().mean()]).tolist()
        return acc, auc, prec

    replayed = replayed_eval = replayed_fidelity = replayed_curve = None
    if args.ragged:
        # the budget of a batch: batch_size graphs of the mean size (never less than the largest graph alone); one host read
        slots = min(args.batch_size, len(graphs))
        n_mean, e_mean, n_max, e_max = torch.stack([ds.node_counts.double().mean(), ds.edge_counts.double().mean(),
                                                    ds.node_counts.max().double(), ds.edge_counts.max().double()]).tolist()
        capacity = (max(int(np.ceil(n_mean * slots)), int(n_max)) + 2, max(int(np.ceil(e_mean * slots)), int(e_max)))
        replayed = G.ReplayedStep(gsat, ds, slots, capacity=capacity, ragged=True, log_k=5 if args.train_scores else None)
        replayed_eval = G.ReplayedEval(gsat, ds, slots, 5, capacity=capacity, ragged=True)
        if args.fidelity is not None:
            replayed_fidelity = G.ReplayedFidelity(gsat, ds, slots, k=args.fidelity, capacity=capacity, ragged=True)
        if args.fidelity_curve is not None:
            replayed_curve = G.ReplayedFidelityCurve(gsat, ds, slots, ratios=args.fidelity_curve, capacity=capacity, ragged=True,
                                                     unit=args.fidelity_unit, connectivity=args.connectivity)
    elif args.graph and n_train >= args.batch_size:
        replayed = G.ReplayedStep(gsat, ds, args.batch_size)      # capacity: ds.capacity_for(batch_size), which no batch exceeds
    if args.graph and not args.ragged:
        replayed_eval = G.ReplayedEval(gsat, ds, min(args.batch_size, len(graphs)), 5)
        if args.fidelity is not None:
            replayed_fidelity = G.ReplayedFidelity(gsat, ds, min(args.batch_size, len(graphs)), k=args.fidelity)
        if args.fidelity_curve is not None:
            replayed_curve = G.ReplayedFidelityCurve(gsat, ds, min(args.batch_size, len(graphs)), ratios=args.fidelity_curve,
                                                     unit=args.fidelity_unit, connectivity=args.connectivity)

    def evaluate_replayed(ids, epoch):
        res = replayed_eval.run(ids, epoch)      # full batches: replays; the tail: eager (--ragged: a replay too); one scoring pass at the end
        return res["clf_acc"], res["att_auroc"], res["precision@5"]

    gen = np.random.RandomState(args.seed)                        # identical permutations on every rank
    for epoch in range(args.epochs):
        perm = gen.permutation(n_train)
        tot, nb = 0.0, 0
        if args.ragged:
            replayed.begin_epoch()                                # empties the training-pass log, when there is one
            for row in replayed.batches(perm):                    # every batch fits the capacity and is a replay; the tail included
                tot, nb = tot + replayed.step(row, epoch), nb + 1
            if replayed.overflowed():
                raise RuntimeError("a budget batch overflowed its capacity")
        for s in ([] if args.ragged else range(0, n_train, args.batch_size)):
            ids = perm[s:s + args.batch_size]
            if replayed is not None and len(ids) == args.batch_size:
                tot, nb = tot + replayed.step(ids, epoch), nb + 1   # the loss stays on the device: no host read per step
                continue
            if world > 1:                                         # whole graphs to ranks, balanced by edge count
                ids = ids[shard_graphs_lpt(edge_counts[ids], world)[rank]]
            b = ds.collate(torch.as_tensor(ids, device=dev))
            w = global_loss_weights(b.num_graphs, b.edge_index.shape[1], dev) if world > 1 else None
            _, loss, ld, _ = gsat.forward_pass(b, epoch, True, loss_weights=w)
            if flat is not None:
                flat.zero_grad()
            else:
                opt.zero_grad(set_to_none=True)
            loss.backward()
            if flat is not None:
                flat.all_reduce(average=True, async_op=True)
                flat.wait()
            opt.step()
            tot, nb = tot + ld["loss"], nb + 1
        if rank == 0 and (epoch % 5 == 4 or epoch == args.epochs - 1):
            test_ids = np.arange(n_train, len(graphs))
            acc, auc, prec = evaluate_replayed(test_ids, epoch) if replayed_eval is not None else evaluate(test_ids)
            print(f"epoch {epoch + 1:3d}  train loss {float(tot) / nb:.4f}  test acc {acc:.3f}  attention ROC-AUC vs motif edges {auc:.3f}  prec@5 {prec:.3f}",
                  flush=True)
            if replayed_fidelity is not None:                     # needs no edge labels: three backbone forwards per batch, one host read
                res = replayed_fidelity.run(test_ids)
                print(f"      fidelity@{args.fidelity}  fidelity_plus {res['fidelity_plus']:.4f}  fidelity_minus {res['fidelity_minus']:.4f}  "
                      f"flip_plus {res['flip_plus']:.3f}  flip_minus {res['flip_minus']:.3f}", flush=True)
            if replayed_curve is not None:                        # every level from ONE ranking and ONE backbone forward per batch
                res = replayed_curve.run(test_ids)
                for s, ratio in enumerate(res["levels"]):
                    nodes = f"  kept nodes {res['kept_node_fraction'][s]:.3f}" if args.fidelity_unit == "node" else ""
                    print(f"      fidelity@{ratio:g}  kept {res['kept_fraction'][s]:.3f}{nodes}  fidelity_plus {res['fidelity_plus'][s]:.4f}  "
                          f"fidelity_minus {res['fidelity_minus'][s]:.4f}  flip_plus {res['flip_plus'][s]:.3f}  "
                          f"flip_minus {res['flip_minus'][s]:.3f}", flush=True)
                if args.connectivity:
                    for key in ("components", "largest_edge_share", "largest_node_share", "connected_fraction"):
                        print(f"      {key:<19}" + "".join(f"  {v:.3f}" for v in res[key]), flush=True)
            if args.train_scores:                                 # scored from what the replays of this epoch logged: no eager batch
                res = replayed.epoch_scores()
                print(f"      train  loss {res['loss']:.4f}  pred {res['pred']:.4f}  info {res['info']:.4f}  acc {res['clf_acc']:.3f}  "
                      f"clf ROC-AUC {res['clf_roc']:.3f}  attention ROC-AUC {res['att_auroc']:.3f}  prec@5 {res['precision@5']:.3f}", flush=True)
    if rank == 0 and erm_clf is not None:
        # GSAT's claim against post-hoc explainers, on the same test split and with the same two scores
        test_ids = np.arange(n_train, len(graphs))
        acc, auc, prec = evaluate_replayed(test_ids, args.epochs - 1) if replayed_eval is not None else evaluate(test_ids)
        print(f"explanations on the test split ({len(test_ids)} graphs)", flush=True)
        print(f"      {'GSAT attention':<26}  attention ROC-AUC {auc:.3f}  prec@5 {prec:.3f}  (test acc {acc:.3f})", flush=True)
        for name in args.baseline:
            if name == "gnnexplainer":                            # every batch three captured graphs: begin, 100 x step, end
                slots = min(args.batch_size, len(graphs))
                kw = dict(capacity=capacity, ragged=True) if args.ragged else {}
                res = G.ReplayedGNNExplainer(erm_clf, G.Criterion(2, False), ds, slots, 5, **kw).run(test_ids)
                auc, prec, acc = res["att_auroc"], res["precision@5"], res["clf_acc"]
            else:                                                 # one forward and one backward of the whole split
                b = ds.collate(torch.as_tensor(test_ids, device=dev))
                sal = G.edge_saliency(erm_clf, b)
                auc, prec = torch.stack([G.attention_auroc(sal, b.edge_label),
                                         G.precision_at_k(sal, b.edge_label, 5, b.batch, b.edge_index, b.num_graphs).double().mean()]).tolist()
                erm_clf.eval()
                with torch.no_grad():
                    acc = float(((erm_clf(b.x, b.edge_index, b.batch, edge_attr=b.edge_attr) > 0).float() == b.y).float().mean())
            print(f"      {name + ' on the ERM backbone':<26}  attention ROC-AUC {auc:.3f}  prec@5 {prec:.3f}  (test acc {acc:.3f})", flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
