#!/usr/bin/env python3
"""Times the dual/primal (DualGSAT) training step over ragged batches two ways and writes profiles/dual_replay_report.json:

  eager    -- two PackedDataset.collate calls (primal and dual dataset) and DualGSAT's training step: dual_forward_pass, both zero_grad,
              backward, both Adam steps and the one host read of the loss dict;
  replayed -- dp_gsat_amd.ReplayedDualStep: the ids are copied into a static buffer and ONE captured hipGraph (collate_padded_pair to a
              fixed capacity, forward, backward, two fused capturable Adam steps) is replayed; nothing is read back.

Shape: the topology of all 4337 Mutagenicity graphs (tests/golden/mutag_full.npz; node labels, graph labels and edge labels are drawn at
random, the fixture stores none) and its dual dataset, batches of 128 graphs, GIN, H 64, 2 layers, node attention on both sides.  The two
modes alternate in one process: both are warmed, then 5 rounds of one eager and one replayed window, each of at least 1 s and ending in
a synchronise.  Reported per mode: the median ms/step of the 5 windows and their min / max; the capacity, the mean real size and the
padding share (cap - mean real) / cap for primal nodes, primal edges (= dual nodes) and dual edges.  Timed at the bound capacity
(PackedDataset.pair_capacity_for(dual, 128)) and again at the tightest capacity that holds the batches visited (a fixed pool of 512,
vetted with ReplayedDualStep.check_epoch).  Epoch 0 throughout: the unmixed graph.

  python tools/bench_dual_replay.py [--out profiles/dual_replay_report.json] [--window 1.0] [--rounds 5]
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

from bench_padded import BATCH, HIDDEN, cycle, id_pool, mutag_graphs, window

MCFG = dict(pred_loss_coef=1, info_loss_coef=1, fix_r=False, decay_interval=10, decay_r=0.1, final_r=0.5)
SHARED = {"learn_edge_att": False, "extractor_dropout_p": 0.5}


def build(dev, capturable):
    import dp_gsat_amd as G
    torch.manual_seed(0)
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=HIDDEN, dropout_p=0.3, use_edge_attr=False)
    mods, opts = [], []
    for x_dim, side in ((14, "primal"), (28, "dual")):
        clf = G.get_model(x_dim, 0, 2, False, cfg, dev)
        ext = G.ExtractorMLP(HIDDEN, SHARED, side).to(dev)
        params = list(clf.parameters()) + list(ext.parameters())
        opts.append(torch.optim.Adam(params, lr=1e-3, weight_decay=3e-6, **(dict(capturable=True, fused=True) if capturable else {})))
        mods += [clf, ext]
    return G.DualGSAT(mods[0], mods[1], opts[0], mods[2], mods[3], opts[1], MCFG, MCFG, False, False).train()


def measure(name, ds, dual, dev, seconds, rounds, tight):
    import dp_gsat_amd as G
    eager, captured = build(dev, False), build(dev, True)
    pool = id_pool(ds.num_graphs, 1)
    counts = [c.cpu().numpy() for c in (ds.node_counts, ds.edge_counts, dual.edge_counts)]
    capacity = None
    if tight:
        n, e, ed = (max(int(c[u].sum()) for u in pool) for c in counts)
        capacity = (n + 2, e, ed)
    replayed = G.ReplayedDualStep(captured, ds, dual, BATCH, capacity=capacity)
    replayed.check_epoch(np.concatenate(pool))

    def eager_step(ids):
        idt = torch.as_tensor(ids, device=dev)
        pb, db = ds.collate(idt), dual.collate(idt)
        _, loss, ld, _ = eager.dual_forward_pass(pb, db, 0, True)
        eager.primal_optimizer.zero_grad(set_to_none=True)
        eager.dual_optimizer.zero_grad(set_to_none=True)
        loss.backward()
        eager.primal_optimizer.step()
        eager.dual_optimizer.step()
        return ld["loss"]

    def replayed_step(ids):
        return replayed.step(ids, 0)

    ids = cycle(pool)
    for _ in range(30):                                    # warm both modes
        eager_step(next(ids))
        replayed_step(next(ids))
    times = {"eager": [], "replayed": []}
    real = [[], [], []]
    for _ in range(rounds):
        for mode, fn in (("eager", eager_step), ("replayed", replayed_step)):
            ms, used = window(fn, ids, seconds)
            times[mode].append(ms)
            for r, c in zip(real, counts):
                r += [int(c[u].sum()) for u in used]
    assert not replayed.overflowed(), "a timed batch did not fit the capacity"
    keys = ("nodes", "edges", "dual_edges")
    mean = [float(np.mean(r)) for r in real]
    out = dict(shape=name, graphs=ds.num_graphs, batch=BATCH, hidden=HIDDEN, capacity_rule="pool maximum" if tight else "pair_capacity_for",
               capacity=dict(zip(keys, replayed.capacity)), mean_real=dict(zip(keys, mean)),
               padding_share={k: (c - m) / c for k, c, m in zip(keys, replayed.capacity, mean)})
    for mode, t in times.items():
        out[mode] = dict(ms_per_step_median=statistics.median(t), ms_per_step_min=min(t), ms_per_step_max=max(t), windows=t)
    out["replayed_over_eager"] = out["replayed"]["ms_per_step_median"] / out["eager"]["ms_per_step_median"]
    G.clear_cache()
    return out


def main():
    import dp_gsat_amd as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_replay_report.json"))
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
    for name, tight in (("mutag_dual_batch128", False), ("mutag_dual_batch128_tight_capacity", True)):
        res = measure(name, ds, dual, dev, args.window, args.rounds, tight)
        report["shapes"].append(res)
        print(json.dumps({k: res[k] for k in ("shape", "capacity", "padding_share", "replayed_over_eager")}), flush=True)
        print(f"  eager {res['eager']['ms_per_step_median']:.3f} ms/step  replayed {res['replayed']['ms_per_step_median']:.3f} ms/step", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
