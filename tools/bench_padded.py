#!/usr/bin/env python3
"""Times a training step over ragged batches two ways and writes profiles/padded_replay_report.json:

  eager    -- the loop of examples/train_ba2motifs.py: PackedDataset.collate(ids), forward_pass, zero_grad, backward, Adam, and the one
              host read of the loss dict per step;
  replayed -- dp_gsat_amd.ReplayedStep: the ids are copied into a static buffer and ONE captured hipGraph (collate_padded to a fixed
              capacity, forward, backward, fused capturable Adam) is replayed; nothing is read back.

Shapes: the example's (1000 BA-2motifs graphs, 800 for training, batch 128, GIN, H 64, edge attention) and Mutagenicity batches of 128
graphs, H 64 (the topology of all 4337 graphs from tests/golden/mutag_full.npz; node labels and graph labels are drawn at random, the
fixture stores none).  For each shape the two modes alternate in one process: both are warmed, then 5 rounds of one eager and one
replayed window, each of at least 1 s and ending in a synchronise.  Reported per mode: the median ms/step of the 5 windows and their
min / max; per shape: the capacity, the mean real size and the padding share (cap - mean real) / cap for nodes and edges.
The capacity is PackedDataset.capacity_for(128), the bound over every possible batch; the Mutagenicity shape is timed a second time with
the tightest capacity that holds the batches it visits (a fixed pool of 512, vetted with ReplayedStep.check_epoch), because the sum of
the 128 largest of 4337 graphs is several times a typical batch.

  python tools/bench_padded.py [--out profiles/padded_replay_report.json] [--window 1.0] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import numpy as np
import torch

BATCH, HIDDEN = 128, 64


def example_graphs():
    from train_ba2motifs import make_graphs
    graphs = make_graphs(1000, 0)
    return graphs[:800], 10


def mutag_graphs():
    from dp_gsat_amd import synth
    ei, batch, _ = synth.mutag_full_topology(os.path.join(ROOT, "tests", "golden", "mutag_full.npz"))
    rng = np.random.RandomState(0)
    counts = torch.bincount(batch)
    start = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    eg = batch[ei[0]]
    order = torch.argsort(eg, stable=True)
    ecount = torch.bincount(eg, minlength=len(counts))
    estart = torch.cat([torch.zeros(1, dtype=torch.int64), ecount.cumsum(0)])
    ei = ei[:, order]
    graphs = []
    for g in range(len(counts)):
        n = int(counts[g])
        x = torch.zeros(n, 14)
        x[torch.arange(n), torch.from_numpy(rng.randint(0, 14, n))] = 1.0
        graphs.append(SimpleNamespace(x=x, edge_index=(ei[:, int(estart[g]):int(estart[g + 1])] - start[g]).contiguous(),
                                      y=torch.tensor([[float(rng.randint(2))]]), edge_attr=None, edge_label=None))
    return graphs, 14


def build(graphs, x_dim, dev, capturable):
    import dp_gsat_amd as G
    torch.manual_seed(0)
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=HIDDEN, dropout_p=0.3, use_edge_attr=False, deg=deg)
    clf = G.get_model(x_dim, 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(HIDDEN, True).to(dev)
    params = list(clf.parameters()) + list(ext.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-6, **(dict(capturable=True, fused=True) if capturable else {}))
    return G.GSAT(clf, ext, G.Criterion(2, False), opt, learn_edge_att=True).train()


POOL = 512


def id_pool(num_graphs, seed):
    """The full batches of successive random permutations, POOL of them: the timed windows cycle through this list."""
    gen = np.random.RandomState(seed)
    pool = []
    while len(pool) < POOL:
        perm = gen.permutation(num_graphs)
        pool += [perm[s:s + BATCH] for s in range(0, num_graphs - BATCH + 1, BATCH)]
    return pool[:POOL]


def cycle(pool):
    while True:
        yield from pool


def window(step, ids, seconds):
    """ms/step of a window of at least ``seconds`` that ends in a synchronise, and the id sets it used."""
    used = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while True:
        for _ in range(20):
            used.append(next(ids))
            step(used[-1])
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(used), used


def measure(name, graphs, x_dim, dev, seconds, rounds, tight):
    """``tight``: the capacity is the largest (N + 2, E) among the pool's batches (vetted by ReplayedStep.check_epoch) instead of
    PackedDataset.capacity_for(BATCH), the bound over every possible batch."""
    import dp_gsat_amd as G
    ds = G.PackedDataset.from_data_list(graphs, dev)
    eager, captured = build(graphs, x_dim, dev, False), build(graphs, x_dim, dev, True)
    pool = id_pool(len(graphs), 1)
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    capacity = (max(int(n_all[u].sum()) for u in pool) + 2, max(int(e_all[u].sum()) for u in pool)) if tight else None
    replayed = G.ReplayedStep(captured, ds, BATCH, capacity=capacity)
    replayed.check_epoch(np.concatenate(pool))

    def eager_step(ids):
        b = ds.collate(torch.as_tensor(ids, device=dev))
        _, loss, ld, _ = eager.forward_pass(b, 0, True)
        eager.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        eager.optimizer.step()
        return ld["loss"]

    def replayed_step(ids):
        return replayed.step(ids, 0)

    ids = cycle(pool)
    for _ in range(30):                                    # warm both modes
        eager_step(next(ids))
        replayed_step(next(ids))
    times = {"eager": [], "replayed": []}
    real_n, real_e = [], []
    for _ in range(rounds):
        for mode, fn in (("eager", eager_step), ("replayed", replayed_step)):
            ms, used = window(fn, ids, seconds)
            times[mode].append(ms)
            real_n += [int(n_all[u].sum()) for u in used]
            real_e += [int(e_all[u].sum()) for u in used]
    N_cap, E_cap = replayed.capacity
    assert int(replayed.batch.valid[3]) == 0, "a timed batch did not fit the capacity"
    out = dict(shape=name, graphs=len(graphs), batch=BATCH, hidden=HIDDEN, capacity_rule="pool maximum" if tight else "capacity_for",
               capacity=dict(nodes=N_cap, edges=E_cap),
               mean_real=dict(nodes=float(np.mean(real_n)), edges=float(np.mean(real_e))),
               padding_share=dict(nodes=(N_cap - float(np.mean(real_n))) / N_cap, edges=(E_cap - float(np.mean(real_e))) / E_cap))
    for mode, t in times.items():
        out[mode] = dict(ms_per_step_median=statistics.median(t), ms_per_step_min=min(t), ms_per_step_max=max(t), windows=t)
    out["replayed_over_eager"] = out["replayed"]["ms_per_step_median"] / out["eager"]["ms_per_step_median"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "padded_replay_report.json"))
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
        print(json.dumps({k: res[k] for k in ("shape", "capacity", "padding_share", "replayed_over_eager")}), flush=True)
        print(f"  eager {res['eager']['ms_per_step_median']:.3f} ms/step  replayed {res['replayed']['ms_per_step_median']:.3f} ms/step", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
