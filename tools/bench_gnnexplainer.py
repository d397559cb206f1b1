#!/usr/bin/env python3
"""Times the batched GNNExplainer and writes profiles/gnnexplainer_report.json.

  (a) step, kernel   -- the captured optimisation step of ReplayedGNNExplainer as built: masked forward, criterion, backward to the mask,
                        gsat_mask_step (one elementwise launch and one single-thread launch).  A timed call is what a batch costs: one
                        replay of the begin graph, then ``--steps`` replays of the step, so the mask stays in the regime an explanation
                        visits; reported per step (the begin replay is inside the figure, for both);
  (b) step, torch    -- the same captured step with the mask update restated in torch: ``sigmoid``, the size and entropy terms and the
                        chain through the sigmoid by autograd, ``torch.optim.Adam(capturable=True, fused=True)`` on the mask logits.
                        It lives in this tool only; the library has no such switch.  The kernel-node counts of both graphs are reported;
  (c) epoch          -- one ``ReplayedGNNExplainer.run`` epoch (``--steps`` optimisation steps per batch) against one ``ReplayedEval.run``
                        epoch of a GSAT model with the same backbone over the same graphs.
Ragged budget batches of at most 128 graphs at a capacity near the mean batch; both steps run on the first budget batch.  Method of
tools/bench_padded.py: everything is warmed, then ``--rounds`` rounds of one window each, alternating in one process, every window
whole calls for at least ``--window`` seconds and ending in a synchronise.  Reported: the median of the windows, their min / max and
the ratios of the medians.

Shapes: tools/bench_padded.py's (800 BA-2motifs graphs; the 4337 Mutagenicity topologies of tests/golden/mutag_full.npz), GIN, H 64.

  python tools/bench_gnnexplainer.py [--out profiles/gnnexplainer_report.json] [--window 1.0] [--rounds 5] [--steps 100]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from bench_fidelity_curve import kernel_nodes
from bench_padded import BATCH, HIDDEN, build, example_graphs, mutag_graphs
from bench_ragged_replay import summary, timed

LOG_EPS = 1e-15


def debug_graph():
    """A CUDAGraph that keeps its hipGraph for ``debug_dump`` where torch can (``keep_graph``), with debug mode on."""
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        graph = torch.cuda.CUDAGraph()
    try:
        graph.enable_debug_mode()
    except Exception:
        pass
    return graph


def torch_step_graph(rs, dev):
    """The step of ``rs`` with the mask update in torch, captured on the batch the begin graph left behind.  Returns (graph, mask logits, reset)."""
    import dp_gsat_amd as G
    from dp_gsat_amd.baselines import _forward, _frozen, _real_rows
    ex, ctx = rs.explainer, rs._ctx
    data, E = ctx["data"], rs.mask.E
    m = torch.zeros(E, device=dev, requires_grad=True)
    opt = torch.optim.Adam([m], lr=ex.lr, betas=ex.betas, eps=ex.eps, capturable=True, fused=True)
    real = (torch.arange(E, device=dev) < ctx["valid"][1]).to(torch.float32)           # the real edge slots, on the device
    inv_eg = rs.mask.inv_eg

    def body():
        a = torch.sigmoid(m)
        logits = _forward(ex.clf, data, a.view(E, 1))
        z, t = _real_rows(data, logits), _real_rows(data, ctx["targets"])
        pred = ex.criterion(z, t, g_valid=ctx["g_valid"]) * ctx["count"].reshape(())
        H = -a * torch.log(a + LOG_EPS) - (1 - a) * torch.log(1 - a + LOG_EPS)
        loss = pred + ((ex.size_coef * a + ex.ent_coef * H * inv_eg) * real).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    graph = debug_graph()
    was = G.graph_index.sync_free()
    G.set_sync_free(True)
    try:
        with _frozen(ex.clf):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    body()
            torch.cuda.current_stream().wait_stream(side)
            with torch.cuda.graph(graph):
                body()
    finally:
        G.set_sync_free(was)

    def reset():
        """Mask logits and Adam state back to the start of an explanation."""
        with torch.no_grad():
            m.zero_()
            for v in opt.state[m].values():
                if isinstance(v, torch.Tensor):
                    v.zero_()

    return graph, m, reset


def measure(name, graphs, x_dim, dev, seconds, rounds, steps):
    import dp_gsat_amd as G
    for g in graphs:
        if getattr(g, "edge_label", None) is None:
            g.edge_label = torch.zeros(g.edge_index.shape[1])         # the reference zero-fills missing edge labels
    ds = G.PackedDataset.from_data_list(graphs, dev)
    n_all, e_all = ds.node_counts.cpu().numpy(), ds.edge_counts.cpu().numpy()
    perm = np.random.RandomState(1).permutation(len(graphs))
    capacity = (max(int(np.ceil(n_all.mean() * BATCH)), int(n_all.max())) + 2, max(int(np.ceil(e_all.mean() * BATCH)), int(e_all.max())))
    gsat = build(graphs, x_dim, dev, True)
    triple = tuple(debug_graph() for _ in range(3))
    rs = G.ReplayedGNNExplainer(gsat.clf, gsat.criterion, ds, BATCH, 5, steps=steps, capacity=capacity, ragged=True, graphs=triple)
    ev = G.ReplayedEval(gsat, ds, BATCH, 5, capacity=capacity, ragged=True)
    rows = rs.batches(perm)
    rs._load_ids(rows[0])
    rs.graphs["begin"].replay()                                       # the batch both steps run on
    torch_graph, m_torch, reset_torch = torch_step_graph(rs, dev)
    # one step of each from the same start must agree: the restatement is the same arithmetic
    rs.graphs["begin"].replay()
    rs.graphs["step"].replay()
    reset_torch()
    torch_graph.replay()
    E_real = int(rs._ctx["valid"][1])
    agree = float((rs.mask.m[:E_real] - m_torch.detach()[:E_real]).abs().max())

    def steps_kernel():
        rs._load_ids(rows[0])
        rs.graphs["begin"].replay()
        for _ in range(steps):
            rs.graphs["step"].replay()

    def steps_torch():
        rs._load_ids(rows[0])
        rs.graphs["begin"].replay()
        reset_torch()
        for _ in range(steps):
            torch_graph.replay()

    runs = {"step_kernel": steps_kernel, "step_torch": steps_torch,
            "explain_epoch": lambda: rs.run(perm), "eval_epoch": lambda: ev.run(perm, 0)}
    for _ in range(2):
        for fn in runs.values():
            fn()
    times = {key: [] for key in runs}
    for _ in range(rounds):
        for key, fn in runs.items():
            times[key].append(timed(fn, seconds))
    for key in ("step_kernel", "step_torch"):
        times[key] = [t / steps for t in times[key]]
    ms = {key: summary(t) for key, t in times.items()}
    out = dict(shape=name, graphs=len(graphs), slots=BATCH, hidden=HIDDEN, steps=steps, capacity=dict(nodes=capacity[0], edges=capacity[1]),
               batches_per_epoch=int(rows.shape[0]), first_batch_real_edges=E_real, one_step_max_abs_difference=agree,
               kernel_nodes=dict(begin=kernel_nodes(triple[0]), step_kernel=kernel_nodes(triple[1]), end=kernel_nodes(triple[2]),
                                 step_torch=kernel_nodes(torch_graph)),
               ms_per_step={k: ms[k] for k in ("step_kernel", "step_torch")}, ms_per_epoch={k: ms[k] for k in ("explain_epoch", "eval_epoch")})
    out["torch_over_kernel_step"] = ms["step_torch"]["median"] / ms["step_kernel"]["median"]
    out["explain_over_eval_epoch"] = ms["explain_epoch"]["median"] / ms["eval_epoch"]["median"]
    G.clear_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnnexplainer_report.json"))
    ap.add_argument("--window", type=float, default=1.0, help="least length of a timed window, seconds")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100, help="optimisation steps per batch")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    report = dict(device=torch.cuda.get_device_name(0), window_seconds=args.window, rounds=args.rounds, shapes=[])
    for name, make in (("ba2motifs_example", example_graphs), ("mutag", mutag_graphs)):
        graphs, x_dim = make()
        res = measure(name, graphs, x_dim, dev, args.window, args.rounds, args.steps)
        report["shapes"].append(res)
        s, e = res["ms_per_step"], res["ms_per_epoch"]
        print(f"{name}: step kernel {s['step_kernel']['median']:.4f} ms ({res['kernel_nodes']['step_kernel']} nodes)  torch "
              f"{s['step_torch']['median']:.4f} ms ({res['kernel_nodes']['step_torch']} nodes)  torch / kernel {res['torch_over_kernel_step']:.3f}  "
              f"one-step difference {res['one_step_max_abs_difference']:.2e}", flush=True)
        print(f"{name}: explain epoch {e['explain_epoch']['median']:.1f} ms  eval epoch {e['eval_epoch']['median']:.2f} ms  "
              f"ratio {res['explain_over_eval_epoch']:.1f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
