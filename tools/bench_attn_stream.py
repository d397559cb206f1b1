#!/usr/bin/env python3
"""Times forward + backward of the edge-attention extractor two ways and writes profiles/attn_stream_report.json:

  staged   -- ExtractorMLP with stream_rows = None: the default paths, which save a1 [E, 4H] and take da1 [E, 4H] from the backward's
              workspace (this is what the comparison is against; nothing here changes it);
  streamed -- the same module with stream_rows set: a1 and da1 exist for one group of whole graphs at a time and the backward computes
              a1 again (ops.StreamedExtractorAttention, gsat_attn_stream_fwd / gsat_attn_stream_bwd).

Workloads: "c5_slice" = 16 power-law graphs of ~98 k directed edges (1/8 of C5's share of one GPU), H = 256, stream_rows = the largest
graph, so every graph is a group; "c4" = C4's batch, 1024 SPMotif-shaped graphs, H = 128, stream_rows = an eighth of the edges.  The
embedding is random: only the extractor runs.  Dropout masks and the sampler's noise are drawn in the kernels from one seed, so both modes
take the same keep decisions; their outputs are compared before anything is timed.  For each workload the two modes alternate in one
process: both are warmed, then 5 rounds of one staged and one streamed window, each of whole calls, at least 1 s long and ending in a
synchronise.  Reported per mode: the median ms/call of the 5 windows, their min / max, and the peak of torch.cuda.max_memory_allocated
over one call above the level before it.  The streamed backward pays one extra a1 recompute; no ratio is expected in advance, and none
is asserted.

  python tools/bench_attn_stream.py [--out profiles/attn_stream_report.json] [--window 1.0] [--rounds 5] [--only c4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def window(fn, seconds):
    """ms/call of a window of whole calls, at least ``seconds`` long, ending in a synchronise."""
    n = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def workloads(only):
    from dp_gsat_amd import synth
    out = {}
    if only in (None, "c5_slice"):
        b = synth.powerlaw_batch(num_nodes=156_250, num_edges=1_562_500, num_graphs=16, seed=0)
        out["c5_slice"] = (b, 256, "largest graph")
    if only in (None, "c4"):
        out["c4"] = (synth.spmotif_batch(1024, seed=0), 128, "edges / 8")
    return out


def measure(name, batch, H, rule, dev, seconds, rounds):
    import dp_gsat_amd as G
    torch.manual_seed(0)
    ei, bvec = batch.edge_index.to(dev), batch.batch.to(dev)
    N, E, graphs = int(batch.x.shape[0]), int(ei.shape[1]), int(batch.num_graphs)
    per_graph = torch.bincount(bvec[ei[0]], minlength=graphs)
    rows = int(per_graph.max()) if rule == "largest graph" else max(E // 8, int(per_graph.max()))
    ext = G.ExtractorMLP(H, True).to(dev).train()
    emb = torch.randn(N, H, device=dev)
    gz, ga = torch.randn(E, 1, device=dev), torch.randn(E, 1, device=dev)
    G.get_index(ei, N).graphs(bvec, graphs)

    def call(stream_rows, keep=False):
        ext.stream_rows = stream_rows
        ext.zero_grad(set_to_none=True)
        e = emb.clone().requires_grad_(True)
        z, a = ext.attend(e, ei, bvec, noise="philox", seed=11)
        torch.autograd.backward([z, a], [gz, ga])
        return (a.detach().clone(), e.grad.clone(), ext.mlp.linears()[1].weight.grad.clone()) if keep else None

    def peak(stream_rows):
        call(stream_rows)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        call(stream_rows)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    ref, got = call(None, True), call(rows, True)
    gaps = {k: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for k, a, b in zip(("att", "demb", "dW2"), got, ref)}
    del ref, got
    plan = G.get_index(ei, N).graphs(bvec, graphs).stream_plan(rows)
    modes = {"staged": None, "streamed": rows}
    peaks = {m: peak(r) for m, r in modes.items()}
    times = {m: [] for m in modes}
    for _ in range(rounds):
        for m, r in modes.items():
            times[m].append(window(lambda: call(r), seconds))
    rep = dict(workload=name, nodes=N, edges=E, graphs=graphs, H=H, stream_rows=rows, rule=rule, groups=plan.n_groups,
               scratch_rows=plan.scratch_rows, activation_bytes=E * 4 * H * 4, streamed_vs_staged_max_rel_gap=gaps)
    for m in modes:
        rep[m] = dict(ms_per_call_median=statistics.median(times[m]), ms_per_call_min=min(times[m]), ms_per_call_max=max(times[m]),
                      peak_bytes_above_start=int(peaks[m]))
    print(json.dumps(rep), flush=True)
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_stream_report.json"))
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["c5_slice", "c4"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    reps = [measure(name, b, H, rule, dev, args.window, args.rounds) for name, (b, H, rule) in workloads(args.only).items()]
    report = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, window_seconds=args.window, rounds=args.rounds,
                  method="forward + backward of ExtractorMLP.attend, staged and streamed windows alternating in one process", workloads=reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
