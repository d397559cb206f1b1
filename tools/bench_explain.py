#!/usr/bin/env python3
"""Times the per-graph edge ranking of dp_gsat_amd.explain at the C3 (molhiv, 2048 graphs) and C2 (ba2motifs, 512 graphs) batch
shapes and writes profiles/explain_metrics.md:

  (a) gsat_rank_edges, fused path (order, rank, topk, hits in one launch)
  (b) gsat_rank_edges, general path (radix sort + two launches)
  (c) two stable torch.sort calls giving the same order -- what a user can write without this module (order only)
  (d) the reference's per-graph loop (src/run_gsat.py:783-791) restated on device tensors, at a reduced graph count

Median of 20 event-timed runs after 5 warm-up runs, one process, nothing else on the device.  Launch counts come from
`rocprofv3 --kernel-trace` runs of this script in --trace mode (a child process each): kernel rows with N calls minus rows with none.

  python tools/bench_explain.py            # everything, writes the report
  python tools/bench_explain.py --no-trace # timings only
"""
import argparse
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

K = 5
LOOP_GRAPHS = 64
TRACE_CALLS = 10


def batches():
    from dp_gsat_amd import synth
    return {"C3": synth.molhiv_batch(2048, seed=0), "C2": synth.ba2motifs_batch(num_graphs=512, seed=0)}


def median_ms(fn, runs=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def setup(b, dev):
    import dp_gsat_amd as G
    d = b.to(dev)
    rng = np.random.RandomState(1)
    att = torch.from_numpy(rng.rand(b.num_edges).astype(np.float32)).to(dev)
    lab = torch.from_numpy((rng.rand(b.num_edges) < 0.25).astype(np.uint8)).to(dev)
    seg = G.get_index(d.edge_index, d.num_nodes).graphs(d.batch, b.num_graphs)
    seg.edge_segments, seg.max_edges_per_graph            # per-batch bookkeeping: cached, outside the timed region for every variant
    return d, att, lab, seg


def rank_call(d, att, lab, G_, path):
    from dp_gsat_amd import explain as X
    return lambda: X._rank(att, d.edge_index, d.batch, G_, path, k=K, label=lab, want=("order", "rank", "topk", "hits"))


def torch_two_sorts(att, eg):
    def fn():
        i1 = torch.sort(-att, stable=True).indices
        i2 = torch.sort(eg[i1], stable=True).indices
        return i1[i2]
    return fn


def reference_loop(att, lab, batch, edge_index, graphs):
    def fn():
        out = []
        for i in range(graphs):
            nodes = batch == i
            edges = nodes[edge_index[0]] & nodes[edge_index[1]]
            top = torch.argsort(-att[edges], stable=True)[:K]
            out.append(lab[edges][top].sum().item() / K)
        return out
    return fn


def trace_child(path, calls):
    dev = torch.device("cuda:0")
    b = batches()["C3"]
    d, att, lab, _ = setup(b, dev)
    fn = rank_call(d, att, lab, b.num_graphs, path)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()


def kernel_rows(path, calls):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--trace", path, "--calls", str(calls)]
        subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            return None
        return sum(max(sum(1 for _ in open(f)) - 1, 0) for f in files)


def resources():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(ROOT, "dp_gsat_amd", "csrc", "explain.hip")],
                         capture_output=True, text=True).stdout
    return [l.rstrip() for l in out.splitlines() if "gsat::k_" in l]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default=None, help="(child mode) run `--calls` ranking calls on this path at C3 and exit")
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_metrics.md"))
    args = ap.parse_args()
    if args.trace:
        trace_child(args.trace, args.calls)
        return
    dev = torch.device("cuda:0")
    lines = ["# Explanation metrics: per-graph edge ranking on the device", "",
             f"`tools/bench_explain.py` on {torch.cuda.get_device_name(0)}: median of 20 event-timed runs after 5 warm-up runs, k = {K}.", "",
             "| shape | graphs | edges | max edges/graph | (a) fused ms | (b) general ms | (c) 2x torch.sort ms | (c)/(a) | (b)/(a) | "
             f"(d) reference loop on {LOOP_GRAPHS} graphs ms |", "|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for name, b in batches().items():
        d, att, lab, seg = setup(b, dev)
        eg = seg.edge_segments[2]
        ta = median_ms(rank_call(d, att, lab, b.num_graphs, "fused"))
        tb = median_ms(rank_call(d, att, lab, b.num_graphs, "general"))
        tc = median_ms(torch_two_sorts(att, eg))
        td = median_ms(reference_loop(att, lab, d.batch, d.edge_index, LOOP_GRAPHS), runs=5, warmup=1)
        lines.append(f"| {name} | {b.num_graphs} | {b.num_edges} | {seg.max_edges_per_graph} | {ta:.4f} | {tb:.4f} | {tc:.4f} | {tc / ta:.2f} | "
                     f"{tb / ta:.2f} | {td:.2f} |")
        ok = ok and ta <= tb and (name != "C3" or ta < tc)
        print(lines[-1], flush=True)
    lines += ["", "(c) produces `order` only; (a) and (b) also produce rank, topk and hits.  (d) is the loop of src/run_gsat.py:783-791 on device "
              f"tensors for the first {LOOP_GRAPHS} graphs of the batch only (its cost is linear in the graph count), recorded for context.",
              "", f"Performance condition (fused beats (c) at C3, fused not slower than general at C3 and C2): {'MET' if ok else 'NOT MET'}.", ""]
    if not args.no_trace:
        base = kernel_rows("fused", 0)
        lines += ["## Launches per ranking call (rocprofv3 --kernel-trace, C3)", ""]
        for path in ("fused", "general"):
            rows = kernel_rows(path, TRACE_CALLS)
            per = "n/a" if rows is None or base is None else f"{(rows - base) / TRACE_CALLS:.1f}"
            lines.append(f"- {path}: {per} kernel launches per call ({rows} kernel rows with {TRACE_CALLS} calls, {base} with none)")
            print(lines[-1], flush=True)
        lines.append("")
    lines += ["## Kernel resources (tools/kernel_resources.py dp_gsat_amd/csrc/explain.hip)", "", "```"] + resources() + ["```", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
