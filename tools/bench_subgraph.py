#!/usr/bin/env python3
"""Times the explanation-subgraph extraction of dp_gsat_amd.subgraph at the C3 (molhiv, 2048 graphs) and C2 (ba2motifs, 512 graphs)
batch shapes, ratio = 0.5, and writes profiles/subgraph_report.json:

  (a) explanation_subgraph(att, data, ratio=0.5)          top-k mask + extraction + attribute gathers (one host read of the sizes)
  (b) edge_subgraph(data, mask)                           the bare extraction on a ready mask (one host read of the sizes)
  (c) edge_subgraph(data, mask, sizes=...)                the same without the host read (the capturable form)
  (e) replay of (c) captured into a graph                 the extraction and its gathers alone ((b) and (c) also build the batch
                                                          index of the result, which the model forward that follows would build)
  (d) torch baseline on the device                        the PyG recipe restated with torch ops: nonzero, index_select, a cumsum
                                                          relabel and one index_select per attribute (one host read inside nonzero)

Median of 20 event-timed runs after 5 warm-up runs, one process.  The launch count of (c) is read from a captured graph's dump.
The baseline lives here, not in the package: the package has no torch fallback.

  python tools/bench_subgraph.py [--out profiles/subgraph_report.json]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

RATIO = 0.5


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


def torch_edge_subgraph(d, mask):
    """Device-side torch restatement of the PyG recipe (edge mask, isolated nodes dropped, nodes relabelled)."""
    N = d.x.shape[0]
    edge_id = mask.nonzero().view(-1)
    ei = d.edge_index.index_select(1, edge_id)
    node_mask = torch.zeros(N, dtype=torch.bool, device=mask.device)
    node_mask[ei.view(-1)] = True
    node_id = node_mask.nonzero().view(-1)
    relabel = node_mask.cumsum(0) - 1
    out = {"edge_index": relabel[ei], "x": d.x.index_select(0, node_id), "batch": d.batch.index_select(0, node_id),
           "node_id": node_id, "edge_id": edge_id}
    if d.get("edge_attr") is not None:
        out["edge_attr"] = d.edge_attr.index_select(0, edge_id)
    return out


def capture(fn):
    """(graph of one captured call, its kernel nodes or None when this build cannot dump the graph)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    try:
        graph.enable_debug_mode()
    except Exception:
        pass
    with torch.cuda.graph(graph):
        fn()
    try:
        path = os.path.join(tempfile.mkdtemp(), "graph.dot")
        graph.debug_dump(path)
        text = open(path, errors="replace").read()
    except Exception:
        return graph, None
    names = set()
    for line in text.splitlines():
        m = re.match(r'^\s*"?([\w.]+)"?\s*\[', line)
        if m and "->" not in line and m.group(1) not in ("node", "edge", "graph"):
            names.add(m.group(1))
    return graph, len(names) or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgraph_report.json"))
    args = ap.parse_args()
    import dp_gsat_amd as G
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(0), "ratio": RATIO, "runs": 20, "warmup": 5, "unit": "ms (median)", "shapes": {}}
    for name, b in batches().items():
        d = b.to(dev)
        att = torch.from_numpy(np.random.RandomState(1).rand(b.num_edges).astype(np.float32)).to(dev)
        seg = G.get_index(d.edge_index, d.num_nodes).graphs(d.batch, b.num_graphs)
        seg.edge_segments, seg.max_edges_per_graph            # per-batch bookkeeping: cached, outside the timed region for every variant
        mask = G.topk_edge_mask(att, d.edge_index, d.batch, ratio=RATIO, num_graphs=b.num_graphs)
        sub = G.edge_subgraph(d, mask)
        ref = torch_edge_subgraph(d, mask)
        for key in ("edge_index", "x", "batch", "node_id", "edge_id"):
            assert torch.equal(getattr(sub, key), ref[key]), key           # the baseline computes the same thing
        sizes = (sub.num_nodes, sub.num_edges)
        row = {"graphs": b.num_graphs, "nodes": b.num_nodes, "edges": b.num_edges, "kept_nodes": sizes[0], "kept_edges": sizes[1],
               "explanation_subgraph": median_ms(lambda: G.explanation_subgraph(att, d, ratio=RATIO)),
               "edge_subgraph": median_ms(lambda: G.edge_subgraph(d, mask)),
               "edge_subgraph_sizes_given": median_ms(lambda: G.edge_subgraph(d, mask, sizes=sizes)),
               "torch_baseline": median_ms(lambda: torch_edge_subgraph(d, mask))}
        # (b) and (c) also build the batch index of the result (edge_subgraph primes it for the model forward that follows); a replay
        # of the captured call is the extraction and its gathers alone
        graph, row["launches_sizes_given"] = capture(lambda: G.edge_subgraph(d, mask, sizes=sizes))
        row["edge_subgraph_graph_replay"] = median_ms(graph.replay)
        row["hip_faster_than_torch"] = row["edge_subgraph"] < row["torch_baseline"]
        report["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        G.clear_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
