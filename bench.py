#!/usr/bin/env python3
"""bench.py -- million directed edges/s through the GSAT hot path on MI355X.

  python bench.py --gpus 1 --steps 20 --warmup 5            # default workload: C3 (molhiv-shaped, PNA H=128, batch 2048)
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

One *step* (scope A) = [per-batch edge bookkeeping -> extractor MLP fwd -> concrete sample ->
symmetrise | lift -> L masked aggregations fwd] + the backward of all of it (+ the flat RCCL gradient all-reduce
when N > 1), on one synthetic collated batch resident in HBM.  `value` = directed edges of all ranks / step time.
A plain run times that step and nothing else.  With `--full` it also re-times the step on exact fp32 products
(`value_fp32_exact`), times the full GSAT training step (both backbone passes, dense node updates, losses, Adam) as
`full_step`, times the CPU oracle on the host cores as `cpu_baseline`, and prices the masked aggregation kernels
against HBM bandwidth as `roofline`; without `--full` those fields are null.

  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR   # + what the last timed step computed, as DIR/<name>.npy
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md); measured copy ~6.3 TB/s

WORKLOADS = {
    # name: backbone, conv, attention mode, hidden, layers, graphs per GPU
    "c1": dict(desc="C1 MUTAG-shaped (real topology fixture) + GIN H=64 L=2, node attention, 128 graphs", backbone="GIN", H=64, L=2, edge_att=False, graphs=128),
    "c2": dict(desc="C2 ba_2motifs-shaped + GIN H=64 L=2, edge attention (symmetrised), 512 graphs", backbone="GIN", H=64, L=2, edge_att=True, graphs=512),
    "c3": dict(desc="C3 ogbg-molhiv-shaped + PNA H=128 L=4 (mean,min,max,std; identity), node attention, 2048 graphs", backbone="PNA", H=128, L=4, edge_att=False, graphs=2048),
    "c4": dict(desc="C4 spmotif-shaped + GIN/GINEConv H=128 L=2, edge attention (directed, no symmetrisation), 1024 graphs/GPU", backbone="GIN", H=128, L=2, edge_att=True, graphs=1024),
    "c5": dict(desc="C5 power-law Chung-Lu, the full per-GPU share of the 8-GPU config: 1.25M nodes, 12.5M directed edges, 128 graphs + GIN H=256 L=2, edge attention", backbone="GIN", H=256, L=2, edge_att=True, graphs=128),
    "c5s": dict(desc="C5 power-law Chung-Lu (scaled 1/64 of the per-GPU share: 19.5k nodes, 195k edges x2, 2 graphs) + GIN H=256 L=2, edge attention", backbone="GIN", H=256, L=2, edge_att=True, graphs=2),
}
PNA_AGGR = ["mean", "min", "max", "std"]


def make_batch(name, num_graphs, seed):
    from dp_gsat_amd import synth
    if name == "c1":
        return synth.mutag_batch(os.path.join(ROOT, "tests", "golden", "mutag128.npz"), min(num_graphs, 128)), 14, 0
    if name == "c2":
        return synth.ba2motifs_batch(num_graphs, seed), 10, 0
    if name == "c3":
        return synth.molhiv_batch(num_graphs, seed), 9, 0
    if name == "c4":
        return synth.spmotif_batch(num_graphs, seed), 4, 1
    if name == "c5":
        return synth.powerlaw_batch(num_nodes=9766 * num_graphs, num_edges=97_656 * num_graphs, num_graphs=num_graphs, seed=seed), 16, 0
    if name == "c5s":
        return synth.powerlaw_batch(num_nodes=19_532 * num_graphs // 2, num_edges=195_312 * num_graphs, num_graphs=num_graphs, seed=seed), 16, 0
    raise ValueError(name)


def local_shard(name, graphs_per_gpu, rank, world, seed):
    """Weak scaling: the global batch has graphs_per_gpu * world graphs; whole graphs go to ranks by the
    edge-balanced LPT partition (no data-path collective)."""
    from dp_gsat_amd.dist import edges_per_graph, shard_graphs_lpt, take_graphs
    if name in ("c5", "c5s") and world > 1:
        # every graph of the power-law workload has the same node and edge count by construction, so the edge-balanced partition
        # is graphs_per_gpu graphs per rank whichever way it is cut: generate ONLY this rank's graphs (its own seed) instead of
        # building the 10 M-node / 100 M-edge global batch on every rank
        return make_batch(name, graphs_per_gpu, seed * 1000 + rank)
    batch, x_dim, e_dim = make_batch(name, graphs_per_gpu * world, seed)
    if world > 1:
        parts = shard_graphs_lpt(edges_per_graph(batch), world)
        batch = take_graphs(batch, parts[rank])
    return batch, x_dim, e_dim


# ------------------------------------------------------------------------------------------------
# scope A: the hot path proper
# ------------------------------------------------------------------------------------------------
class HotPath:
    def __init__(self, wl, data, dev, seed=0):
        import dp_gsat_amd as G
        from dp_gsat_amd import synth
        self.G, self.wl, self.dev, self.data = G, wl, dev, data
        g = torch.Generator().manual_seed(seed)
        N, E, H, L = data.num_nodes, data.num_edges, wl["H"], wl["L"]
        self.N, self.E = N, E
        self.ext = G.ExtractorMLP(H, wl["edge_att"]).to(dev).train()
        self.emb = torch.randn(N, H, generator=g).to(dev).requires_grad_(True)
        self.xs = [torch.randn(N, H, generator=g).to(dev).requires_grad_(True) for _ in range(L)]
        self.gine = data.edge_attr is not None
        self.edge_emb = [torch.randn(E, H, generator=g).to(dev).requires_grad_(True) for _ in range(L)] if self.gine else None
        if wl["backbone"] == "PNA":
            self.avg_deg = {"lin": 1.0, "log": 1.0}
            width = len(PNA_AGGR) * 2 * H
        else:
            width = H
        self.gouts = [torch.randn(N, width, generator=g).to(dev) for _ in range(L)]
        self.flat = None
        self.reuse_index = False
        self.keep_outputs = False      # --dump-outputs: hold the forward results of the latest step (in a captured step: the graph's buffers)
        self.last = None

    def attach_dp(self):
        from dp_gsat_amd.dist import FlatGradAllReduce
        self.flat = FlatGradAllReduce(self.ext.parameters())

    def outputs(self):
        """What a caller of the step receives, by name: the forward results of the latest step and the gradients its backward left."""
        out = dict(self.last)
        out["grad_emb"] = self.emb.grad
        for l, t in enumerate(self.xs):
            out[f"grad_x_l{l}"] = t.grad
        for l, t in enumerate(self.edge_emb or []):
            out[f"grad_edge_emb_l{l}"] = t.grad
        for n, p in self.ext.named_parameters():
            out["grad_ext." + n] = p.grad
        return {k: v for k, v in out.items() if v is not None}

    def step(self):
        self.compute()
        self.reduce()

    def reduce(self):
        """The one collective of the step (N > 1): flat gradient all-reduce, enqueued behind the last backward kernel."""
        if self.flat is not None:
            self.flat.all_reduce(average=True, async_op=True)
            self.flat.wait()

    def compute(self):
        """Everything of the step but the collective (this part is what a hipGraph captures, also for N > 1: the gradients land in the
        flat buffer at fixed addresses)."""
        G, d, wl = self.G, self.data, self.wl
        if not self.reuse_index:
            G.clear_cache()                       # every step is a NEW batch: re-derive CSRs / reverse perm / segments
        if self.flat is not None:
            self.flat.zero()
        else:
            for p in self.ext.parameters():
                p.grad = None
        self.emb.grad = None
        for t in self.xs + (self.edge_emb or []):      # zero_grad(set_to_none=True): no accumulate-into-old-gradient adds
            t.grad = None
        index = G.get_index(d.edge_index, self.N)
        index.graphs(d.batch, d.num_graphs)
        logits, att = self.ext.attend(self.emb, d.edge_index, d.batch, noise="philox")      # concrete-sample noise drawn in the head kernel
        edge_att = G.symmetrise_edge_att(att, d.edge_index, self.N) if wl["edge_att"] else G.lift_node_att_to_edge_att(att, d.edge_index)
        outs = []
        for l in range(wl["L"]):
            if wl["backbone"] == "PNA":
                outs.append(G.ops.pna_aggregate(self.xs[l], index, edge_att, None, PNA_AGGR, ["identity"], self.avg_deg))
            else:
                outs.append(G.ops.masked_sum_aggregate(self.xs[l], index, edge_att, self.edge_emb[l] if self.gine else None))
        torch.autograd.backward(outs, self.gouts)
        if self.keep_outputs:
            self.last = dict(att_log_logits=logits.detach(), att=att.detach(), **{f"out_l{l}": o.detach() for l, o in enumerate(outs)})
            if isinstance(edge_att, torch.Tensor):      # node attention stays a lazy view (LiftedAttention) of `att`: nothing more to keep
                self.last["edge_att"] = edge_att.detach()


class FullStep:
    """Whole GSAT training step (example/trainer.py:28-36): forward_pass, zero_grad, backward, Adam."""

    def __init__(self, wl, data, x_dim, e_dim, dev, capturable=False):
        import dp_gsat_amd as G
        from dp_gsat_amd import synth
        self.G, self.data = G, data
        H = wl["H"]
        cfg = dict(model_name=wl["backbone"], n_layers=wl["L"], hidden_size=H, dropout_p=0.3, use_edge_attr=e_dim != 0,
                   atom_encoder=data.x.dtype == torch.int64, aggregators=PNA_AGGR, scalers=False, deg=synth.in_degree_histogram(data))
        num_class = 2 if data.y.dtype == torch.float32 else 3
        self.clf = G.get_model(x_dim, e_dim, num_class, False, cfg, dev)
        self.ext = G.ExtractorMLP(H, wl["edge_att"]).to(dev)
        params = list(self.clf.parameters()) + list(self.ext.parameters())
        # the reference's optimizer (torch.optim.Adam, example/trainer.py); its fused implementation is one multi-tensor kernel per step -- the
        # default "foreach" one with capturable=True adds ~70 microsecond-sized launches per step to a captured graph (GSAT_ADAM_FUSED=0)
        try:
            if os.environ.get("GSAT_ADAM_FUSED", "1") == "0":
                raise RuntimeError("fused Adam switched off")
            self.opt = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-6, capturable=capturable, fused=True)
            self.adam = "fused"
        except (RuntimeError, ValueError, TypeError):
            self.opt = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-6, capturable=capturable)
            self.adam = "foreach"
        self.gsat = G.GSAT(self.clf, self.ext, G.Criterion(num_class, False), self.opt, learn_edge_att=wl["edge_att"]).train()
        self.gsat.sync_loss_dict = False
        self.flat = None
        self.params = params

    def attach_dp(self):
        from dp_gsat_amd.dist import FlatGradAllReduce
        self.flat = FlatGradAllReduce(self.params)

    def step(self):
        self.G.clear_cache()
        att, loss, _, _ = self.gsat.forward_pass(self.data, 0, True)
        if self.flat is not None:
            self.flat.zero()
        else:
            self.opt.zero_grad(set_to_none=True)
        loss.backward()
        if self.flat is not None:
            self.flat.all_reduce(average=True, async_op=True)     # enqueued behind the last backward kernel, on the backend's stream
            self.flat.wait()                                      # ... and joined right before the optimizer reads the gradients
        self.opt.step()


def timed(step_fn, steps, warmup, dev, distributed):
    for _ in range(warmup):
        step_fn()
    if distributed:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step_fn()
    torch.cuda.synchronize(dev)
    if distributed:
        dist.barrier()
    dt = time.perf_counter() - t0
    if distributed:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


DUMP_BYTES = 60_000_000       # array bytes --dump-outputs writes in all (with their .npy headers the files stay below 64 MB)
DUMP_WHOLE_BYTES = 1 << 20    # an array of at most this many bytes is always written whole


def dump_outputs(arrays, out_dir, budget=DUMP_BYTES):
    """--dump-outputs: every array as <out_dir>/<name>.npy, in float32 (float64 stays float64).  When they hold more than `budget`
    bytes in all, each array larger than DUMP_WHOLE_BYTES keeps the same fraction of its rows, chosen so that the total fits: a
    sorted sample drawn by a generator seeded with 0, so the same shape keeps the same rows in every run and every build.
    Returns each array's full shape and how many of its rows were written (null: all of them), for the result line."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: v.detach() if v.dtype == torch.float64 else v.detach().float() for k, v in arrays.items()}
    nbytes = {k: v.numel() * v.element_size() for k, v in arrays.items()}
    sampled = {k for k, v in arrays.items() if nbytes[k] > DUMP_WHOLE_BYTES and v.dim() >= 1 and v.shape[0] > 1}
    frac = 1.0
    if sum(nbytes.values()) > budget:
        frac = max(budget - sum(n for k, n in nbytes.items() if k not in sampled), 0) / sum(nbytes[k] for k in sampled)
    manifest = {}
    for name, t in arrays.items():
        shape, kept = list(t.shape), None
        if name in sampled and frac < 1.0:
            rows = np.sort(np.random.default_rng(0).choice(t.shape[0], max(1, int(t.shape[0] * frac)), replace=False))
            t = t.index_select(0, torch.from_numpy(rows).to(t.device))
            kept = len(rows)
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())
        manifest[name] = dict(shape=shape, rows_kept=kept)
    return manifest


# ------------------------------------------------------------------------------------------------
# roofline of the masked aggregation kernel: HIP events around back-to-back launches on torch's stream
# ------------------------------------------------------------------------------------------------
def aggregation_roofline(wl, data, dev, reps=30, rounds=5, step_fn=None):
    """Forward masked-aggregation kernel and the WHOLE aggregation backward (every launch it takes), priced on compulsory bytes.
    `us_per_launch` / `frac` = the launch timed with HIP events (torch's stream = the launch stream) right behind a real hot-path step
    (cold caches, the state the kernel meets inside the timed region); rocprofv3's per-kernel average of the bench command
    (profiles/) agrees with that one.  `us_isolated` / `frac_isolated` = back-to-back launches with the queue kept busy: the kernel's
    best case."""
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import call, ptr, stream
    N, E, H = data.num_nodes, data.num_edges, wl["H"]
    ix = G.get_index(data.edge_index, N)
    ix.graphs(data.batch, data.num_graphs)
    x = torch.randn(N, H, device=dev)
    att = torch.rand(E, device=dev)
    if wl["backbone"] == "PNA":
        A, S = len(PNA_AGGR), 1
        codes = [G.ops.AGGREGATOR_CODES[a] for a in PNA_AGGR]
        a_arr, s_arr = (ctypes.c_int32 * A)(*codes), (ctypes.c_int32 * 1)(0)
        y = torch.empty(N, S * A * 2 * H, device=dev)
        node_att = not wl["edge_att"]               # the step forms att[row] * att[source] inside the kernels (no lifted [E] tensor): price THAT variant
        na = torch.rand(N, device=dev)
        def launch():
            if node_att:
                call("gsat_pna_fwd_node_att", ptr(x), ptr(na), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), N, H, a_arr, A, s_arr, S, 1.0, 1.0, ptr(y), stream())
            else:
                call("gsat_pna_fwd", ptr(x), ptr(att), None, ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst), N, H,
                     a_arr, A, s_arr, S, 1.0, 1.0, ptr(y), stream())
        alg_bytes = 4 * N * H + 8 * A * S * N * H + 8 * E + 4 * N        # SURVEY 8d (unfused PNA forward)
        kname = "k_pna_fwd"
    else:
        y = torch.empty(N, H, device=dev)
        ee = torch.randn(E, H, device=dev) if data.edge_attr is not None else None
        def launch():
            call("gsat_aggr_sum_fwd", ptr(x), None, ptr(att), ptr(ee), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst),
                 N, E, H, 1.0, ptr(y), ptr(ix.long_rows[0]), ptr(ix.partial(H)) if ix.long_rows[0] is not None else None, stream())
        alg_bytes = 8 * N * H + 8 * E + 4 * N + (4 * E * H if ee is not None else 0)   # SURVEY 8d (+ edge_emb read for GINE)
        kname = "k_aggr_sum_fwd"

    def time_launches(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(rounds):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(4_000_000)              # keep the queue busy so the launches below run back to back
            start.record()
            for _ in range(reps):
                fn()
            end.record()
            torch.cuda.synchronize(dev)
            ts.append(start.elapsed_time(end) * 1e-3 / reps)
        return float(np.median(ts))

    def time_in_step(fn, samples=15):
        """One launch right behind a real step: the queue is never empty (the step is still executing when the launch is
        enqueued), and the caches hold what the step left, not the kernel's own previous run."""
        if step_fn is None:
            return None
        ts = []
        for _ in range(samples):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            step_fn()
            start.record()
            fn()
            end.record()
            torch.cuda.synchronize(dev)
            ts.append(start.elapsed_time(end) * 1e-3)
        return float(np.median(ts))

    t = time_launches(launch)
    t_in = time_in_step(launch)
    achieved = alg_bytes / t / 1e9
    traffic = None          # HBM bytes per launch from rocprofv3 PMC passes (offline, profiles/pmc_traffic.json), same shape only
    bwd_traffic = None
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get(wl.get("key", ""))
        if rec and rec["algorithmic_bytes_per_launch"] == int(alg_bytes):
            traffic = rec["traffic_bytes_per_launch"]
            bwd_traffic = rec.get("backward_traffic_bytes")
    except (OSError, ValueError, KeyError):
        pass
    # `achieved` / `frac` / `us_per_launch` are the IN-STEP figures (one launch timed with HIP events right behind a real hot-path step: cold
    # caches, the state the kernel meets inside the timed region; rocprofv3's in-step average of the same command is in profiles/ and
    # agrees within a dispatch gap).  The back-to-back best case -- the number round 2 reported as `frac` -- stays as `*_isolated`.
    t_rep = t_in if t_in else t
    out = dict(bound="hbm", kernel=kname, achieved=round(alg_bytes / t_rep / 1e9, 1), peak=HBM_PEAK_GBS, unit="GB/s",
               frac=round(alg_bytes / t_rep / 1e9 / HBM_PEAK_GBS, 4), traffic=traffic, alg_bytes_per_launch=int(alg_bytes),
               us_per_launch=round(t_rep * 1e6, 2), timing="in_step" if t_in else "isolated",
               us_isolated=round(t * 1e6, 2), achieved_isolated=round(achieved, 1), frac_isolated=round(achieved / HBM_PEAK_GBS, 4),
               nodes=N, edges=E)
    # what plain streaming passes over a buffer of the kernel's output size reach on this box (quote the vendor
    # peak AND the measured rate): a write-only fill and a device-to-device copy (bytes = read + write)
    y2 = torch.empty_like(y)
    t_fill = time_launches(lambda: y.fill_(1.0))
    t_copy = time_launches(lambda: y2.copy_(y))
    fill_gbs, copy_gbs = y.numel() * 4 / t_fill / 1e9, 2 * y.numel() * 4 / t_copy / 1e9
    out["measured_stream"] = dict(fill_GBps=round(fill_gbs, 1), copy_GBps=round(copy_gbs, 1), buffer_bytes=int(y.numel() * 4),
                                  frac_of_fill=round(achieved / fill_gbs, 4), frac_of_copy=round(achieved / copy_gbs, 4))
    del y2
    # the WHOLE backward of the same aggregation -- every launch it takes -- against its compulsory bytes (upstream gradient in,
    # x in, dx out, att / datt / both index arrays, row pointers); scratch the implementation writes for itself is NOT counted
    if wl["backbone"] == "PNA":
        dout = torch.randn(N, S * A * 2 * H, device=dev)
        dx, dmsg, datt = torch.empty(N, H, device=dev), torch.empty(E, H, device=dev), torch.empty(E, device=dev)
        tiles = ix.pna_tiles(H) if os.environ.get("GSAT_PNA_TILED", "1") != "0" else None
        if tiles:
            tile_desc, T, rows_nominal, rows_cap, edges_cap, spill = tiles
            dna, dw = torch.empty(N, device=dev), torch.empty(max(E, 1), device=dev)
            def launch_bwd():
                if node_att:
                    call("gsat_pna_bwd_tiled_node_att", ptr(x), ptr(na), ptr(dout), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(tile_desc), T,
                         rows_nominal, rows_cap, edges_cap, ptr(ix.rowptr_src), ptr(ix.slot_dst_of_srcslot), N, E, H, a_arr, A, s_arr, S,
                         ptr(spill[1:]), ptr(spill[:1]), ptr(dx), ptr(dmsg), ptr(dna), ptr(dw), None, 0, stream())
                else:
                    call("gsat_pna_bwd_tiled", ptr(x), ptr(att), ptr(dout), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst),
                         ptr(tile_desc), T, rows_nominal, rows_cap, edges_cap, ptr(ix.rowptr_src), ptr(ix.slot_dst_of_srcslot), N, E, H,
                         a_arr, A, s_arr, S, ptr(spill[1:]), ptr(spill[:1]), ptr(dx), ptr(dmsg), ptr(datt), None, stream())
            bname = "k_pna_bwd_tile + k_pna_bwd_spill"
        else:
            dx_self = torch.empty(N, H, device=dev)
            def launch_bwd():
                call("gsat_pna_bwd", ptr(x), ptr(att), None, ptr(dout), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst), N, H,
                     a_arr, A, s_arr, S, 1.0, 1.0, ptr(dx_self), ptr(dmsg), ptr(datt), None, stream())
                call("gsat_aggr_sum_fwd", ptr(dmsg), ptr(dx_self), None, None, ptr(ix.rowptr_src), ptr(ix.slot_dst_of_srcslot), None, N, E, H,
                     1.0, ptr(dx), None, None, stream())
            bname = "k_pna_bwd_dst + k_aggr_sum_fwd"
        bwd_bytes = 4 * S * A * 2 * N * H + 4 * N * H + 4 * N * H + 16 * E + 4 * N          # dout, x, dx, att/datt/col/eid, rowptr
    else:
        dout = torch.randn(N, H, device=dev)
        dx, datt = torch.empty(N, H, device=dev), torch.empty(E, device=dev)
        dee = torch.empty(E, H, device=dev) if data.edge_attr is not None else None
        def launch_bwd():
            call("gsat_aggr_sum_bwd", ptr(x), ptr(att), ptr(ee), ptr(dout), ptr(ix.rowptr_src), ptr(ix.dst_by_src), ptr(ix.eid_by_src),
                 N, E, H, 1.0, ptr(dx), ptr(datt), ptr(dee), ptr(ix.long_rows[1]),
                 ptr(ix.partial(H)) if ix.long_rows[1] is not None else None, stream())
        bwd_bytes = 12 * N * H + 16 * E + 8 * N + (8 * E * H if ee is not None else 0)            # SURVEY 8d (+ edge_emb read, dedge write)
        bname = "k_aggr_sum_bwd"
    tb = time_launches(launch_bwd)
    tb_in = time_in_step(launch_bwd)
    tb_rep = tb_in if tb_in else tb
    out["backward"] = dict(kernels=bname, achieved=round(bwd_bytes / tb_rep / 1e9, 1), frac=round(bwd_bytes / tb_rep / 1e9 / HBM_PEAK_GBS, 4),
                           compulsory_bytes=int(bwd_bytes), us_all_launches=round(tb_rep * 1e6, 2), timing="in_step" if tb_in else "isolated",
                           us_isolated=round(tb * 1e6, 2), frac_isolated=round(bwd_bytes / tb / 1e9 / HBM_PEAK_GBS, 4), traffic=bwd_traffic)
    return out


# ------------------------------------------------------------------------------------------------
# CPU baseline: the oracle (plain-PyTorch restatement of the reference op sequence) on the host cores
# ------------------------------------------------------------------------------------------------
def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(wl, name, seed, sample_graphs=0, warmup=3, steps=10, budget_s=120.0):
    """SURVEY 8d / BASELINE.md 2: the oracle's scope-A step on the host, FULL batch, 3 warm-up + median of 10 steps, at
    torch.set_num_threads(5) (the reference's own setting, src/run_gsat.py:1049) and at all physical cores; both are reported,
    `value` is the faster.  If the protocol at 5 threads would exceed half of `budget_s` the batch is cut to its leading graphs and
    `sample_fraction` says by how much (edges/s is size-independent to first order: per-graph work); a thread setting that is much
    slower (oversubscribed cores) stops after the steps that fit its half of the budget (`steps_measured`)."""
    from oracle import bookkeeping as bk
    from oracle import modules as om
    from oracle import ops as oops
    from dp_gsat_amd.dist import take_graphs
    full, _, _ = make_batch(name, wl["graphs"], seed)

    def build(d):
        N, E, H, L = d.num_nodes, d.num_edges, wl["H"], wl["L"]
        g = torch.Generator().manual_seed(seed)
        ext = om.ExtractorMLP(H, wl["edge_att"]).train()
        emb = torch.randn(N, H, generator=g).requires_grad_(True)
        xs = [torch.randn(N, H, generator=g).requires_grad_(True) for _ in range(L)]
        gine = d.edge_attr is not None
        ees = [torch.randn(E, H, generator=g).requires_grad_(True) for _ in range(L)] if gine else None
        width = len(PNA_AGGR) * 2 * H if wl["backbone"] == "PNA" else H
        gouts = [torch.randn(N, width, generator=g) for _ in range(L)]
        M = E if wl["edge_att"] else N
        C1 = 4 * H if wl["edge_att"] else 2 * H

        def step():
            for p in ext.parameters():
                p.grad = None
            emb.grad = None
            u = torch.empty(M, 1).uniform_(1e-10, 1 - 1e-10)
            masks = [(torch.rand(M, C1) > 0.5).float(), (torch.rand(M, H) > 0.5).float()]
            z = ext(emb, d.edge_index, d.batch, masks=masks)
            att = oops.concrete_sample(z, u, True)
            if wl["edge_att"]:
                rev = torch.from_numpy(bk.reverse_edge_perm(d.edge_index, N)) if bk.is_undirected(d.edge_index, N) else None
                edge_att = oops.symmetrise(att, rev)
            else:
                edge_att = oops.lift_node_att_to_edge_att(att, d.edge_index)
            outs = []
            for l in range(L):
                if wl["backbone"] == "PNA":
                    outs.append(oops.pna_aggregate(xs[l], d.edge_index, edge_att, PNA_AGGR, ["identity"], {"lin": 1.0, "log": 1.0}))
                elif gine:
                    outs.append(oops.gine_aggregate(xs[l], d.edge_index, ees[l], edge_att))
                else:
                    outs.append(oops.gin_aggregate(xs[l], d.edge_index, edge_att))
            torch.autograd.backward(outs, gouts)
        return step, N, E

    default_threads = torch.get_num_threads()
    physical = max(1, (os.cpu_count() or 2) // 2)            # SMT host: logical / 2
    # 5 = the reference's own setting; all physical cores per SURVEY 8d; 16 / 32 / 64 so that one datum is not an oversubscription artefact
    thread_settings = sorted({5, physical} | {t for t in (16, 32, 64) if t <= physical})
    load0 = os.getloadavg() if hasattr(os, "getloadavg") else (None, None, None)
    d = full if not sample_graphs else take_graphs(full, range(min(sample_graphs, full.num_graphs)))
    step, N, E = build(d)
    torch.set_num_threads(5)
    t0 = time.perf_counter(); step(); t_probe = time.perf_counter() - t0      # probe at the reference's thread count
    share = budget_s / len(thread_settings)
    if not sample_graphs and t_probe * (warmup + steps) > share and full.num_graphs > 1:
        keep = max(1, int(full.num_graphs * share / (t_probe * (warmup + steps))))
        d = take_graphs(full, range(keep))
        step, N, E = build(d)
    results, measured = {}, {}
    for threads in thread_settings:
        torch.set_num_threads(threads)
        t_begin = time.perf_counter()
        for i in range(warmup):
            step()
            if time.perf_counter() - t_begin > budget_s / (4 * len(thread_settings)):
                break                                   # a very slow setting (oversubscribed cores): do not burn the budget on warm-up
        ts = []
        for i in range(steps):
            t0 = time.perf_counter()
            step()
            ts.append(time.perf_counter() - t0)
            if len(ts) >= 3 and time.perf_counter() - t_begin > budget_s / len(thread_settings):
                break
        results[threads] = float(np.median(ts))
        measured[threads] = len(ts)
    torch.set_num_threads(default_threads)
    threads, t = min(results.items(), key=lambda kv: kv[1])
    frac = d.num_graphs / full.num_graphs
    return dict(value=round(E / t / 1e6, 5), unit="million edges/s", cores=int(threads), kind="port",
                sample=f"oracle scope-A step on {d.num_graphs} of {full.num_graphs} graphs of the workload ({N} nodes, {E} directed edges), "
                       f"{warmup} warm-up + median of {steps} steps per thread setting, {t * 1e3:.1f} ms/step",
                sample_fraction=round(frac, 4), warmup=warmup, steps=steps, steps_measured={str(k): v for k, v in measured.items()},
                by_threads={str(k): round(E / v / 1e6, 5) for k, v in results.items()}, physical_cores=physical,
                host_cpus=os.cpu_count(), cpu_model=_cpu_model(), host_loadavg_before=[round(x, 1) for x in load0 if x is not None],
                host_loadavg_after=[round(x, 1) for x in os.getloadavg()] if hasattr(os, "getloadavg") else None)


def main():
    # dump every thread's stack and exit if the run takes longer than this many seconds (GSAT_BENCH_WATCHDOG); on by default for N > 1,
    # where a rank that misses a collective would otherwise sit silently until the launcher's own timeout (N > 1 runs take < 2 minutes)
    watchdog = os.environ.get("GSAT_BENCH_WATCHDOG", "540" if int(os.environ.get("WORLD_SIZE", "1")) > 1 else "")
    if watchdog and float(watchdog) > 0:
        import faulthandler
        faulthandler.dump_traceback_later(float(watchdog), exit=True)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 200; 10 for the c5 workloads)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up steps (default 20; 3 for the c5 workloads)")
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reuse-index", action="store_true", help="keep the per-batch bookkeeping cached across steps")
    ap.add_argument("--full", action="store_true", help="after the timed steps also run the exact-fp32 re-timing, the whole training step, "
                                                         "the roofline leg and the CPU baseline (each can be left out with its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB in all: larger outputs "
                         "as a fixed, seeded sample of their rows; the result line's `dump_outputs` gives the full shapes)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-full-step", action="store_true", help="with --full: skip the whole training step")
    ap.add_argument("--no-exact-rerun", action="store_true", help="with --full: skip the second timing with the extractor's backward products on exact fp32")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline leg")
    ap.add_argument("--cpu-sample-graphs", type=int, default=0)
    ap.add_argument("--graph", dest="graph", action="store_true", default=None,
                    help="capture the step into a hipGraph (torch.cuda.graph) and time replays; DEFAULT on one GPU for c1-c4: the fork's "
                         "loaders are unshuffled (src/utils/get_data_loaders.py:133,141), so every batch recurs with the same shape each epoch "
                         "and a per-batch graph is what a training loop would replay; the index is still rebuilt inside every replay")
    ap.add_argument("--eager", dest="graph", action="store_false", help="plain eager launches (the default for the c5 workloads and for N > 1)")
    ap.add_argument("--sync-free", action="store_true", help="eager launches, but no device->host read inside the step (dp_gsat_amd.set_sync_free)")
    ap.add_argument("--roofline-only", action="store_true", help="only run the aggregation-kernel roofline leg (for rocprofv3 --pmc passes)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only to rehearse N>1 on one GPU)")
    args = ap.parse_args()
    big = args.workload in ("c5", "c5s")
    if args.steps is None:
        args.steps = 10 if big else 200          # a 1.2 ms step needs a few hundred repetitions for a stable mean
    if args.warmup is None:
        args.warmup = 3 if big else 20

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    mode_given = args.graph is not None
    if args.graph is None:
        # launch-bound batches (c1, c2, c4: 60-70 launches of a few microseconds) replay as one hipGraph.  c3 issues ~110 launches in
        # ~0.9 ms of host time against ~0.95 ms of GPU time: eager it measures the same on an idle host (0.965 ms) and 5-13 % worse on a
        # loaded one (tools/host_time_c3.py, profiles/r02_summary.md), so it replays as a graph too; c5 is GPU-bound by a wide margin
        # N > 1 stays eager by default: graph replay per rank + an eager RCCL all-reduce behind it (`--graph` under torchrun does exactly
        # that) could only be rehearsed with two gloo ranks sharing one GPU, never on a multi-GPU node
        args.graph = world == 1 and "RANK" not in os.environ and args.workload in ("c1", "c2", "c3", "c4") and not args.sync_free
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # under torchrun (RANK set) the process group is initialised even at world size 1, so the RCCL path can be rehearsed on one GPU
    distributed = world > 1 or ("RANK" in os.environ and "MASTER_PORT" in os.environ)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    dev = torch.device("cuda", local_rank % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    if args.gpus != world and rank == 0:
        print(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)

    import __graft_entry__ as ge
    from dp_gsat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) and rank == 0:
        ge.build()
    if distributed:
        dist.barrier()
    _lib.load()

    wl = dict(WORKLOADS[args.workload], key=args.workload)
    host_batch, x_dim, e_dim = local_shard(args.workload, wl["graphs"], rank, world, args.seed)
    data = host_batch.to(dev)
    torch.manual_seed(args.seed + rank)

    if args.roofline_only:
        print(json.dumps({"roofline": aggregation_roofline(wl, data, dev, reps=10, rounds=2)}))
        return
    hot = HotPath(wl, data, dev, seed=args.seed + rank)
    hot.reuse_index = args.reuse_index
    hot.keep_outputs = bool(args.dump_outputs) and rank == 0
    if distributed:
        hot.attach_dp()
    def captured(fn):
        """Capture one call of `fn` into a hipGraph (after eager warm-up on a side stream) and return the replay callable."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return graph.replay

    import dp_gsat_amd as G
    G.set_sync_free(bool(args.graph or args.sync_free))    # graph mode: no host read-backs inside the step, so it is capturable
    if args.graph and distributed:
        try:
            replay = captured(hot.compute)        # everything but the collective; the gradients land in the flat buffer at fixed addresses

            def step_fn():
                replay()
                hot.reduce()
        except Exception as exc:                  # a backend that does not tolerate captures next to its communicator: measure eagerly
            print(f"[bench] rank {rank}: capture failed ({exc}); falling back to eager launches", file=sys.stderr)
            args.graph = False
            G.set_sync_free(bool(args.sync_free))
            step_fn = hot.step
    else:
        step_fn = captured(hot.step) if args.graph else hot.step
    dt = timed(step_fn, args.steps, args.warmup, dev, distributed)
    dumped = None
    if hot.keep_outputs:
        dumped = dump_outputs(hot.outputs(), args.dump_outputs)      # before any --full leg runs the step again
    e_local = torch.tensor([float(data.num_edges), float(data.num_nodes)], dtype=torch.float64, device=dev)
    if distributed:
        dist.all_reduce(e_local)
    e_total, n_total = e_local.tolist()
    ms = dt / args.steps * 1e3
    value = e_total / (dt / args.steps) / 1e6

    from dp_gsat_amd.ops import ExtractorAttention
    fwd_kind = ExtractorAttention.last_forward_kind                  # what the timed steps ran (gsat_attn_fwd_kind)
    FWD_PRECISION = {0: "extractor forward: staged kernels, layer products (P|Q, h2) exact fp32 MFMA",
                     1: "extractor forward: one-launch kernel (whole graphs per workgroup), layer products exact fp32 MFMA",
                     2: "extractor forward: one-launch kernel (whole graphs per workgroup), layer products split-bf16 x6 (operands as three bf16 planes, six "
                        "bf16 MFMA per 16 k, fp32 accumulate: rel. error ~1e-6, fp32-GEMM level)"}
    # the same step with every extractor product on exact fp32 MFMA (GSAT_ATTN_BWD_SPLIT=0, staged forward), measured in the same
    # process so that the line says what the default costs / buys
    value_exact = ms_exact = None
    if args.full and world == 1 and not distributed and not args.no_exact_rerun:
        os.environ["GSAT_ATTN_BWD_SPLIT"] = "0"
        fused_env = os.environ.get("GSAT_ATTN_FUSED")
        os.environ["GSAT_ATTN_FUSED"] = "0"            # the staged forward: exact fp32 MFMA
        try:
            step_exact = captured(hot.step) if args.graph else hot.step
            dte = timed(step_exact, args.steps, max(args.warmup // 2, 2), dev, False)
            ms_exact = dte / args.steps * 1e3
            value_exact = e_total / (dte / args.steps) / 1e6
        finally:
            del os.environ["GSAT_ATTN_BWD_SPLIT"]
            if fused_env is None:
                del os.environ["GSAT_ATTN_FUSED"]
            else:
                os.environ["GSAT_ATTN_FUSED"] = fused_env

    full = None
    if args.full and not args.no_full_step:
        # the whole training step of C3 is GPU-bound by a wide margin (4.6 ms) and measures ~4 % better eager than captured (capturable
        # Adam, device-side seeds): unless a mode was asked for, only the launch-bound workloads replay it as a graph
        full_graph = bool(args.graph) and (mode_given or args.workload != "c3") and not distributed      # N > 1: forward/backward, all-reduce, Adam stay eager
        G.set_sync_free(bool(full_graph or args.sync_free))
        fs = FullStep(wl, data, x_dim, e_dim, dev, capturable=full_graph)
        if distributed:
            fs.attach_dp()
        fstep = captured(fs.step) if full_graph else fs.step
        fsteps = max(args.steps // 2, 3)
        fdt = timed(fstep, fsteps, max(args.warmup // 2, 2), dev, distributed)
        by_mode = {"hipgraph" if full_graph else "eager": round(fdt / fsteps * 1e3, 3)}
        if args.graph and not mode_given and not full_graph and not distributed:
            # C3's whole step, default run: eager it is ~10 % faster than the replayed graph on an idle host (4.2 vs 4.8 ms) and slower on a
            # loaded one (its ~450 launches make it host-sensitive; 5.1-5.3 ms seen).  Time the captured step too and report the faster mode;
            # both figures stay in `ms_by_mode`.
            G.set_sync_free(True)
            fs2 = FullStep(wl, data, x_dim, e_dim, dev, capturable=True)
            fdt2 = timed(captured(fs2.step), fsteps, max(args.warmup // 2, 2), dev, False)
            by_mode["hipgraph"] = round(fdt2 / fsteps * 1e3, 3)
            if fdt2 < fdt:
                fdt, full_graph = fdt2, True
            del fs2
        full = dict(value=round(e_total / (fdt / fsteps) / 1e6, 3), unit="million edges/s", ms_per_step=round(fdt / fsteps * 1e3, 3), ms_by_mode=by_mode, adam=fs.adam,
                    what="whole GSAT training step: 2 backbone passes + extractor + losses + backward + Adam (+ all-reduce)", hipgraph=full_graph,
                    gemm_precision=FWD_PRECISION[ExtractorAttention.last_forward_kind] + "; extractor backward products (da1, demb, dW1, dW2) and backbone "
                                   "Linear layers >= 2 GFLOP (forward, dx, dW): bf16x3 (split-bf16 hi*hi + hi*lo + lo*hi, fp32 accumulate, rel. error ~1e-5); "
                                   "smaller Linear layers: library fp32 GEMM")

    G.set_sync_free(False)
    roof, cpu = None, None
    if args.full and rank == 0:
        hot.reuse_index = True
        hot.flat = None          # rank 0 alone runs this leg: its in-step timing must not enter the gradient all-reduce (the other ranks wait at the barrier below)
        roof = None if args.no_roofline else aggregation_roofline(wl, data, dev, step_fn=hot.step)
        if not args.no_cpu_baseline and world == 1:          # reported at N=1 only
            cpu = cpu_baseline(wl, args.workload, args.seed, args.cpu_sample_graphs)
    if distributed:
        dist.barrier()

    if rank == 0:
        line = {
            "metric": "million edges/s (attn+sample+aggregate fwd+bwd)", "value": round(value, 3), "unit": "million edges/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "gemm_precision": "timed region: " + FWD_PRECISION[fwd_kind] + "; extractor backward products (da1, demb, dW1, dW2) "
                              "split-bf16 x3 (hi*hi + hi*lo + lo*hi on bf16 MFMA, fp32 accumulate, rel. error ~1e-5 of each gradient's scale); "
                              "aggregation kernels fp32 VALU; no other GEMM in scope A",
            "value_fp32_exact": None if value_exact is None else round(value_exact, 3),
            "ms_per_step_fp32_exact": None if ms_exact is None else round(ms_exact, 4),
            "config": {"workload": wl["desc"], "graphs_per_gpu": wl["graphs"], "nodes_total": int(n_total), "edges_total": int(e_total),
                       "hidden": wl["H"], "layers": wl["L"], "attention": "edge" if wl["edge_att"] else "node",
                       "parallelism": f"dp{world}", "index_rebuilt_every_step": not args.reuse_index, "hipgraph": bool(args.graph), "sync_free": bool(args.graph or args.sync_free)},
            "roofline": roof, "cpu_baseline": cpu, "full_step": full,
        }
        if dumped is not None:
            line["dump_outputs"] = dict(dir=args.dump_outputs, arrays=dumped)
        if cpu:
            line["speedup_vs_cpu_port"] = round(value / world / cpu["value"], 1) if cpu["value"] > 0 else None
        print(json.dumps(line))
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
