"""-m gpu: the dual/primal step on ragged batches -- the count-aware soft-F1 kernel against fp64, the dual dataset and the paired
fixed-capacity collation bit-exact, DualGSAT on a padded pair (eager and as replays of ReplayedDualStep's two captured graphs) against the
oracle's DualGSAT on the UNPADDED batches.  Floating-point comparisons follow tests.util.close (TOL = 1e-4, fp64 evaluation as ref64).

The per-graph dual reference is oracle.bookkeeping.line_graph_by_source (source nodes taken in ascending order), the rule of
dp_gsat_amd.line_graph that gives the reference's 451 808 dual edges on Mutagenicity.  tests.graphs.line_graph joins primal edges
that share ANY endpoint (about four times the edges, in sorted order), so it cannot equal that rule bit for bit; it is checked as far
as the two rules agree: its pairs with a common source are exactly the dual's edge set."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import dual_oracle as do
from tests import padded_oracle as po
from tests.graphs import line_graph
from tests.test_gpu_padded import _adam64
from tests.util import TOL, assert_no_memset_nodes, close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = do.H


# ---- 1. soft-F1 sparsity loss over the first m entries -------------------------------------------------------------------------------------
def _f1_case(dev, M, m, counted):
    import dp_gsat_amd as G
    g = torch.Generator().manual_seed(M + 7 * m)
    p = torch.rand(M, 1, generator=g) * 0.96 + 0.02
    y = (torch.rand(M, generator=g) > 0.6).float()
    gout = 1.7
    ref, dref = do.f1_reference(p, y, m, gout)
    runs = []
    for spoil in (False, True):
        pp, yy = p.clone(), y.clone()
        if spoil:
            pp[m:], yy[m:] = float("nan"), 1.0                 # entries beyond the count are never loaded
        pd = pp.to(dev).requires_grad_(True)
        yd = yy.to(dev).requires_grad_(True)
        mv = torch.tensor([m], dtype=torch.int32, device=dev) if counted else None
        out = G.f1_sparsity_loss_valid(pd, yd, mv)
        (out * gout).backward()
        torch.cuda.synchronize()
        what = f"M={M} m={m} counted={counted} spoil={spoil}: "
        assert yd.grad is None, what + "y gets no gradient"
        assert torch.isfinite(out) and torch.isfinite(pd.grad).all(), what + "not finite"
        print(what, "loss", float(out.detach()), "ref", float(ref), "max|dp err|", float((pd.grad[:m].cpu().double().reshape(-1) - dref).abs().max()) if m else 0.0)
        close(out, ref, TOL, what=what + "loss")
        close(pd.grad[:m].reshape(-1), dref, TOL, what=what + "dp")
        if m:                                                   # the gradients are of size 1/m: compare at their own scale too
            err = float((pd.grad[:m].cpu().double().reshape(-1) - dref).abs().max())
            assert err <= TOL * float(dref.abs().max()), what + f"dp relative: {err:.3e}"
        assert pd.grad.shape == p.shape and not pd.grad[m:].any(), what + "dp beyond the count must be exactly 0"
        runs.append((out.detach().clone(), pd.grad.detach().clone()))
        if not counted or m == M:
            break
    if len(runs) == 2:
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "NaN beyond the count changed the result"
    return p, y


@pytest.mark.parametrize("m", [0, 1, 257, 1500])
def test_f1_sparsity_counts_valid_entries_only(dev, m):
    import dp_gsat_amd as G
    _f1_case(dev, 1500, m, True)
    if m == 0:
        z = torch.zeros(1, dtype=torch.int32, device=dev)
        pd = torch.full((1500, 1), float("nan"), device=dev, requires_grad=True)
        out = G.f1_sparsity_loss_valid(pd, torch.ones(1500, device=dev), z)
        out.backward()
        assert float(out.detach()) == 1.0 and not pd.grad.any()


def test_f1_sparsity_lengths_labels_and_repeatability(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import load
    chunk, blocks = int(load().gsat_f1_sparsity_block_entries()), int(load().gsat_f1_sparsity_max_blocks())
    assert (chunk, blocks) == (1024, 256)
    block = 256                                                 # threads per block: one float4 each per sweep
    for M in (block - 1, block, block + 1, chunk - 1, chunk, chunk + 1, chunk * (blocks - 1) + 5,
              300_001):                                     # above chunk * blocks: every block sweeps its range more than once
        p, y = _f1_case(dev, M, M, False)
        pd, yd = p.to(dev), y.to(dev)
        a, b = G.f1_sparsity_loss_valid(pd, yd), G.f1_sparsity_loss_valid(pd, yd)
        assert torch.equal(a, b), "two calls must be bitwise equal"
        close(a, G.f1_sparsity_loss(pd, yd.view(-1, 1)), TOL, what=f"M={M}: against f1_sparsity_loss")
    # a view that is not 16-byte aligned takes the scalar loads
    p, y = torch.rand(1031, 1) * 0.9 + 0.05, (torch.rand(1031) > 0.5).float()
    pd = p.to(dev).requires_grad_(True)
    out = G.f1_sparsity_loss_valid(pd[1:], y.to(dev)[1:], torch.tensor([1000], dtype=torch.int32, device=dev))
    out.backward()
    ref, dref = do.f1_reference(p[1:], y[1:], 1000)
    close(out, ref, TOL, what="unaligned loss")
    close(pd.grad[1:1001].reshape(-1), dref, TOL, what="unaligned dp")
    assert not pd.grad[1001:].any() and not pd.grad[:1].any()
    # all-zero labels: TP = G = 0, f1 = 0
    pd = torch.rand(700, 1, device=dev).requires_grad_(True)
    out = G.f1_sparsity_loss_valid(pd, torch.zeros(700, device=dev), torch.tensor([300], dtype=torch.int32, device=dev))
    out.backward()
    assert torch.isfinite(out) and torch.isfinite(pd.grad).all()
    close(out, 1.0 + pd[:300].detach().abs().mean(), TOL, what="all-zero labels")


# ---- 2. the dual dataset ---------------------------------------------------------------------------------------------------------------------
def test_line_graph_dataset_is_bit_exact_per_graph(dev):
    import dp_gsat_amd as G
    graphs = do.labelled_graphs(count=12)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    dual = ds.line_graph_dataset()
    assert dual.num_graphs == 12 and torch.equal(dual.node_counts, ds.edge_counts) and torch.equal(dual.node_ptr_all, ds.edge_ptr_all)
    assert torch.equal(dual.y_all, ds.y_all) and dual.edge_attr_all is None
    want = do.dual_edges(graphs)
    ptr = dual.edge_ptr_all.cpu().numpy()
    got_all = dual.edge_local_all.cpu().numpy()
    assert ptr[-1] == got_all.shape[1] == sum(w.shape[1] for w in want)
    xs = dual.x_all.cpu()
    eptr = ds.edge_ptr_all.cpu().numpy()
    for g, (gr, w) in enumerate(zip(graphs, want)):
        got = got_all[:, ptr[g]:ptr[g + 1]]
        assert np.array_equal(got, w), f"graph {g}"
        ei = gr.edge_index
        loose, _ = line_graph(ei, torch.zeros(gr.x.shape[0], dtype=torch.int64))       # any shared endpoint; sorted
        same_src = ei[0][loose[0]] == ei[0][loose[1]]
        assert sorted(map(tuple, loose[:, same_src].T.tolist())) == sorted(map(tuple, got.T.tolist())), f"graph {g}: edge set"
        assert torch.equal(xs[eptr[g]:eptr[g + 1]], torch.cat([gr.x[ei[0]], gr.x[ei[1]]], dim=1)), f"graph {g}: dual x"
    feats = torch.randn(int(eptr[-1]), 3)
    assert torch.equal(ds.line_graph_dataset(feats.to(dev)).x_all.cpu(), feats)
    with pytest.raises(ValueError, match="one row per primal edge"):
        ds.line_graph_dataset(feats[:-1].to(dev))
    lonely = G.PackedDataset.from_data_list(po.mutag_graphs(count=12, single_node=(11,)), dev)
    with pytest.raises(ValueError, match="without edges"):
        lonely.line_graph_dataset()
    G.clear_cache()


def test_line_graph_dataset_of_whole_mutagenicity(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd.synth import mutag_full_topology
    ei, batch, _ = mutag_full_topology(os.path.join(ROOT, "tests", "golden", "mutag_full.npz"))
    counts = torch.bincount(batch)
    start = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    eg = batch[ei[0]]
    ei = ei[:, torch.argsort(eg, stable=True)]
    eg = batch[ei[0]]
    ecount = torch.bincount(eg, minlength=len(counts))
    ds = G.PackedDataset(torch.ones(len(batch), 1).to(dev), (ei - start[eg]).to(dev), start.to(dev),
                         torch.cat([torch.zeros(1, dtype=torch.int64), ecount.cumsum(0)]).to(dev), torch.zeros(len(counts), 1).to(dev))
    dual = ds.line_graph_dataset()
    assert dual.num_graphs == 4337 and int(dual.edge_local_all.shape[1]) == 451808 == int(dual.edge_ptr_all[-1])
    assert torch.equal(dual.node_counts, ds.edge_counts) and dual.x_all.shape == (266894, 2)
    g_of = torch.repeat_interleave(torch.arange(4337, device=dev), dual.edge_counts)
    assert int(dual.edge_local_all.min()) == 0 and bool((dual.edge_local_all < dual.node_counts[g_of]).all())
    G.clear_cache()


# ---- 3. the padded pair ----------------------------------------------------------------------------------------------------------------------
def _pair_datasets(dev, **kw):
    import dp_gsat_amd as G
    graphs = do.labelled_graphs(**kw)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    return graphs, ds, ds.line_graph_dataset()


@pytest.mark.parametrize("case", ["fits", "primal_nodes_one_short", "dual_edges_one_short"])
def test_collate_padded_pair_layout(dev, case):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=12)
    ids_l = po.LAYOUT_IDS[:1] + [3] + po.LAYOUT_IDS[2:]            # LAYOUT_IDS without the graph the host tests cut to one node
    ids = torch.tensor(ids_l, device=dev)
    N, E, Ed = do.pair_totals(graphs, ids_l)
    up, ud = ds.collate(ids), dual.collate(ids)
    assert (up.x.shape[0], up.edge_index.shape[1], ud.x.shape[0], ud.edge_index.shape[1]) == (N, E, E, Ed)
    if case == "fits":
        bound = ds.pair_capacity_for(dual, 5)
        n_all, e_all = po.sizes(graphs)
        d_all = np.array([d.shape[1] for d in do.dual_edges(graphs)])
        assert bound == po.capacity_for(n_all, e_all, 5) + (int(np.sort(d_all)[::-1][:5].sum()),)
        for cap in (None, (N + 2, E, Ed), (N + 7, E + 3, Ed + 5)):
            pb, db = G.collate_padded_pair(ds, dual, ids, cap)
            Np, Ep, Edc = cap or bound
            assert pb.pair is db and db.pair is pb
            assert pb.capacity == (Np, Ep) and db.capacity == (Ep + 2, Edc) and db.capacity[0] == pb.capacity[1] + 2
            assert pb.valid.tolist() == [N, E, 5, 0] and db.valid.tolist() == [E, Ed, 5, 0] and int(db.valid[0]) == int(pb.valid[1])
            assert torch.equal(db.node_src_row[:E], pb.edge_src_slot[:E])
            for b, u, n, e in ((pb, up, N, E), (db, ud, E, Ed)):
                assert torch.equal(b.x[:n], u.x) and torch.equal(b.edge_index[:, :e], u.edge_index) and torch.equal(b.batch[:n], u.batch)
                assert torch.equal(b.y[:5], u.y) and not b.x[n:].any()
            assert torch.equal(pb.edge_label[:E], up.edge_label) and not pb.edge_label[E:].any()
            solo = dual.collate_padded(ids, (Ep + 2, Edc))
            for name in ("batch", "node_src_row", "edge_index", "edge_src_slot", "valid"):
                assert torch.equal(getattr(db, name), getattr(solo, name)), name
        return
    cap = (N + 1, E, Ed) if case == "primal_nodes_one_short" else (N + 2, E, Ed - 1)
    with pytest.raises(ValueError, match="does not fit"):
        G.collate_padded_pair(ds, dual, ids, cap)
    G.set_sync_free(True)
    try:
        pb, db = G.collate_padded_pair(ds, dual, ids, cap)          # nothing is read back: both are flagged and all padding
    finally:
        G.set_sync_free(False)
    assert pb.valid.tolist() == [0, 0, 5, 1] and db.valid.tolist() == [0, 0, 5, 1]
    for b, c in ((pb, (cap[0], cap[1])), (db, (cap[1] + 2, cap[2]))):
        assert not b.x.any() and bool((b.batch == 5).all()) and bool((b.node_src_row == -1).all()) and bool((b.edge_src_slot == -1).all())
        po.check_invariants(dict(valid=np.array([0, 0, 5, 1]), edge_index=b.edge_index.cpu().numpy(), batch=b.batch.cpu().numpy(),
                                 node_src_row=b.node_src_row.cpu().numpy(), edge_src_slot=b.edge_src_slot.cpu().numpy()), c)
    G.clear_cache()


# ---- 4. / 5. whole steps against the oracle on the unpadded batches --------------------------------------------------------------------------
def _dual_gsat(dev, backbone, graphs, optimizers, **kw):
    import dp_gsat_amd as G
    omods, mods = do.models(dev, backbone, graphs)
    opts = (None, None)
    if optimizers:
        opts = tuple(torch.optim.Adam(list(mods[i].parameters()) + list(mods[i + 1].parameters()), lr=1e-3, weight_decay=3e-6,
                                      capturable=True, fused=True) for i in (0, 2))
    dg = G.DualGSAT(mods[0], mods[1], opts[0], mods[2], mods[3], opts[1], do.MCFG, dict(do.MCFG, **kw.pop("dual_cfg", {})), False, False,
                    **kw).train()
    return omods, mods, dg, opts


@pytest.mark.parametrize("epoch", [3, 60], ids=["unmixed", "mixed"])
@pytest.mark.parametrize("backbone", ["GIN", "PNA"])
def test_eager_padded_pair_matches_oracle(dev, backbone, epoch):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, **po.STEP_GRAPHS)
    omods, mods, dg, _ = _dual_gsat(dev, backbone, graphs, False)
    ids_l = po.STEP_IDS[1]
    ids = torch.tensor(ids_l, device=dev)
    B = len(ids_l)
    N, E, Ed = do.pair_totals(graphs, ids_l)
    Np, Ep, Edc = ds.pair_capacity_for(dual, B)
    g = torch.Generator().manual_seed(11 + epoch)
    pu = torch.rand(Np, 1, generator=g).clamp_(1e-10, 1 - 1e-10)
    dU = torch.rand(Ep + 2, 1, generator=g)
    pm = [(torch.rand(Np, 2 * H, generator=g) > 0.5).float(), (torch.rand(Np, H, generator=g) > 0.5).float()]
    dm = [(torch.rand(Ep + 2, 2 * H, generator=g) > 0.5).float(), (torch.rand(Ep + 2, H, generator=g) > 0.5).float()]
    states = do.state_of(mods)
    pb, db = G.collate_padded_pair(ds, dual, ids)
    upb, udb = ds.collate(ids).to("cpu"), dual.collate(ids).to("cpu")
    r = G.get_r(10, 0.1, epoch, final_r=0.5)
    r32, r64 = do.oracle_step(omods, states, upb, udb, epoch > 50, r, pu[:N], dU[:E], [m[:N] for m in pm], [m[:E] for m in dm])
    att, loss, ld, logits = dg.dual_forward_pass(pb, db, epoch, True, pu.to(dev), dU.to(dev), [m.to(dev) for m in pm], [m.to(dev) for m in dm])
    loss.backward()
    torch.cuda.synchronize()
    att = G.ops.edge_tensor(att)
    assert att.shape == (Ep, 1) and logits.shape == (B + 1, 1) and torch.isfinite(logits).all() and torch.isfinite(att).all()
    assert set(ld) == {"loss", "pred", "info"} and all(np.isfinite(v) for v in ld.values())
    do.check_step(att, loss, logits, mods, r32, r64, E, B, f"{backbone} epoch {epoch}: ")
    G.clear_cache()


def _dump(graph):
    try:
        path = os.path.join(tempfile.mkdtemp(), "graph.dot")
        graph.debug_dump(path)
        if os.path.exists(path) and os.path.getsize(path) > 0:
            return open(path, errors="replace").read()
    except Exception:
        pass
    return None


@pytest.mark.parametrize("backbone", ["GIN", "PNA"])
def test_two_captured_graphs_replay_real_pairs(dev, backbone):
    """ReplayedDualStep(pinned=True, mix_after_epoch=1, decay_interval=1): three id sets of different sizes at epochs 0, 1 (the unmixed
    graph) and 2 (the mixed graph, a third r).  The pinned noise and masks, sliced to the real rows, feed the oracle's step on the unpadded
    batches from the pre-step state: loss, attention, logits, every gradient of the four modules and both backbones' running statistics;
    the parameters after the step against fp64 Adam for both optimizers.

    The gradients are compared through tests.util.close with ref64 like everything else, but against the fp32 evaluation of the oracle that
    lies farthest from fp64 among five valid ones (tests.dual_oracle.widest_fp32_gradients: scatter means one ulp apart, as between the
    reference's division and the kernels' multiplication by fl(1 / n)).  With the default dual features PNA's std on the dual graph is
    ill-conditioned, and the plain fp32 oracle under-states the reference's own fp32 spread: measured on an MI355X at replay 0 (graphs
    16..31), the dual node encoder's weight gradient is 3.36e-4 from fp64 -- identically on the unpadded eager step -- where the plain fp32
    oracle is 2.4e-6 away and the four one-ulp variations of it up to 1.06e-4 (allowed: 1e-4 + 4 x 1.06e-4).  Every other tensor of that
    step is within 6e-6 on the device.  For GIN the
    references are the plain ones."""
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, **po.STEP_GRAPHS)
    omods, mods, dg, opts = _dual_gsat(dev, backbone, graphs, True, mix_after_epoch=1, dual_cfg=dict(decay_interval=1))
    names, params = do.names_and_params(mods)
    before = [p.detach().clone() for p in params]
    bufs_before = {k: v.detach().clone() for k, v in dg.state_dict().items()}
    graphs_dbg = []
    for _ in range(2):
        gr = torch.cuda.CUDAGraph()
        try:
            gr.enable_debug_mode()
        except Exception:
            pass
        graphs_dbg.append(gr)
    B = po.STEP_BATCH
    rs = G.ReplayedDualStep(dg, ds, dual, B, pinned=True, keep_edge_att=True, graphs=graphs_dbg)
    assert not G.graph_index.sync_free() and dg.sync_loss_dict
    for p, p0 in zip(params, before):                          # capturing (three warm-up steps, two captures) did not train
        assert torch.equal(p, p0)
    for k, v in dg.state_dict().items():
        assert torch.equal(v, bufs_before[k]), k
    for which, gr in zip(("unmixed", "mixed"), graphs_dbg):
        assert_no_memset_nodes(_dump(gr), "ReplayedDualStep " + which)
    Np, Ep, Edc = cap = ds.pair_capacity_for(dual, B)
    assert rs.capacity == cap
    assert rs.primal_noise.shape == (Np, 1) and rs.dual_noise.shape == (Ep + 2, 1)
    assert [tuple(m.shape) for m in rs.primal_masks] == [(Np, 2 * H), (Np, H)]
    assert [tuple(m.shape) for m in rs.dual_masks] == [(Ep + 2, 2 * H), (Ep + 2, H)]
    opt_of = [opts[0]] * (len(list(mods[0].parameters())) + len(list(mods[1].parameters())))
    opt_of += [opts[1]] * (len(params) - len(opt_of))
    gen = torch.Generator().manual_seed(5)
    for epoch, ids_l in enumerate(po.STEP_IDS):
        N, E, Ed = do.pair_totals(graphs, ids_l)
        rs.primal_noise.copy_(torch.rand(Np, 1, generator=gen).clamp_(1e-10, 1 - 1e-10))       # the caller owns the pinned buffers
        rs.dual_noise.copy_(torch.rand(Ep + 2, 1, generator=gen))
        states = do.state_of(mods)
        pre = [p.detach().clone() for p in params]
        st = [(o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone(), float(o.state[p]["step"])) for p, o in zip(params, opt_of)]
        assert st[0][2] == epoch and st[-1][2] == epoch
        loss = rs.step(np.asarray(ids_l), epoch)
        torch.cuda.synchronize()
        assert rs.batch.valid.tolist() == [N, E, B, 0] and rs.dual_batch.valid.tolist() == [E, Ed, B, 0]
        assert rs.edge_att.shape == (Ep, 1) and rs.clf_logits.shape == (B + 1, 1) and rs.batch.x.shape == (Np, 14)
        r = G.get_r(1, 0.1, epoch, final_r=0.5)
        assert abs(float(rs.r) - r) < 1e-6
        idt = torch.tensor(ids_l, device=dev)
        upb, udb = ds.collate(idt).to("cpu"), dual.collate(idt).to("cpu")
        step_args = (omods, states, upb, udb, epoch > 1, float(np.float32(r)), rs.primal_noise.cpu()[:N], rs.dual_noise.cpu()[:E],
                     [m.cpu()[:N] for m in rs.primal_masks], [m.cpu()[:E] for m in rs.dual_masks])
        r32, r64 = do.oracle_step(*step_args)
        what = f"{backbone} replay {epoch}: "
        if backbone == "PNA":
            r32 = do.widest_fp32_gradients(r32, r64, *step_args)
            for n, a, c in zip(names, r32[3], r64[3]):
                d = float((a.double() - c).abs().max())
                if d > 2e-5:
                    print(what + f"reference fp32 spread of grad {n}: {d:.2e}; device {float((params[names.index(n)].grad.cpu().double() - c).abs().max()):.2e}")
        do.check_step(rs.edge_att, loss, rs.clf_logits, mods, r32, r64, E, B, what)
        for n, p, q32, p0, (m, v, t) in zip(names, params, r32[3], pre, st):
            if q32 is not None:
                close(p, _adam64(p0, p.grad, m, v, t + 1), 1e-6, what=what + "adam " + n)
    G.clear_cache()


# ---- 6. fresh noise, overflow -------------------------------------------------------------------------------------------------------------------
def test_unpinned_replay_draws_noise_and_reports_overflow(dev):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=12)
    omods, mods, dg, opts = _dual_gsat(dev, "GIN", graphs, True)
    N, E, Ed = do.pair_totals(graphs, range(5))
    before = {k: v.detach().clone() for k, v in dg.state_dict().items()}
    with pytest.raises(ValueError, match="do not fit"):
        G.ReplayedDualStep(dg, ds, dual, 5, capacity=(N + 2, E, Ed - 1))
    for k, v in dg.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not G.graph_index.sync_free() and dg.sync_loss_dict
    rs = G.ReplayedDualStep(dg, ds, dual, 5, capacity=(N + 2, E, Ed))
    assert rs.primal_noise is None and rs.dual_masks is None and not rs.overflowed()
    a = float(rs.step([0, 1, 2, 3, 4], 0))
    b = float(rs.step([0, 1, 2, 3, 4], 0))
    assert np.isfinite(a) and np.isfinite(b) and a != b, (a, b)
    assert rs.batch.valid.tolist() == [N, E, 5, 0] and rs.dual_batch.valid.tolist() == [E, Ed, 5, 0] and not rs.overflowed()
    big = [0, 1, 2, 6, 7]
    assert po.totals(graphs, big)[0] > N
    with pytest.raises(ValueError, match="capacity"):
        rs.check_epoch(big)
    rs.check_epoch([0, 1, 2, 3, 4])
    rs.step(big, 0)
    assert rs.batch.valid.tolist() == [0, 0, 5, 1] and rs.dual_batch.valid.tolist() == [0, 0, 5, 1] and torch.isfinite(rs.loss)
    rs.step([0, 1, 2, 3, 4], 0)
    assert rs.overflowed() and not rs.overflowed()
    G.clear_cache()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_padded_pairs_are_refused_where_unsupported(dev):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=12)
    ids = torch.arange(5, device=dev)
    other = G.PackedDataset.from_data_list(do.labelled_graphs(count=12), dev)          # node counts are not ds.edge_counts
    omods, mods, dg, opts = _dual_gsat(dev, "GIN", graphs, True)
    with pytest.raises(ValueError, match="not a dual"):
        G.collate_padded_pair(ds, other, ids)
    with pytest.raises(ValueError, match="not a dual"):
        G.ReplayedDualStep(dg, ds, other, 5)
    pb, db = G.collate_padded_pair(ds, dual, ids)
    lone = dual.collate_padded(ids, db.capacity)
    with pytest.raises(ValueError, match="padded"):                                       # the right shapes, but not a pair
        dg.dual_forward_pass(pb, lone, 0, True)
    plain = lambda i: torch.optim.Adam(list(mods[i].parameters()) + list(mods[i + 1].parameters()))
    mk = lambda po_, do_, **kw: G.DualGSAT(mods[0], mods[1], po_, mods[2], mods[3], do_, do.MCFG, do.MCFG, kw.pop("pe", False),
                                           kw.pop("de", False), **kw).train()
    with pytest.raises(ValueError, match="capturable"):
        G.ReplayedDualStep(mk(plain(0), opts[1]), ds, dual, 5)
    with pytest.raises(ValueError, match="capturable"):
        G.ReplayedDualStep(mk(opts[0], plain(2)), ds, dual, 5)
    for kw in (dict(primal_multi_label=True), dict(dual_multi_label=True)):
        with pytest.raises(ValueError, match="multi-label"):
            G.ReplayedDualStep(mk(opts[0], opts[1], **kw), ds, dual, 5)
        with pytest.raises(ValueError, match="multi-label"):
            mk(None, None, **kw).dual_forward_pass(pb, db, 0, True)
    for kw in (dict(pe=True), dict(de=True)):
        with pytest.raises(ValueError, match="edge attention"):
            mk(None, None, **kw).dual_forward_pass(pb, db, 0, True)
        with pytest.raises(ValueError, match="edge attention"):
            G.ReplayedDualStep(mk(opts[0], opts[1], **kw), ds, dual, 5)
    G.clear_cache()
