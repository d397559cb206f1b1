"""-m gpu: the dual/primal pair on batches of a ragged graph count -- collate_padded_pair(..., ragged=True) bit-exact against collate with
its joint verdict from gsat_ragged_pair_scan, ReplayedDualStep(..., ragged=True) replayed on the seven three-budget batches of
tests/ragged_pair_oracle.py against the oracle's DualGSAT step on the UNPADDED pair, and ReplayedDualEval(..., ragged=True).run without an
eager tail against tests/eval_log_oracle.py.  Builders, oracle step and score comparisons are those of tests/test_gpu_dual_replay.py,
tests/test_gpu_dual_eval.py and tests/test_gpu_ragged.py; floating-point comparisons follow tests.util.close (TOL = 1e-4) and
tests.dual_oracle.check_step / widest_fp32_gradients."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import dual_oracle as do
from tests import eval_log_oracle as lo
from tests import padded_oracle as po
from tests import ragged_oracle as ro
from tests import ragged_pair_oracle as rp
from tests.replay import pin_seed_stream, seed_next_ref, seed_state
from tests.test_gpu_dual_eval import BASE, DUAL_KEYS, MIX, _debug_graphs, _reported_noise, _same_result, _set_counter
from tests.test_gpu_dual_replay import _dual_gsat, _dump, _pair_datasets
from tests.test_gpu_eval_log import HITS_KEY, _training_state
from tests.test_gpu_padded import _adam64
from tests.test_gpu_ragged import EVAL_PERM, _match
from tests.util import TOL, assert_no_memset_nodes, close

pytestmark = pytest.mark.gpu
SLOTS, CAP = rp.PAIR_SLOTS, rp.PAIR_CAPACITY
H = do.H
LAYOUT_IDS = po.LAYOUT_IDS[:1] + [3] + po.LAYOUT_IDS[2:]        # the ids of test_collate_padded_pair_layout
TENSORS = ("x", "edge_index", "batch", "y", "node_src_row", "edge_src_slot", "valid")


def _all_padding(b, slots):
    return not b.x.any() and bool((b.batch == slots).all()) and bool((b.node_src_row == -1).all()) and bool((b.edge_src_slot == -1).all())


# ---- 1. layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("room", [(0, 0, 0), (7, 3, 5)], ids=["exact-fit", "roomier"])
def test_ragged_pair_is_collate_on_the_filled_slots(dev, room):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=12)
    N, E, Ed = do.pair_totals(graphs, LAYOUT_IDS)
    cap = (N + 2 + room[0], E + room[1], Ed + room[2])
    slots = torch.tensor(LAYOUT_IDS + [-1, -1, -1], device=dev)
    ids = torch.tensor(LAYOUT_IDS, device=dev)
    pb, db = G.collate_padded_pair(ds, dual, slots, cap, ragged=True)
    up, ud = ds.collate(ids), dual.collate(ids)
    assert pb.pair is db and db.pair is pb and pb.ragged is True and db.ragged is True
    assert pb.num_graphs == 9 and db.num_graphs == 9 and pb.capacity == cap[:2] and db.capacity == (cap[1] + 2, cap[2])
    assert pb.valid.dtype == torch.int32 and pb.valid.tolist() == [N, E, 5, 0] and db.valid.tolist() == [E, Ed, 5, 0]
    assert torch.equal(db.node_src_row[:E], pb.edge_src_slot[:E])
    for b, u, n, e in ((pb, up, N, E), (db, ud, E, Ed)):
        assert torch.equal(b.x[:n], u.x) and torch.equal(b.edge_index[:, :e], u.edge_index) and torch.equal(b.batch[:n], u.batch)
        assert torch.equal(b.y[:5], u.y) and not b.y[5:].any() and not b.x[n:].any() and b.y.shape == (9, 1)
        assert bool((b.batch[n:] == 8).all()), "the padding graph is graph B; the empty slots 5..7 own no node"
        solo_ds = ds if b is pb else dual
        solo = solo_ds.collate_padded(slots, b.capacity, ragged=True)
        for name in ("batch", "node_src_row", "edge_index", "edge_src_slot", "valid"):
            assert torch.equal(getattr(b, name), getattr(solo, name)), name
        layout = {k: getattr(b, k).cpu().numpy() for k in ("batch", "node_src_row", "edge_index", "edge_src_slot")}
        layout["valid"] = np.array([n, e, 8, 0])             # check_invariants reads the padding graph's id from valid[2]
        po.check_invariants(layout, b.capacity)
    assert int(up.y.abs().sum()) > 0
    assert torch.equal(pb.edge_label[:E], up.edge_label) and not pb.edge_label[E:].any()
    # with every slot filled the ragged pair is the fixed-count pair, bit for bit
    rpb, rdb = G.collate_padded_pair(ds, dual, ids, cap, ragged=True)
    fpb, fdb = G.collate_padded_pair(ds, dual, ids, cap)
    assert not hasattr(fpb, "ragged") and not hasattr(fdb, "ragged")
    for r, f in ((rpb, fpb), (rdb, fdb)):
        for name in TENSORS:
            assert torch.equal(getattr(r, name), getattr(f, name)), name
        assert r.num_graphs == f.num_graphs == 6 and r.capacity == f.capacity
    assert torch.equal(rpb.edge_label, fpb.edge_label)
    # capacity=None is the bound for the slot count
    bpb, bdb = G.collate_padded_pair(ds, dual, slots, ragged=True)
    bound = ds.pair_capacity_for(dual, 8)
    assert bpb.capacity == bound[:2] and bdb.capacity == (bound[1] + 2, bound[2]) and bpb.valid.tolist() == [N, E, 5, 0]
    G.clear_cache()


# ---- 2. the joint verdict ------------------------------------------------------------------------------------------------------------------
def test_the_verdict_is_joint_and_stays_on_the_device(dev):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=12)
    N, E, Ed = do.pair_totals(graphs, [7, 2])
    fit = (N + 2, E, Ed)
    t = lambda *ids: torch.tensor(list(ids), device=dev)
    with pytest.raises(ValueError, match="does not fit"):
        G.collate_padded_pair(ds, dual, t(7, 2, -1), (N + 2, E, Ed - 1), ragged=True)
    with pytest.raises(ValueError, match="does not fit"):
        G.collate_padded_pair(ds, dual, t(7, -1, 2), fit, ragged=True)
    G.set_sync_free(True)
    try:
        ok = G.collate_padded_pair(ds, dual, t(7, 2, -1), fit, ragged=True)
        spoiled = {"nodes one short": G.collate_padded_pair(ds, dual, t(7, 2, -1), (N + 1, E, Ed), ragged=True),
                   "edges one short": G.collate_padded_pair(ds, dual, t(7, 2, -1), (N + 2, E - 1, Ed), ragged=True),
                   "dual edges one short": G.collate_padded_pair(ds, dual, t(7, 2, -1), (N + 2, E, Ed - 1), ragged=True),
                   "filled behind empty": G.collate_padded_pair(ds, dual, t(7, -1, 2), fit, ragged=True),
                   "no graph 12": G.collate_padded_pair(ds, dual, t(7, 12, -1), ds.pair_capacity_for(dual, 3), ragged=True)}
        none = G.collate_padded_pair(ds, dual, t(-1, -1, -1), fit, ragged=True)
    finally:
        G.set_sync_free(False)
    assert ok[0].valid.tolist() == [N, E, 2, 0] and ok[1].valid.tolist() == [E, Ed, 2, 0]
    for what, (pb, db) in spoiled.items():
        assert pb.valid.tolist() == [0, 0, 0, 1] and db.valid.tolist() == [0, 0, 0, 1], what
        assert _all_padding(pb, 3) and _all_padding(db, 3), what
        for b in (pb, db):
            po.check_invariants(dict(valid=np.array([0, 0, 3, 1]), edge_index=b.edge_index.cpu().numpy(), batch=b.batch.cpu().numpy(),
                                     node_src_row=b.node_src_row.cpu().numpy(), edge_src_slot=b.edge_src_slot.cpu().numpy()), b.capacity)
    assert none[0].valid.tolist() == [0, 0, 0, 0] and none[1].valid.tolist() == [0, 0, 0, 0]
    assert _all_padding(none[0], 3) and _all_padding(none[1], 3) and not none[0].y.any() and not none[1].y.any()
    G.clear_cache()


# ---- 3. the scans' carries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [255, 256, 257, 600])
def test_pair_scans_carry_across_their_chunks(dev, slots):
    """More slots than one chunk of gsat_ragged_pair_scan (256): repeated ids, the last 1, 2 or 90 slots empty; all three scans are read
    through the collated pair."""
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=12)
    rng = np.random.RandomState(slots)
    empty = 90 if slots == 600 else slots - 254
    ids = rng.randint(0, 12, slots - empty).tolist()
    N, E, Ed = do.pair_totals(graphs, ids)
    pb, db = G.collate_padded_pair(ds, dual, torch.tensor(ids + [-1] * empty, device=dev), (N + 2, E + 3, Ed + 1), ragged=True)
    idt = torch.tensor(ids, device=dev)
    assert pb.valid.tolist() == [N, E, len(ids), 0] and db.valid.tolist() == [E, Ed, len(ids), 0] and pb.num_graphs == slots + 1
    for b, u, n, e in ((pb, ds.collate(idt), N, E), (db, dual.collate(idt), E, Ed)):
        assert torch.equal(b.x[:n], u.x) and torch.equal(b.edge_index[:, :e], u.edge_index) and torch.equal(b.batch[:n], u.batch)
        assert torch.equal(b.y[:len(ids)], u.y) and not b.y[len(ids):].any()
        assert bool((b.batch[n:] == slots).all()) and bool((b.node_src_row[n:] == -1).all()) and bool((b.edge_src_slot[e:] == -1).all())
    assert torch.equal(db.node_src_row[:E], pb.edge_src_slot[:E])
    # one dual edge short, decided behind the last chunk
    G.set_sync_free(True)
    try:
        sp, sd = G.collate_padded_pair(ds, dual, torch.tensor(ids + [-1] * empty, device=dev), (N + 2, E + 3, Ed - 1), ragged=True)
    finally:
        G.set_sync_free(False)
    assert sp.valid.tolist() == [0, 0, 0, 1] and sd.valid.tolist() == [0, 0, 0, 1]
    G.clear_cache()


# ---- 4. the replayed training step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", ["GIN", "PNA"])
def test_two_captured_graphs_replay_pairs_of_any_graph_count(dev, backbone):
    """ReplayedDualStep(pinned=True, ragged=True, mix_after_epoch=3, dual decay_interval=1) at the capacity (320, 620, 1000) with 16 slots:
    graphs 0..15 do not fit it, so the constructor warms up on the first three-budget batch.  The seven batches of range(48) (7, 9, 10, 5, 9,
    7 and 1 graphs) are replayed at epochs 0..6 -- four on the unmixed graph, three on the mixed one, which gets the one-graph batch -- and
    each is checked as tests/test_gpu_dual_replay.py checks its replays, against the oracle's step on the UNPADDED pair."""
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, **po.STEP_GRAPHS)
    omods, mods, dg, opts = _dual_gsat(dev, backbone, graphs, True, mix_after_epoch=3, dual_cfg=dict(decay_interval=1))
    names, params = do.names_and_params(mods)
    before = {k: v.detach().clone() for k, v in dg.state_dict().items()}
    n16, e16, d16 = do.pair_totals(graphs, range(SLOTS))
    assert n16 + 2 > CAP[0], "graphs 0..15 must not fit: the constructor has to cope"
    dbg = _debug_graphs()
    rs = G.ReplayedDualStep(dg, ds, dual, SLOTS, capacity=CAP, pinned=True, keep_edge_att=True, graphs=dbg, ragged=True)
    assert rs.ragged and not G.graph_index.sync_free() and dg.sync_loss_dict
    for k, v in dg.state_dict().items():                       # capturing (three warm-up steps, two captures) did not train
        assert torch.equal(v, before[k]), k
    for which, gr in zip(("unmixed", "mixed"), dbg):
        assert_no_memset_nodes(_dump(gr), "ReplayedDualStep(ragged) " + which)
    Np, Ep, Edc = CAP
    assert rs.capacity == CAP and rs.primal_noise.shape == (Np, 1) and rs.dual_noise.shape == (Ep + 2, 1)
    rows = rs.batches(range(48))
    lists = ro.rows_to_lists(rows)
    assert rows.is_cuda and [len(r) for r in lists] == rp.PAIR_SIZES
    assert rs.graph_ids.tolist() == lists[0] + [-1] * (SLOTS - len(lists[0]))
    opt_of = [opts[0]] * (len(list(mods[0].parameters())) + len(list(mods[1].parameters())))
    opt_of += [opts[1]] * (len(params) - len(opt_of))
    gen = torch.Generator().manual_seed(5)
    for epoch, ids in enumerate(lists):
        b = len(ids)
        N, E, Ed = do.pair_totals(graphs, ids)
        rs.primal_noise.copy_(torch.rand(Np, 1, generator=gen).clamp_(1e-10, 1 - 1e-10))       # the caller owns the pinned buffers
        rs.dual_noise.copy_(torch.rand(Ep + 2, 1, generator=gen))
        states = do.state_of(mods)
        pre = [p.detach().clone() for p in params]
        st = [(o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone(), float(o.state[p]["step"])) for p, o in zip(params, opt_of)]
        assert st[0][2] == epoch and st[-1][2] == epoch
        loss = rs.step(rows[epoch] if epoch % 2 else ids, epoch)          # a row with its -1s, or just the ids
        torch.cuda.synchronize()
        assert rs.batch.valid.tolist() == [N, E, b, 0] and rs.dual_batch.valid.tolist() == [E, Ed, b, 0]
        assert rs.batch.ragged and rs.dual_batch.ragged and rs.graph_ids.tolist() == ids + [-1] * (SLOTS - b)
        assert rs.edge_att.shape == (Ep, 1) and rs.clf_logits.shape == (SLOTS + 1, 1) and rs.batch.x.shape == (Np, 14)
        r = G.get_r(1, 0.1, epoch, final_r=0.5)
        assert abs(float(rs.r) - r) < 1e-6
        idt = torch.tensor(ids, device=dev)
        upb, udb = ds.collate(idt).to("cpu"), dual.collate(idt).to("cpu")
        step_args = (omods, states, upb, udb, epoch > 3, float(np.float32(r)), rs.primal_noise.cpu()[:N], rs.dual_noise.cpu()[:E],
                     [m.cpu()[:N] for m in rs.primal_masks], [m.cpu()[:E] for m in rs.dual_masks])
        r32, r64 = do.oracle_step(*step_args)
        what = f"{backbone} replay {epoch} ({b} graphs): "
        if backbone == "PNA":
            r32 = do.widest_fp32_gradients(r32, r64, *step_args)
        print(what, "loss", float(loss), "oracle", float(r64[1]))
        do.check_step(rs.edge_att, loss, rs.clf_logits, mods, r32, r64, E, b, what)
        for n, p, q32, p0, (m, v, t) in zip(names, params, r32[3], pre, st):
            if q32 is not None:
                close(p, _adam64(p0, p.grad, m, v, t + 1), 1e-6, what=what + "adam " + n)
    # a row that does not fit: both batches are all padding without a filled slot, and the replay still runs
    assert not rs.overflowed()
    loss = rs.step(list(range(SLOTS)), 7)
    torch.cuda.synchronize()
    assert rs.batch.valid.tolist() == [0, 0, 0, 1] and rs.dual_batch.valid.tolist() == [0, 0, 0, 1] and bool(torch.isfinite(loss))
    assert rs.overflowed() and not rs.overflowed()
    with pytest.raises(ValueError, match="1 to 16"):
        rs.step(list(range(17)), 0)
    with pytest.raises(ValueError, match="1 to 16"):
        rs.step([], 0)
    G.clear_cache()


# ---- 5. the replayed evaluation ------------------------------------------------------------------------------------------------------------
def test_ragged_dual_evaluation_replays_every_batch(dev):
    import dp_gsat_amd as G
    assert len(EVAL_PERM) == 43 == len(set(EVAL_PERM))
    graphs, ds, dual = _pair_datasets(dev, **po.STEP_GRAPHS)
    omods, mods, dg, _ = _dual_gsat(dev, "GIN", graphs, False, **MIX)
    modes = [m.training for m in dg.modules()]
    dbg = _debug_graphs()
    ev = G.ReplayedDualEval(dg, ds, dual, SLOTS, 5, capacity=CAP, score_dual=True, seed=BASE, graphs=dbg, ragged=True)
    assert [m.training for m in dg.modules()] == modes and not G.graph_index.sync_free() and dg.sync_loss_dict
    assert ev.ragged and ev.log.state.tolist() == [0, 0, 0, 0] and ev.dual_log.state.tolist() == [0, 0, 0, 0]
    assert ev.log.max_batches == 48 and ev.dual_log.max_batches == 48 and ev.seed_state.tolist() == [BASE, 0]
    for which, gr in zip(("unmixed", "mixed"), dbg):
        assert_no_memset_nodes(_dump(gr), "ReplayedDualEval(ragged) " + which)
    rows = ev.batches(EVAL_PERM)
    lists = ro.rows_to_lists(rows)
    n, e, d = rp.pair_sizes(graphs)
    assert lists == rp.budget_batches(n, e, d, EVAL_PERM, CAP, SLOTS)[0]
    assert len(lists) > 43 // SLOTS + 1 and {len(b) for b in lists} != {SLOTS}
    cpu = lambda t: t.detach().cpu().numpy()
    Ep = CAP[1]
    for epoch in (0, 2):                                        # the unmixed and the mixed graph
        calls = []
        eager = {id(s): s.collate for s in (ds, dual)}
        for s in (ds, dual):
            s.collate = lambda *a, _f=eager[id(s)], **k: calls.append(1) or _f(*a, **k)
        try:
            got = ev.run(np.asarray(EVAL_PERM), epoch)
            state, dual_state = ev.log.state.tolist(), ev.dual_log.state.tolist()
            again = ev.run(np.asarray(EVAL_PERM), epoch)
        finally:
            del ds.collate, dual.collate
        assert not calls, "ragged run() must replay every batch: no eager forward"
        assert state[1:] == [43, len(lists), 0] and dual_state == state
        assert ev.seed_state.tolist() == [BASE, (epoch << 32) + len(lists)]
        _same_result(got, again)
        # the oracles fed the same batches: the replays' own outputs at capacity shape, and the eager unpadded forward next to them
        oracle, oracle_d = (lo.LogOracle(5, ds.num_graphs, int(ds.edge_local_all.shape[1]), 48, 1) for _ in range(2))
        dg.eval()
        try:
            for j, ids in enumerate(lists):
                _set_counter(ev, (epoch << 32) + j)               # the word run() drew for batch j
                ev.step(rows[j], epoch)
                pb, b = ev.batch, len(ids)
                N, E, Ed = do.pair_totals(graphs, ids)
                assert pb.valid.tolist() == [N, E, b, 0] and ev.dual_batch.valid.tolist() == [E, Ed, b, 0]
                assert ev.edge_att.shape == (Ep, 1) and ev.dual_att.shape == (Ep, 1) and ev.clf_logits.shape == (SLOTS + 1, 1)
                for orc, att in ((oracle, ev.edge_att), (oracle_d, ev.dual_att)):
                    orc.append(cpu(att), cpu(pb.edge_label), cpu(pb.edge_index), cpu(pb.batch), SLOTS + 1, cpu(ev.clf_logits), cpu(pb.y),
                               cpu(ev.losses), real_graphs=b)
                with torch.no_grad():
                    idt = torch.tensor(ids, device=dev)
                    ub, ud = ds.collate(idt), dual.collate(idt)
                    U = _reported_noise(seed_next_ref(BASE, (epoch << 32) + j), E, dev)
                    att, _, ld, logits = dg.dual_forward_pass(ub, ud, epoch, False, dual_noise=U)
                what = f"epoch {epoch} batch {j} ({b} graphs): "
                close(ev.edge_att[:E], G.ops.edge_tensor(att), TOL, what=what + "edge_att")
                close(ev.clf_logits[:b], logits, TOL, what=what + "clf_logits")
                close(ev.losses, torch.tensor([ld["loss"], ld["pred"], ld["info"]]), TOL, what=what + "losses")
        finally:
            dg.train()
        _match(got, oracle.compute(), f"epoch {epoch}: ragged run against the oracle")
        want = oracle_d.compute()
        for key in DUAL_KEYS:
            exact = key in ("att_auroc", HITS_KEY)                # functions of integer counts
            assert abs(got["dual_" + key] - want[key]) <= (1e-12 if exact else TOL * max(1.0, abs(want[key]))), (epoch, key)
    G.clear_cache()


# ---- 6. evaluation does not disturb training -------------------------------------------------------------------------------------------------
def test_ragged_dual_evaluation_does_not_disturb_ragged_dual_training(dev):
    """Three unpinned ragged training replays (three-budget batches of EVAL_PERM backwards, one cut to four graphs, the third on the mixed
    graph) with a ragged evaluation epoch after each, and the same three without: parameters, BatchNorm buffers, both Adam states and the
    device seed counter are bitwise equal."""
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, **po.STEP_GRAPHS)
    train_rows = ro.rows_to_lists(ds.budget_batches(EVAL_PERM[::-1], CAP, SLOTS, dual=dual))[:3]
    train_rows[1] = train_rows[1][:4]
    assert len({len(r) for r in train_rows}) == 3
    runs = []
    for with_eval in (True, False):
        torch.manual_seed(99)
        omods, mods, dg, opts = _dual_gsat(dev, "GIN", graphs, True, **MIX)
        rs = G.ReplayedDualStep(dg, ds, dual, SLOTS, capacity=CAP, ragged=True)
        ev = G.ReplayedDualEval(dg, ds, dual, SLOTS, 5, capacity=CAP, ragged=True) if with_eval else None
        pin_seed_stream(dev, 0x5EED)
        for epoch, ids in enumerate(train_rows):
            rs.step(ids, epoch)
            assert rs.batch.valid.tolist()[2:] == [len(ids), 0]
            if ev is not None:
                res = ev.run(np.asarray(EVAL_PERM), epoch)
                assert np.isfinite(res["loss"]) and dg.training
        torch.cuda.synchronize()
        assert not rs.overflowed()
        state = {}
        for side, opt in (("primal", opts[0]), ("dual", opts[1])):
            got, _ = _training_state(NS(optimizer=opt, named_parameters=dg.named_parameters, named_buffers=dg.named_buffers), dev)
            state.update({side + "." + k if k.startswith("adam.") else k: v for k, v in got.items()})
        runs.append((state, seed_state(dev)))
    (a, seed_a), (b, seed_b) = runs
    assert set(a) == set(b) and any(k.startswith("primal.adam.") for k in a) and any(k.startswith("dual.adam.") for k in a)
    assert any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()


# ---- 7. defaults and refusals ------------------------------------------------------------------------------------------------------------------
def test_ragged_pair_keywords_leave_the_defaults_alone(dev):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=12)
    omods, mods, dg, opts = _dual_gsat(dev, "GIN", graphs, True)
    rs = G.ReplayedDualStep(dg, ds, dual, 5)
    assert rs.ragged is False and rs.graph_ids.tolist() == [0, 1, 2, 3, 4] and rs.capacity == ds.pair_capacity_for(dual, 5)
    with pytest.raises(ValueError, match="captured for 5"):
        rs.step([0, 1, 2], 0)
    assert torch.equal(rs.batches(range(12)), ds.budget_batches(range(12), rs.capacity, 5, dual=dual))
    ids = torch.tensor([0, 1, 2, -1, -1], device=dev)
    cap = ds.pair_capacity_for(dual, 5)
    pb, db = G.collate_padded_pair(ds, dual, ids, cap, ragged=True)
    fpb, fdb = G.collate_padded_pair(ds, dual, torch.arange(5, device=dev), cap)
    pb.pair, fdb.pair = fdb, pb                                 # the right shapes and linked, but only one side is ragged
    with pytest.raises(ValueError, match="one side is ragged"):
        dg.dual_forward_pass(pb, fdb, 0, True)
    pb.pair = db
    mk = lambda po_, do_, **kw: G.DualGSAT(mods[0], mods[1], po_, mods[2], mods[3], do_, do.MCFG, do.MCFG, kw.pop("pe", False),
                                           kw.pop("de", False), **kw).train()
    for kw in (dict(primal_multi_label=True), dict(dual_multi_label=True)):
        with pytest.raises(ValueError, match="multi-label"):
            mk(None, None, **kw).dual_forward_pass(pb, db, 0, True)
        with pytest.raises(ValueError, match="multi-label"):
            G.ReplayedDualStep(mk(opts[0], opts[1], **kw), ds, dual, 5, ragged=True)
        with pytest.raises(ValueError, match="multi-label"):
            G.ReplayedDualEval(mk(None, None, **kw), ds, dual, 5, 5, ragged=True)
    for kw in (dict(pe=True), dict(de=True)):
        with pytest.raises(ValueError, match="edge attention"):
            mk(None, None, **kw).dual_forward_pass(pb, db, 0, True)
        with pytest.raises(ValueError, match="edge attention"):
            G.ReplayedDualStep(mk(opts[0], opts[1], **kw), ds, dual, 5, ragged=True)
    with pytest.raises(ValueError, match="graph 0"):            # no graph fits: budget batching says so before anything is captured
        G.ReplayedDualStep(dg, ds, dual, 5, capacity=(4, 4, 4), ragged=True)
    G.clear_cache()
