"""-m gpu: batches of a ragged graph count -- collate_padded(..., ragged=True) bit-exact against collate, ONE captured training step
replayed on budget batches of 6 to 10 graphs in 16 slots against the oracle's step on the unpadded batch, and ReplayedEval(...,
ragged=True).run without an eager tail against tests/eval_log_oracle.py.  The model builders, the oracle step and the score comparison are
those of tests/test_gpu_padded.py and tests/test_gpu_eval_log.py; floating-point comparisons follow tests.util.close (TOL = 1e-4)."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import eval_log_oracle as lo
from tests import padded_oracle as po
from tests import ragged_oracle as ro
from tests.replay import SeedRecorder, philox_inputs, pin_seed_stream, seed_state
from tests.test_gpu_eval_log import FLOAT_KEYS, HITS_KEY, INT_KEYS, _gsat, _labelled_graphs, _training_state
from tests.test_gpu_padded import H, STREAM_BASE, _adam64, _check_step, _layout_dataset, _models, _oracle_step
from tests.util import TOL, assert_no_memset_nodes, close

pytestmark = pytest.mark.gpu
SLOTS, CAP = ro.RAGGED_SLOTS, ro.RAGGED_CAPACITY


def _debug_graph():
    graph = torch.cuda.CUDAGraph()
    try:
        graph.enable_debug_mode()
    except Exception:
        pass
    return graph


def _dump(graph):
    try:
        path = os.path.join(tempfile.mkdtemp(), "graph.dot")
        graph.debug_dump(path)
        if os.path.exists(path) and os.path.getsize(path) > 0:
            return open(path, errors="replace").read()
    except Exception:
        pass
    return None


# ---- 1. collation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tight", "odd_self_loop", "duplicated", "wide"])
def test_ragged_collation_is_collate_on_the_filled_slots(dev, case):
    graphs, ds = _layout_dataset(dev)
    cap = po.layout_cases()[case]
    slots = po.LAYOUT_IDS + [-1, -1, -1]
    b = ds.collate_padded(torch.tensor(slots, device=dev), cap, ragged=True)
    u = ds.collate(torch.tensor(po.LAYOUT_IDS, device=dev))
    N, E = u.x.shape[0], u.edge_index.shape[1]
    assert b.ragged is True and b.valid.dtype == torch.int32 and b.valid.tolist() == [N, E, 5, 0]
    assert b.num_graphs == 9 and b.capacity == cap and b.y.shape == (9, 1)
    assert torch.equal(b.x[:N], u.x) and torch.equal(b.edge_index[:, :E], u.edge_index) and torch.equal(b.batch[:N], u.batch)
    assert torch.equal(b.y[:5], u.y) and torch.equal(b.edge_attr[:E], u.edge_attr) and torch.equal(b.edge_label[:E], u.edge_label)
    assert not b.x[N:].any() and not b.edge_attr[E:].any() and not b.edge_label[E:].any() and not b.y[5:].any()
    assert int(u.y.abs().sum()) > 0
    assert (b.batch[N:] == 8).all(), "the padding graph is graph B_cap; the empty slots 5..7 own no node"
    # the layout is the oracle's for the real ids with the padding graph renumbered to B_cap
    want = po.collate_padded(graphs, po.LAYOUT_IDS, cap)
    want["batch"][N:] = 8
    for name in ("batch", "node_src_row", "edge_index", "edge_src_slot"):
        assert np.array_equal(getattr(b, name).cpu().numpy(), want[name]), name
    layout = {k: getattr(b, k).cpu().numpy() for k in ("batch", "node_src_row", "edge_index", "edge_src_slot")}
    layout["valid"] = np.array([N, E, 8, 0])                 # check_invariants reads the padding graph's id from valid[2]
    po.check_invariants(layout, cap)
    # the default is untouched: no ragged attribute, the host's graph count
    plain = ds.collate_padded(torch.tensor(po.LAYOUT_IDS, device=dev), cap)
    assert not hasattr(plain, "ragged") and plain.valid.tolist() == [N, E, 5, 0]


def test_ragged_collation_refuses_a_filled_slot_after_an_empty_one(dev):
    import dp_gsat_amd as G
    graphs, ds = _layout_dataset(dev)
    cap = ds.capacity_for(3)
    bad = torch.tensor([7, -1, 2], device=dev)
    with pytest.raises(ValueError, match="does not fit"):
        ds.collate_padded(bad, cap, ragged=True)
    N, E = po.totals(graphs, [7, 2])
    G.set_sync_free(True)
    try:
        b = ds.collate_padded(bad, cap, ragged=True)
        small = ds.collate_padded(torch.tensor([7, 2, -1], device=dev), (N + 1, E), ragged=True)       # one padding node short
        ok = ds.collate_padded(torch.tensor([7, 2, -1], device=dev), (N + 2, E), ragged=True)
        none = ds.collate_padded(torch.tensor([-1, -1, -1], device=dev), cap, ragged=True)
        beyond = ds.collate_padded(torch.tensor([7, 12, -1], device=dev), cap, ragged=True)          # 12 graphs: no graph 12
    finally:
        G.set_sync_free(False)
    assert b.valid.tolist() == [0, 0, 0, 1] and small.valid.tolist() == [0, 0, 0, 1] and beyond.valid.tolist() == [0, 0, 0, 1]
    assert ok.valid.tolist() == [N, E, 2, 0] and none.valid.tolist() == [0, 0, 0, 0]
    for t in (b, small, none, beyond):
        assert not t.x.any() and (t.node_src_row == -1).all() and (t.edge_src_slot == -1).all() and (t.batch == 3).all()
    assert not none.y.any()


@pytest.mark.parametrize("slots", [255, 256, 257, 600])
def test_ragged_scans_carry_across_their_chunks(dev, slots):
    """More slots than one chunk of gsat_ragged_scan (256): repeated ids, the last 1, 2 or 90 slots empty."""
    graphs, ds = _layout_dataset(dev)
    rng = np.random.RandomState(slots)
    empty = 90 if slots == 600 else slots - 254
    ids = rng.randint(0, 12, slots - empty).tolist()
    n_all, e_all = po.sizes(graphs)
    cap = (int(n_all[ids].sum()) + 2, int(e_all[ids].sum()) + 3)
    b = ds.collate_padded(torch.tensor(ids + [-1] * empty, device=dev), cap, ragged=True)
    u = ds.collate(torch.tensor(ids, device=dev))
    N, E = u.x.shape[0], u.edge_index.shape[1]
    assert b.valid.tolist() == [N, E, len(ids), 0] and b.num_graphs == slots + 1
    assert torch.equal(b.x[:N], u.x) and torch.equal(b.edge_index[:, :E], u.edge_index) and torch.equal(b.batch[:N], u.batch)
    assert torch.equal(b.y[:len(ids)], u.y) and not b.y[len(ids):].any() and torch.equal(b.edge_attr[:E], u.edge_attr)
    assert (b.batch[N:] == slots).all() and (b.node_src_row[N:] == -1).all() and (b.edge_src_slot[E:] == -1).all()


# ---- 2. the replayed step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])
def test_one_captured_graph_replays_batches_of_any_graph_count(dev, backbone, edge):
    """ReplayedStep(..., ragged=True) at the capacity (300, 620) with 16 slots: graphs 0..15 do not fit it, so the constructor warms up on
    the first budget batch.  The six budget batches of range(48) (7, 10, 10, 6, 9 and 6 graphs) are replayed at epochs 0..5 and each is
    checked as tests/test_gpu_padded.py checks its replays: loss, attention on the real rows, logits [:b], every gradient, the BatchNorm
    running statistics against the oracle's step on the UNPADDED batch from the pre-step state, the parameters against fp64 Adam."""
    import dp_gsat_amd as G
    graphs = po.mutag_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    cfg, oclf, oext, clf, ext = _models(dev, backbone, edge, graphs)
    params = list(clf.parameters()) + list(ext.parameters())
    names = [n for n, _ in clf.named_parameters()] + ["ext." + n for n, _ in ext.named_parameters()]
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-6, capturable=True, fused=True)
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), opt, learn_edge_att=edge, decay_interval=1).train()
    before = [p.detach().clone() for p in params]
    n16, e16 = po.totals(graphs, range(SLOTS))
    assert n16 + 2 > CAP[0] or e16 > CAP[1], "graphs 0..15 must not fit: the constructor has to cope"
    graph = _debug_graph()
    with SeedRecorder() as rec:
        rs = G.ReplayedStep(gsat, ds, SLOTS, capacity=CAP, keep_edge_att=True, graph=graph, ragged=True)
    assert not G.graph_index.sync_free() and gsat.sync_loss_dict
    for p, p0 in zip(params, before):                        # capturing (three warm-up steps) did not train
        assert torch.equal(p, p0)
    assert_no_memset_nodes(_dump(graph), "ReplayedStep(ragged)")
    pin_seed_stream(dev, STREAM_BASE)
    rows = rs.batches(range(48))
    assert rows.is_cuda and [len(r) for r in ro.rows_to_lists(rows)] == ro.RAGGED_SIZES
    N_cap, E_cap = CAP
    M_cap = E_cap if edge else N_cap
    for epoch, ids in enumerate(ro.rows_to_lists(rows)):
        b = len(ids)
        N, E = po.totals(graphs, ids)
        clf_sd = {k: v.detach().clone().cpu() for k, v in clf.state_dict().items()}
        ext_sd = {k: v.detach().clone().cpu() for k, v in ext.state_dict().items()}
        pre = [p.detach().clone() for p in params]
        st = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), float(opt.state[p]["step"])) for p in params]
        assert st[0][2] == epoch
        base, counter = seed_state(dev)
        loss = rs.step(rows[epoch] if epoch % 2 else ids, epoch)          # a row with its -1s, or just the ids
        torch.cuda.synchronize()
        (word,) = rec.check(base, counter)
        assert rs.batch.valid.tolist() == [N, E, b, 0] and rs.batch.ragged
        assert rs.graph_ids.tolist() == ids + [-1] * (SLOTS - b)
        assert rs.edge_att.shape == (E_cap, 1) and rs.clf_logits.shape == (SLOTS + 1, 1) and rs.batch.x.shape == (N_cap, 14)
        assert abs(float(rs.r) - G.get_r(1, 0.1, epoch, final_r=0.7)) < 1e-6
        ub = ds.collate(torch.tensor(ids, device=dev)).to("cpu")
        assert ub.x.shape[0] == N and ub.edge_index.shape[1] == E
        M = E if edge else N
        masks, u = philox_inputs(word, M_cap, 4 * H if edge else 2 * H, H, 0.5, dev)
        r32, r64 = _oracle_step(oclf, oext, clf_sd, ext_sd, ub, edge, epoch, u[:M], [m[:M] for m in masks], 1)
        what = f"replay {epoch} ({b} graphs): "
        _check_step(rs.edge_att, loss, rs.clf_logits, params, names, clf, r32, r64, E, b, what)
        for n, p, q32, p0, (m, v, t) in zip(names, params, r32[3], pre, st):
            if q32 is not None:
                close(p, _adam64(p0, p.grad, m, v, t + 1), 1e-6, what=what + "adam " + n)
    # a row that does not fit: an all-padding batch without a filled slot, a loss of exactly 0 and no gradient from either loss term
    assert not rs.overflowed()
    loss = rs.step(list(range(SLOTS)), 6)
    torch.cuda.synchronize()
    assert rs.batch.valid.tolist() == [0, 0, 0, 1] and float(loss) == 0.0
    for n, p in zip(names, params):
        assert p.grad is None or not p.grad.any(), n
    assert rs.overflowed() and not rs.overflowed()
    with pytest.raises(ValueError, match="1 to 16"):
        rs.step(list(range(17)), 0)
    with pytest.raises(ValueError, match="1 to 16"):
        rs.step([], 0)
    G.clear_cache()


# ---- 3. the replayed evaluation ----------------------------------------------------------------------------------------------------------------
EVAL_PERM = [33, 5, 12, 0, 27, 39, 8, 19, 2, 30, 31, 7, 22, 14, 36, 9, 11, 3, 25, 38, 17, 41, 1, 46, 20, 6, 44, 28, 15, 35, 10, 43, 4, 24, 47,
             13, 29, 21, 40, 16, 34, 26, 45]


def _match(got, want, what):
    """Every key of the oracle's compute(): the keys that are functions of integer counts exactly, the continuous ones at TOL."""
    assert set(want) <= set(got), set(want) - set(got)
    for key in FLOAT_KEYS:
        assert abs(got[key] - want[key]) <= TOL * max(1.0, abs(want[key])), f"{what}: {key}: {got[key]!r} / {want[key]!r}"
    assert abs(got[HITS_KEY] - want[HITS_KEY]) <= 1e-12, f"{what}: {HITS_KEY}"
    for key in INT_KEYS:
        if isinstance(want[key], np.ndarray):
            assert np.array_equal(got[key], want[key]), f"{what}: {key}"
        else:
            assert abs(got[key] - want[key]) <= 1e-12, f"{what}: {key}: {got[key]!r} / {want[key]!r}"
    for name in ("tp", "fp", "tn", "fn"):
        assert np.array_equal(got["pr_curve"][name], want["pr_curve"][name]), f"{what}: pr_curve {name}"
    assert set(want) == set(FLOAT_KEYS) | set(INT_KEYS) | {HITS_KEY, "pr_curve"}


def _same(a, b):
    assert set(a) == set(b)
    for key, v in a.items():
        if isinstance(v, dict):
            _same(v, b[key])
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, b[key]), key
        else:
            assert v == b[key], key


@pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])
def test_ragged_evaluation_replays_every_batch(dev, backbone, edge):
    import dp_gsat_amd as G
    assert len(EVAL_PERM) == 43 == len(set(EVAL_PERM))
    graphs = _labelled_graphs(48, self_loop=(5,))
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = _gsat(dev, backbone, edge, graphs)
    graph = _debug_graph()
    modes = [m.training for m in gsat.modules()]
    ev = G.ReplayedEval(gsat, ds, SLOTS, 5, capacity=CAP, graph=graph, ragged=True)
    assert [m.training for m in gsat.modules()] == modes and not G.graph_index.sync_free() and gsat.sync_loss_dict
    assert ev.log.state.tolist() == [0, 0, 0, 0] and ev.log.max_batches == 48
    assert_no_memset_nodes(_dump(graph), "ReplayedEval(ragged)")
    rows = ds.budget_batches(EVAL_PERM, CAP, SLOTS)
    lists = ro.rows_to_lists(rows)
    assert len(lists) > 43 // SLOTS + 1 and {len(b) for b in lists} != {SLOTS}
    calls = []
    eager_collate = ds.collate
    ds.collate = lambda *a, **k: calls.append(1) or eager_collate(*a, **k)
    try:
        got = ev.run(np.asarray(EVAL_PERM), 1)
        state = ev.log.state.tolist()
        again = ev.run(np.asarray(EVAL_PERM), 1)
    finally:
        del ds.collate
    assert not calls, "ragged run() must replay every batch: no eager forward"
    assert state[1:] == [43, len(lists), 0], "the number of logged batches is len(budget_batches(...))"
    _same(got, again)
    # the oracle fed the same batches: the replay's own outputs at capacity shape, and the eager unpadded forward next to them
    oracle = lo.LogOracle(5, ds.num_graphs, int(ds.edge_local_all.shape[1]), 48, 1)
    cpu = lambda t: t.detach().cpu().numpy()
    ev.log.reset()
    gsat.eval()
    try:
        for j, ids in enumerate(lists):
            ev.step(rows[j], 1)
            pb = ev.batch
            N, E = po.totals(graphs, ids)
            assert pb.valid.tolist() == [N, E, len(ids), 0]
            oracle.append(cpu(ev.edge_att), cpu(pb.edge_label), cpu(pb.edge_index), cpu(pb.batch), SLOTS + 1, cpu(ev.clf_logits), cpu(pb.y),
                          cpu(ev.losses), real_graphs=len(ids))
            with torch.no_grad():
                ub = ds.collate(torch.tensor(ids, device=dev))
                att, _, ld, logits = gsat.forward_pass(ub, 1, False)
            what = f"batch {j} ({len(ids)} graphs): "
            close(ev.edge_att[:E], G.ops.edge_tensor(att), TOL, what=what + "edge_att")
            close(ev.clf_logits[:len(ids)], logits, TOL, what=what + "clf_logits")
            close(ev.losses, torch.tensor([ld["loss"], ld["pred"], ld["info"]]), TOL, what=what + "losses")
    finally:
        gsat.train()
    _match(got, oracle.compute(), "ragged run against the oracle")
    G.clear_cache()


def test_ragged_evaluation_does_not_disturb_ragged_training(dev):
    """Three ragged training replays (the first budget batches of EVAL_PERM backwards, one cut to four graphs) with a ragged evaluation epoch
    after each, and the same three without: parameters, BatchNorm buffers, Adam state and the device seed counter are bitwise equal."""
    import dp_gsat_amd as G
    graphs = _labelled_graphs(48, self_loop=(5,))
    ds = G.PackedDataset.from_data_list(graphs, dev)
    runs = []
    train_rows = ro.rows_to_lists(ds.budget_batches(EVAL_PERM[::-1], CAP, SLOTS))[:3]
    train_rows[1] = train_rows[1][:4]
    assert len({len(r) for r in train_rows}) == 3
    for with_eval in (True, False):
        torch.manual_seed(99)
        gsat = _gsat(dev, "GIN", True, graphs)
        rs = G.ReplayedStep(gsat, ds, SLOTS, capacity=CAP, ragged=True)
        ev = G.ReplayedEval(gsat, ds, SLOTS, 5, capacity=CAP, ragged=True) if with_eval else None
        pin_seed_stream(dev, 0x5EED)
        for epoch, ids in enumerate(train_rows):
            rs.step(ids, epoch)
            assert rs.batch.valid.tolist()[2:] == [len(ids), 0]
            if ev is not None:
                res = ev.run(np.asarray(EVAL_PERM), epoch)
                assert np.isfinite(res["loss"]) and gsat.training
        torch.cuda.synchronize()
        assert not rs.overflowed()
        runs.append(_training_state(gsat, dev))
    (a, seed_a), (b, seed_b) = runs
    assert set(a) == set(b) and any(k.startswith("adam.") for k in a) and any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()


def test_ragged_keywords_leave_the_defaults_alone(dev):
    """Without ragged=True: a wrong id count is refused as before, and the multi-label criterion stays refused on ragged batches too."""
    import dp_gsat_amd as G
    graphs = _labelled_graphs(12)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = _gsat(dev, "GIN", True, graphs)
    rs = G.ReplayedStep(gsat, ds, 5)
    assert rs.ragged is False and rs.graph_ids.tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="captured for 5"):
        rs.step([0, 1, 2], 0)
    b = ds.collate_padded(torch.tensor([0, 1, -1], device=dev), ds.capacity_for(3), ragged=True)
    multi = G.GSAT(gsat.clf, gsat.extractor, G.Criterion(2, True), None, learn_edge_att=True).train()
    with pytest.raises(ValueError, match="multi-label"):
        multi.forward_pass(b, 0, True)
    with pytest.raises(ValueError, match="multi-label"):
        G.ReplayedStep(G.GSAT(gsat.clf, gsat.extractor, G.Criterion(2, True), gsat.optimizer, learn_edge_att=True), ds, 5, ragged=True)
    with pytest.raises(ValueError, match="graph 0"):
        G.ReplayedStep(gsat, ds, 5, capacity=(4, 4), ragged=True)
    G.clear_cache()
