"""gpu: the multi-label criterion constructed as capturable -- on unpadded, padded and ragged batches against the torch criterion, inside
ReplayedStep / ReplayedEval / ReplayedFidelityCurve, with per-task scores from EpochLog.compute() -- and what stays refused.  Label
fixtures and the model builder: tests/multitask.py (T = 3, NaNs, one unscorable task, one column unlabelled throughout a batch)."""
import numpy as np
import pytest
import torch

from tests import eval_log_oracle as lo
from tests import fidelity_tasks_oracle as fto
from tests import multitask as mt
from tests import padded_oracle as po
from tests import ragged_oracle as ro
from tests import train_log as tl
from tests.replay import pin_seed_stream, seed_state
from tests.test_gpu_eval_log import FLOAT_KEYS, HITS_KEY, INT_KEYS, _training_state
from tests.test_gpu_fidelity_curve_log import P_RTOL
from tests.test_gpu_ragged import _match
from tests.util import TOL, close

pytestmark = pytest.mark.gpu
SLOTS, CAP = ro.RAGGED_SLOTS, ro.RAGGED_CAPACITY
K = tl.K
T = mt.T
BACKBONES = pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])


# ---- 1. the criterion and its way through forward_pass ---------------------------------------------------------------------------------------
def test_capturable_criterion_equals_the_torch_criterion_on_an_unpadded_batch(dev):
    import dp_gsat_amd as G
    y = torch.from_numpy(mt.task_labels(po.mutag_graphs(**po.LAYOUT_GRAPHS))[po.LAYOUT_IDS]).to(dev)
    assert y.shape == (5, T) and torch.isnan(y).any() and not torch.isnan(y).all()
    z = (torch.randn(5, T, generator=torch.Generator().manual_seed(3)) * 2).to(dev)
    new, old = G.Criterion(T, True, capturable=True), G.Criterion(T, True)
    assert new.capturable is True and old.capturable is False and G.Criterion(2, False).capturable is False
    grads = []
    for crit in (new, old):
        zz = z.clone().requires_grad_(True)
        loss = crit(zz, y)
        loss.backward()
        grads.append((loss.detach(), zz.grad))
    close(grads[0][0], grads[1][0], TOL, what="loss")
    close(grads[0][1], grads[1][1], TOL, what="dlogits")
    # the single-label modes go the same way when asked to
    for num_class, target in ((2, (torch.rand(5, 1, device=dev) < 0.5).float()), (4, torch.randint(0, 4, (5,), device=dev).float())):
        zc = torch.randn(5, 1 if num_class == 2 else num_class, device=dev)
        close(G.Criterion(num_class, False, capturable=True)(zc, target), G.Criterion(num_class, False)(zc, target), TOL, what=f"C={num_class}")
    # the documented deviation: no labelled entry gives 0 and zero gradients where torch gives NaN
    zz = z.clone().requires_grad_(True)
    loss = new(zz, torch.full_like(y, float("nan")))
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(zz.grad.abs().max()) == 0.0 and bool(torch.isnan(old(z, torch.full_like(y, float("nan")))))


def _noise(M_cap, edge, seed=11):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(M_cap, 1, generator=g).clamp_(1e-10, 1 - 1e-10)
    return u, [(torch.rand(M_cap, 4 * mt.H if edge else 2 * mt.H, generator=g) > 0.5).float(), (torch.rand(M_cap, mt.H, generator=g) > 0.5).float()]


def _pred_loss_of(gsat, b, dev, u, masks):
    """(prediction loss with its graph, loss, loss dict) of one training-mode forward_pass: the criterion's output is taken by a hook."""
    taken = []
    hook = gsat.criterion.register_forward_hook(lambda m, i, o: taken.append(o))
    try:
        _, loss, ld, _ = gsat.forward_pass(b, 0, True, noise=u.to(dev), dropout_masks=[m.to(dev) for m in masks])
    finally:
        hook.remove()
    assert len(taken) == 1
    return taken[0], loss, ld


@BACKBONES
def test_forward_pass_on_padded_and_ragged_batches_equals_the_unpadded_pass(dev, backbone, edge):
    """The five graphs of po.LAYOUT_IDS: fixed-count padded, and ragged with 5 filled and 3 empty slots, against the unpadded eager pass
    with the TORCH criterion -- loss and every parameter gradient at the project's tolerance; then all-NaN labels and overflow batches."""
    import dp_gsat_amd as G
    graphs = mt.labelled_graphs(**po.LAYOUT_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = mt.gsat(dev, backbone, edge, graphs, dropout_p=0.0)
    params = [p for _, p in gsat.named_parameters()]
    names = [n for n, _ in gsat.named_parameters()]
    sd = {k: v.detach().clone() for k, v in gsat.state_dict().items()}
    ids = torch.tensor(po.LAYOUT_IDS, device=dev)
    N, E = po.totals(graphs, po.LAYOUT_IDS)
    N_cap, E_cap = cap = ds.capacity_for(8)
    M_cap, M = (E_cap, E) if edge else (N_cap, N)
    u, masks = _noise(M_cap, edge)
    ragged_ids = torch.tensor(po.LAYOUT_IDS + [-1, -1, -1], device=dev)

    def run(b, rows, criterion):
        gsat.load_state_dict(sd)
        gsat.criterion = criterion
        for p in params:
            p.grad = None
        _, loss, ld, logits = gsat.forward_pass(b, 0, True, noise=u[:rows].to(dev), dropout_masks=[m[:rows].to(dev) for m in masks])
        loss.backward()
        return loss.detach(), ld, [None if p.grad is None else p.grad.clone() for p in params], logits.detach()

    capturable = gsat.criterion
    ref_loss, ref_ld, ref_grads, ref_logits = run(ds.collate(ids), M, G.Criterion(T, True))
    assert np.isfinite(ref_ld["pred"]) and ref_ld["pred"] > 0
    cases = {"unpadded": (ds.collate(ids), M), "fixed-count": (ds.collate_padded(ids, cap), M_cap),
             "ragged": (ds.collate_padded(ragged_ids, cap, ragged=True), M_cap)}
    assert cases["fixed-count"][0].valid.tolist() == [N, E, 5, 0] and cases["ragged"][0].valid.tolist() == [N, E, 5, 0]
    assert cases["ragged"][0].num_graphs == 9 and cases["fixed-count"][0].num_graphs == 6
    for what, (b, rows) in cases.items():
        loss, ld, grads, logits = run(b, rows, capturable)
        close(loss, ref_loss, TOL, what=f"{what}: loss")
        assert abs(ld["pred"] - ref_ld["pred"]) <= TOL * max(1.0, abs(ref_ld["pred"])), what
        close(logits[:5], ref_logits, TOL, what=f"{what}: logits")
        for n, g, r in zip(names, grads, ref_grads):
            assert (g is None) == (r is None), (what, n)
            if g is not None:
                close(g, r, TOL, what=f"{what}: grad {n}")
    # labels that are all NaN: a prediction loss of exactly 0 (torch gives NaN)
    gsat.load_state_dict(sd)
    gsat.criterion = capturable
    for what, (b, rows) in cases.items():
        b.y = torch.full_like(b.y, float("nan"))
        pred, loss, ld = _pred_loss_of(gsat, b, dev, u[:rows], [m[:rows] for m in masks])
        assert float(pred.detach()) == 0.0 and ld["pred"] == 0.0 and np.isfinite(ld["loss"]), what
    # overflow batches: a filled slot behind an empty one (ragged), a capacity one node short (fixed-count)
    G.set_sync_free(True)               # outside sync-free mode collate_padded raises instead of marking the batch
    try:
        over = {"ragged": ds.collate_padded(torch.tensor([7, -1, 2], device=dev), cap, ragged=True),
                "fixed-count": ds.collate_padded(ids, (N + 1, E_cap))}
    finally:
        G.set_sync_free(False)
    assert over["ragged"].valid.tolist() == [0, 0, 0, 1] and over["fixed-count"].valid.tolist() == [0, 0, 5, 1]
    for what, b in over.items():
        rows = int(b.edge_index.shape[1]) if edge else int(b.x.shape[0])
        uo, mo = _noise(rows, edge, seed=5)
        assert not torch.isnan(b.y[:b.num_graphs - 1]).all()
        pred, loss, ld = _pred_loss_of(gsat, b, dev, uo, mo)
        assert float(pred.detach()) == 0.0 and ld["pred"] == 0.0, what
        for n, g in zip(names, torch.autograd.grad(pred, params, allow_unused=True)):
            assert g is None or float(g.abs().max()) == 0.0, (what, n)          # zero, not NaN
    G.clear_cache()


# ---- 2. replayed training ---------------------------------------------------------------------------------------------------------------------
def _tensors(gsat):
    opt = gsat.optimizer
    out = {"param." + n: p for n, p in gsat.named_parameters()}
    out.update({"buffer." + n: b for n, b in gsat.named_buffers()})
    for i, p in enumerate(p for grp in opt.param_groups for p in grp["params"]):
        for key, v in opt.state[p].items():
            if isinstance(v, torch.Tensor):
                out[f"adam.{i}.{key}"] = v
    return out


@BACKBONES
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed-count", "ragged"])
def test_three_replays_equal_the_same_bodies_run_eagerly(dev, backbone, edge, ragged):
    """ReplayedStep.step three times, then -- from the same parameters, buffers, Adam state and seed stream -- the body the graph holds
    (run_once) three times without the graph: not a bit differs.  The second ragged batch has task 1 unlabelled throughout."""
    import dp_gsat_amd as G
    graphs = mt.labelled_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = mt.gsat(dev, backbone, edge, graphs)
    if ragged:
        rs = G.ReplayedStep(gsat, ds, SLOTS, capacity=CAP, ragged=True)
        steps = ro.rows_to_lists(rs.batches(range(48)))[:3]
        assert [len(s) for s in steps] == ro.RAGGED_SIZES[:3] and steps[1] == list(mt.NAN_GRAPHS)
    else:
        rs = G.ReplayedStep(gsat, ds, po.STEP_BATCH)
        steps = po.STEP_IDS
    live = _tensors(gsat)
    assert any(k.startswith("adam.") for k in live) and any("running_mean" in k for k in live)
    start = {k: v.detach().clone() for k, v in live.items()}
    pin_seed_stream(dev, 0x5EED)
    losses = []
    for epoch, ids in enumerate(steps):
        losses.append(rs.step(ids, epoch).clone())
        assert rs.batch.valid.tolist()[2:] == [len(ids), 0] and rs.clf_logits.shape[1] == T
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(l)) for l in losses) and not rs.overflowed()
    replayed = {k: v.detach().clone() for k, v in live.items()}
    assert any(not torch.equal(replayed[k], start[k]) for k in live if k.startswith("param."))
    with torch.no_grad():
        for k, v in live.items():
            v.copy_(start[k])
    pin_seed_stream(dev, 0x5EED)
    was = G.graph_index.sync_free()
    G.set_sync_free(True)
    gsat.sync_loss_dict = False
    try:
        for epoch, ids in enumerate(steps):
            rs._load_ids(ids)
            rs.r.fill_(float(rs._r_of(epoch)))
            rs.run_once()
            assert torch.equal(rs.loss, losses[epoch]), epoch
    finally:
        G.set_sync_free(was)
        gsat.sync_loss_dict = True
    torch.cuda.synchronize()
    for k, v in _tensors(gsat).items():
        assert torch.equal(v, replayed[k]), k
    G.clear_cache()


# ---- 3. scores ----------------------------------------------------------------------------------------------------------------------------------
def _check_scores(got, oracle, what):
    want = oracle.compute(multi_label=True)
    _match({k: v for k, v in got.items() if k != "clf_roc_tasks"}, want, what)
    assert set(got) == set(want) | {"clf_roc_tasks"}
    G_logged = int(oracle.state[1])
    per = mt.roc_tasks_oracle(oracle.logits[:G_logged], oracle.y[:G_logged])
    tasks = got["clf_roc_tasks"]
    assert isinstance(tasks, np.ndarray) and tasks.shape == (T,) and tasks.dtype == np.float64
    assert np.array_equal(np.isnan(tasks), np.arange(T) == mt.UNSCORABLE), tasks            # NaN exactly at the unscorable task
    ok = ~np.isnan(per)
    assert np.max(np.abs(tasks[ok] - per[ok])) <= 1e-12
    assert abs(got["clf_roc"] - float(np.mean(tasks[ok]))) <= 1e-12, what                   # the ogb mean over the scorable tasks


@BACKBONES
def test_ragged_evaluation_and_training_log_score_per_task(dev, backbone, edge):
    """ReplayedEval(ragged=True).run and ReplayedStep(ragged=True, log_k=5).epoch_scores() against the oracle's compute(multi_label=True)
    fed the tensors the replays published."""
    import dp_gsat_amd as G
    graphs = mt.labelled_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = mt.gsat(dev, backbone, edge, graphs)
    ev = G.ReplayedEval(gsat, ds, SLOTS, K, capacity=CAP, ragged=True)
    log = ev.log
    assert (log.multi_label, log.logit_cols, log.y_cols, log.max_batches) == (True, T, T, 48)
    got = ev.run(np.arange(48), 1)
    rows = ev.batches(range(48))
    lists = ro.rows_to_lists(rows)
    oracle = lo.LogOracle(K, ds.num_graphs, int(ds.edge_local_all.shape[1]), 48, T, T)
    ev.log.reset()
    for j, ids in enumerate(lists):
        ev.step(rows[j], 1)
        assert ev.batch.valid.tolist()[2:] == [len(ids), 0]
        tl.feed_padded(oracle, ev.edge_att, ev.batch, ev.clf_logits, ev.losses, len(ids))
    _check_scores(got, oracle, f"{backbone}: ragged ReplayedEval.run")
    # the training pass logs itself
    rs = G.ReplayedStep(gsat, ds, SLOTS, capacity=CAP, keep_edge_att=True, ragged=True, log_k=K)
    assert rs.log.multi_label and (rs.log.logit_cols, rs.log.y_cols) == (T, T) and rs.log.state.tolist() == [0, 0, 0, 0]
    rs.begin_epoch()
    oracle = lo.LogOracle(K, ds.num_graphs, int(ds.edge_local_all.shape[1]), 48, T, T)
    for epoch, j in enumerate((1, 4, 0, 2)):
        rs.step(rows[j], epoch)
        torch.cuda.synchronize()
        tl.feed_padded(oracle, rs.edge_att, rs.batch, rs.clf_logits, rs.losses, len(lists[j]))
    _check_scores(rs.epoch_scores(), oracle, f"{backbone}: ragged epoch_scores")
    G.clear_cache()


def test_fixed_count_evaluation_and_training_log_score_per_task(dev):
    """The fixed-count instances: two full batches as replays and the tail of five eagerly (ReplayedEval.run does it itself; the training
    log takes the caller's append)."""
    import dp_gsat_amd as G
    from tests.test_gpu_eval_log import BATCH, EVAL_IDS
    graphs = mt.labelled_graphs(40, self_loop=(5,))
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = mt.gsat(dev, "GIN", True, graphs)
    ev = G.ReplayedEval(gsat, ds, BATCH, K)
    got = ev.run(np.asarray(EVAL_IDS), 0)
    assert ev.log.state.tolist()[1:] == [len(EVAL_IDS), 3, 0] and ev.log.multi_label
    oracle = lo.LogOracle(K, ds.num_graphs, int(ds.edge_local_all.shape[1]), 5, T, T)
    for s in (0, BATCH):
        ev.step(EVAL_IDS[s:s + BATCH], 0)
        tl.feed_padded(oracle, ev.edge_att, ev.batch, ev.clf_logits, ev.losses, BATCH)
    tail = ds.collate(torch.tensor(EVAL_IDS[2 * BATCH:], device=dev))
    gsat.eval()
    try:
        with torch.no_grad():
            att, _, ld, logits = gsat.forward_pass(tail, 0, False)          # unpadded, through the capturable criterion
    finally:
        gsat.train()
    losses = np.array([ld["loss"], ld["pred"], ld["info"]], np.float32)
    oracle.append(tl.cpu(G.ops.edge_tensor(att)), tl.cpu(tail.edge_label), tl.cpu(tail.edge_index), tl.cpu(tail.batch), 5, tl.cpu(logits),
                  tl.cpu(tail.y), losses)
    _check_scores(got, oracle, "fixed-count ReplayedEval.run")
    rs = G.ReplayedStep(gsat, ds, BATCH, keep_edge_att=True, log_k=K)
    rs.begin_epoch()
    oracle = lo.LogOracle(K, ds.num_graphs, int(ds.edge_local_all.shape[1]), 5, T, T)
    for s in (0, BATCH):
        rs.step(EVAL_IDS[s:s + BATCH], 0)
        torch.cuda.synchronize()
        tl.feed_padded(oracle, rs.edge_att, rs.batch, rs.clf_logits, rs.losses, BATCH)
    gsat.sync_loss_dict = False
    try:
        att, loss, ld, logits = gsat.forward_pass(tail, 0, True)
    finally:
        gsat.sync_loss_dict = True
    losses = torch.stack([ld["loss"], ld["pred"], ld["info"]])
    rs.log.append(att, tail, logits, losses)
    oracle.append(tl.cpu(G.ops.edge_tensor(att)), tl.cpu(tail.edge_label), tl.cpu(tail.edge_index), tl.cpu(tail.batch), 5, tl.cpu(logits),
                  tl.cpu(tail.y), tl.cpu(losses))
    _check_scores(rs.epoch_scores(), oracle, "fixed-count epoch_scores")
    G.clear_cache()


def test_single_label_compute_keeps_its_keys(dev):
    import dp_gsat_amd as G
    from tests.test_gpu_eval_log import _random_batch
    keys = set(FLOAT_KEYS) | set(INT_KEYS) | {HITS_KEY, "pr_curve"}
    assert len(keys) == 14
    for multi in (False, True):
        log = G.EpochLog(5, 16, 400, 2, 1, 1, multi_label=multi, device=dev)
        b, att, z = _random_batch([10, 20, 0, 30, 4], 3, dev)
        log.append(att, b, z, torch.rand(3, device=dev))
        res = log.compute()
        assert set(res) == (keys | {"clf_roc_tasks"} if multi else keys)
        if multi:
            assert res["clf_roc_tasks"].shape == (1,) and (np.isnan(res["clf_roc"]) or res["clf_roc_tasks"][0] == res["clf_roc"])
    G.clear_cache()


# ---- 4. the curve -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,edge,levels,ragged", [("GIN", True, dict(ratios=[0.3, 0.7]), True), ("PNA", False, dict(ks=[2, 5]), False)],
                         ids=["GIN-ratios-ragged", "PNA-ks-fixed"])
def test_replayed_curve_of_a_multi_task_model_equals_the_oracle(dev, backbone, edge, levels, ragged):
    import dp_gsat_amd as G
    graphs = mt.labelled_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = mt.gsat(dev, backbone, edge, graphs)
    values = next(iter(levels.values()))
    S, V = len(values), 2 * len(values) + 1
    rc = G.ReplayedFidelityCurve(gsat, ds, SLOTS, capacity=CAP if ragged else None, ragged=ragged, **levels)
    assert rc.log.tasks == T and rc.log.cls.shape == (48, T, V) and rc.log.state.tolist() == [0] * 20
    ids = list(range(48))
    got = rc.run(np.asarray(ids))
    assert got == rc.run(np.asarray(ids))                                                  # bitwise repeatable
    rows = ro.rows_to_lists(rc.batches(ids)) if ragged else [ids[s:s + SLOTS] for s in range(0, 48, SLOTS)]
    assert got["n"] == 48 and rc.log.state.tolist()[:3] == [48, len(rows), 0] and got["levels"] == values
    cls, p, kept, edges = [], [], np.zeros(S, np.int64), 0
    for row in rows:
        rc.step(row, 0)
        sv = rc.stack.valid.cpu().numpy()
        assert rc.logits.shape == (V * (SLOTS + 1), T) and (sv[:, 3] == 0).all() and rc.batch.valid.tolist()[2:] == [len(row), 0]
        c, q = fto.rows(rc.logits.cpu().numpy(), SLOTS + 1, S, len(row), T)
        cls.append(c)
        p.append(q)
        kept += sv[1:1 + S, 1]
        edges += int(sv[0, 1])
    want = fto.compute(np.concatenate(cls), np.concatenate(p), S, kept, edges, values)
    assert set(got) == set(want)
    for key in fto.EXACT_KEYS + ("flip_plus", "flip_minus"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in fto.PROB_KEYS:
        a, b = np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 2 * (P_RTOL + 48 * 2.0 ** -53), (key, got[key], want[key])
    assert np.asarray(got["fidelity_plus_tasks"]).shape == (S, T) and len(got["p_full_tasks"]) == T and not rc.overflowed()
    G.clear_cache()


def test_multi_task_evaluation_and_curve_epochs_do_not_disturb_training(dev):
    """Three ragged training replays with a multi-task evaluation epoch and a curve epoch after each, and the same three without:
    parameters, buffers, Adam state, the device seed state and torch's CUDA generator state are bitwise equal."""
    import dp_gsat_amd as G
    graphs = mt.labelled_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    runs = []
    for with_epochs in (True, False):
        torch.manual_seed(99)
        gsat = mt.gsat(dev, "GIN", True, graphs)
        rs = G.ReplayedStep(gsat, ds, SLOTS, capacity=CAP, ragged=True)
        ev = G.ReplayedEval(gsat, ds, SLOTS, K, capacity=CAP, ragged=True) if with_epochs else None
        rc = G.ReplayedFidelityCurve(gsat, ds, SLOTS, ratios=[0.3, 0.7], capacity=CAP, ragged=True) if with_epochs else None
        pin_seed_stream(dev, 0x5EED)
        rng = torch.cuda.get_rng_state(dev)
        for epoch, row in enumerate(rs.batches(range(48))[:3]):
            rs.step(row, epoch)
            if with_epochs:
                res = ev.run(np.arange(48), epoch)
                curve = rc.run(np.arange(48))
                assert np.isfinite(res["loss"]) and res["clf_roc_tasks"].shape == (T,) and curve["n"] == 48 and gsat.training
        torch.cuda.synchronize()
        assert not rs.overflowed()
        runs.append(_training_state(gsat, dev) + (torch.equal(torch.cuda.get_rng_state(dev), rng),))
    (a, seed_a, rng_a), (b, seed_b, rng_b) = runs
    assert rng_a and rng_b
    assert set(a) == set(b) and any(k.startswith("adam.") for k in a) and any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()


# ---- 5. what stays refused ----------------------------------------------------------------------------------------------------------------------
def test_what_stays_refused(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd.encoders import BatchNorm1d
    graphs = mt.labelled_graphs(**po.LAYOUT_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    good = mt.gsat(dev, "GIN", True, graphs)
    plain = G.GSAT(good.clf, good.extractor, G.Criterion(T, True), good.optimizer, learn_edge_att=True).train()
    ids = torch.tensor(po.LAYOUT_IDS, device=dev)
    batches = (ds.collate_padded(ids, ds.capacity_for(5)), ds.collate_padded(torch.tensor([0, 1, -1], device=dev), ds.capacity_for(3), ragged=True))
    for b in batches:                                                           # without the keyword: refused as before, with the hint
        with pytest.raises(ValueError, match="multi-label.*capturable=True"):
            plain.forward_pass(b, 0, True)
    makers = {"ReplayedStep": lambda m, **kw: G.ReplayedStep(m, ds, 5, **kw), "ReplayedStep(log_k)": lambda m, **kw: G.ReplayedStep(m, ds, 5, log_k=5, **kw),
              "ReplayedEval": lambda m, **kw: G.ReplayedEval(m, ds, 5, 5, **kw),
              "ReplayedFidelityCurve": lambda m, **kw: G.ReplayedFidelityCurve(m, ds, 5, ks=[2], **kw)}
    for name, make in makers.items():
        for ragged in (False, True):
            with pytest.raises(ValueError, match="multi-label.*capturable=True"):
                make(plain, ragged=ragged)
    for model in (plain, good):                                                 # the single-level class refuses the capturable one too
        with pytest.raises(ValueError, match="multi-label"):
            G.ReplayedFidelity(model, ds, 5, k=2)
    with pytest.raises(ValueError, match="ReplayedFidelityCurve"):
        G.ReplayedFidelity(good, ds, 5, k=2)
    H = mt.H
    shared = {"learn_edge_att": False, "extractor_dropout_p": 0.5}
    mcfg = dict(pred_loss_coef=1, info_loss_coef=1, fix_r=False, decay_interval=10, decay_r=0.1, final_r=0.5)
    dual = G.DualGSAT(good.clf, G.ExtractorMLP(H, shared, "primal").to(dev), None, good.clf, G.ExtractorMLP(H, shared, "dual").to(dev), None,
                      mcfg, mcfg, False, False)
    dual.primal_criterion = G.Criterion(T, True, capturable=True)
    dual.dual_criterion = G.Criterion(T, True, capturable=True)
    from dp_gsat_amd.collate import collate_padded_pair
    pds = G.PackedDataset.from_data_list(mt.labelled_graphs(8), dev)               # every graph has an edge: it has a line graph
    dual_ds = pds.line_graph_dataset()
    pb, db = collate_padded_pair(pds, dual_ds, torch.arange(5, device=dev))
    with pytest.raises(ValueError, match="multi-label"):
        dual.dual_forward_pass(pb, db, 0, True)
    for make in (lambda: G.ReplayedDualEval(dual, pds, dual_ds, 5, 5), lambda: G.ReplayedDualFidelityCurve(dual, pds, dual_ds, 5, ks=[2])):
        with pytest.raises(ValueError, match="multi-label"):
            make()
    bns = [m for m in good.modules() if isinstance(m, BatchNorm1d)]
    bns[0].sync_group = True
    try:
        for make in (makers["ReplayedEval"], makers["ReplayedFidelityCurve"]):
            with pytest.raises(ValueError, match="sync_group"):
                make(good)
    finally:
        del bns[0].sync_group
    G.clear_cache()
