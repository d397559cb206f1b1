"""-m gpu: ReplayedClfStep / ReplayedClfEval -- the ERM step and the evaluation of a bare backbone as replays of one captured hipGraph.
24 random graphs of 5 to 12 nodes (tests/graphs.py); GIN, H = 16, two layers, dropout 0 unless a case says otherwise.  Padded against
unpadded arithmetic is compared at tests.util.TOL (``close``), the bound the padded tests use for forwards and gradients alike; a replay
against the same body run eagerly, and everything that says 'does not change training', bit for bit."""
from contextlib import contextmanager
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import clf_log_oracle as co
from tests.graphs import random_batch
from tests.util import TOL, close

pytestmark = pytest.mark.gpu
H, X_DIM, T, BATCH = 16, 10, 3, 8
COUNT = 24


def clf_graphs(count=COUNT, seed=3, tasks=None):
    """``count`` graphs of 5 to 12 nodes: random float features, y [1, 1] in {0, 1} or, ``tasks``, [1, tasks] in {0, 1, NaN}."""
    ei, batch, _ = random_batch(seed, count, 5, 12, isolated=False)
    rng = np.random.RandomState(seed + 1)
    out = []
    for g in range(count):
        nodes = torch.nonzero(batch == g).reshape(-1)
        mine = ei[:, batch[ei[0]] == g] - int(nodes[0])
        n = int(nodes.numel())
        if tasks is None:
            y = torch.tensor([[float(rng.rand() < 0.5)]])
        else:
            y = (rng.rand(1, tasks) < 0.5).astype(np.float32)
            y[rng.rand(1, tasks) < 0.2] = np.nan
            y = torch.from_numpy(y)
        out.append(NS(x=torch.from_numpy(rng.randn(n, X_DIM).astype(np.float32)), edge_index=mine.contiguous(), y=y, edge_attr=None,
                      edge_label=None))
    return out


def clf_model(dev, graphs, backbone="GIN", tasks=None, dropout_p=0.0, lr=1e-2, capturable=True):
    """(model, criterion, optimizer): the backbone alone, as src/pretrain_clf.py trains it."""
    import dp_gsat_amd as G
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=dropout_p, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=deg)
    multi = tasks is not None
    model = G.get_model(X_DIM, 0, tasks if multi else 2, multi, cfg, dev).train()
    crit = G.Criterion(tasks if multi else 2, multi, capturable=multi)
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=3e-6, capturable=capturable, fused=capturable)
    return model, crit, opt


def training_state(model, opt):
    out = {"param." + n: p.detach().clone() for n, p in model.named_parameters()}
    out.update({"buffer." + n: b.detach().clone() for n, b in model.named_buffers()})
    for i, p in enumerate(p for grp in opt.param_groups for p in grp["params"]):
        for key, v in opt.state.get(p, {}).items():
            if isinstance(v, torch.Tensor):
                out[f"adam.{i}.{key}"] = v.detach().clone()
    return out


def assert_bitwise(a, b, what=""):
    assert set(a) == set(b), what
    for key in a:
        assert torch.equal(a[key], b[key]), f"{what}{key}"


def eager_step(model, crit, opt, ds, ids, dev, train=True):
    """The unpadded step of src/pretrain_clf.py: collate, forward, criterion, (zero_grad, backward, step)."""
    ub = ds.collate(torch.as_tensor(ids, device=dev))
    logits = model(ub.x, ub.edge_index, ub.batch, edge_attr=ub.edge_attr)
    loss = crit(logits, ub.y)
    if train:
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return ub, logits.detach(), loss.detach()


@contextmanager
def sync_free_on():
    """What the captured body runs under: an eager run_once() is compared bit for bit in the same mode."""
    import dp_gsat_amd as G
    was = G.graph_index.sync_free()
    G.set_sync_free(True)
    try:
        yield
    finally:
        G.set_sync_free(was)
        G.clear_cache()


def _setup(dev, backbone="GIN", tasks=None, seed=5, **kw):
    import dp_gsat_amd as G
    graphs = clf_graphs(tasks=tasks)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    torch.manual_seed(seed)
    return graphs, ds, clf_model(dev, graphs, backbone, tasks, **kw)


IDS = [3, 17, 9, 0, 22, 5, 11, 14]
CASES = [("GIN", None), ("PNA", None), ("GIN", T)]
CASE_IDS = ["GIN", "PNA", "GIN-multitask"]


@pytest.mark.parametrize("backbone,tasks", CASES, ids=CASE_IDS)
def test_construction_does_not_train_and_run_once_is_the_unpadded_step(dev, backbone, tasks):
    import dp_gsat_amd as G
    graphs, ds, (model, crit, opt) = _setup(dev, backbone, tasks)
    _, ds2, (model2, crit2, opt2) = _setup(dev, backbone, tasks)
    for m, c, o, d in ((model, crit, opt, ds), (model2, crit2, opt2, ds2)):
        eager_step(m, c, o, d, IDS[::-1], dev)                              # Adam state exists before the snapshot
    before = training_state(model, opt)
    modes = [m.training for m in model.modules()]
    rs = G.ReplayedClfStep(model, crit, opt, ds, BATCH)
    assert_bitwise(training_state(model, opt), before, "after construction: ")
    assert [m.training for m in model.modules()] == modes and not G.graph_index.sync_free()
    assert rs.capacity == ds.capacity_for(BATCH) and rs.log is None
    assert_bitwise(training_state(model2, opt2), before, "the twin: ")
    # the body, run eagerly, against the unpadded step from the same state
    rs._load_ids(IDS)
    rs.run_once()
    ub, logits, loss = eager_step(model2, crit2, opt2, ds2, IDS, dev)
    torch.cuda.synchronize()
    assert rs.batch.valid.tolist() == [ub.num_nodes, ub.num_edges, BATCH, 0]
    assert rs.clf_logits.shape == (BATCH + 1, tasks or 1)
    close(rs.loss, loss, TOL, what="loss")
    close(rs.clf_logits[:BATCH], logits, TOL, what="logits")
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        close(p.grad, q.grad, TOL, what="grad " + n)
    G.clear_cache()


@pytest.mark.parametrize("backbone,tasks", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("ragged", [False, True], ids=["fixed-count", "ragged"])
def test_replays_equal_the_body_run_eagerly(dev, backbone, tasks, ragged):
    """Three replays, then -- from the same parameters, buffers and Adam state -- run_once three times without the graph: not a bit
    differs.  Ragged: 1, 5 and all 8 slots."""
    import dp_gsat_amd as G
    graphs, ds, (model, crit, opt) = _setup(dev, backbone, tasks, dropout_p=0.0)
    rs = G.ReplayedClfStep(model, crit, opt, ds, BATCH, ragged=ragged)
    start = training_state(model, opt)
    steps = [[4], IDS[:5], IDS] if ragged else [IDS, IDS[::-1], list(range(8, 16))]
    losses, logits = [], []
    for ids in steps:
        losses.append(rs.step(ids).clone())
        logits.append(rs.clf_logits.clone())
        assert rs.batch.valid.tolist()[2:] == [len(ids), 0]
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(l)) for l in losses) and not rs.overflowed()
    after = training_state(model, opt)
    assert any(not torch.equal(after[k], start[k]) for k in after if k.startswith("param."))
    with torch.no_grad():                                                   # back to the start, in place: the graph holds the addresses
        for n, p in model.named_parameters():
            p.copy_(start["param." + n])
        for n, b in model.named_buffers():
            b.copy_(start["buffer." + n])
        for i, p in enumerate(p for grp in opt.param_groups for p in grp["params"]):
            for key, v in opt.state[p].items():
                if isinstance(v, torch.Tensor):
                    v.copy_(start[f"adam.{i}.{key}"])
    with sync_free_on():
        for j, ids in enumerate(steps):
            rs._load_ids(ids)
            rs.run_once()
            assert torch.equal(rs.loss, losses[j]) and torch.equal(rs.clf_logits, logits[j]), j
    torch.cuda.synchronize()
    assert_bitwise(training_state(model, opt), after, "eager bodies: ")


def test_ragged_overflow(dev):
    """A batch over the capacity: loss exactly 0, overflowed() True once, epoch_scores() raising until the next begin_epoch()."""
    import dp_gsat_amd as G
    graphs, ds, (model, crit, opt) = _setup(dev)
    n = sorted(g.x.shape[0] for g in graphs)
    e = sorted(g.edge_index.shape[1] for g in graphs)
    cap = (sum(n[-4:]) + 2, sum(e[-4:]))                                    # any four graphs fit, all eight of IDS do not
    assert sum(graphs[i].x.shape[0] for i in IDS) + 2 > cap[0]
    rs = G.ReplayedClfStep(model, crit, opt, ds, BATCH, capacity=cap, ragged=True, log=True)
    assert isinstance(rs.log, G.ClfLog) and rs.log.state.tolist() == [0, 0, 0, 0] and rs.log.loss_sum.tolist() == [0.0]
    assert (rs.log.max_graphs, rs.log.max_batches, rs.log.logit_cols, rs.log.y_cols, rs.log.multi_label) == (COUNT, COUNT, 1, 1, False)
    with pytest.raises(ValueError, match="before any append"):
        rs.epoch_scores()
    rs.begin_epoch()
    rs.step(IDS[:3])
    loss = rs.step(IDS)
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and rs.batch.valid.tolist() == [0, 0, 0, 1]
    assert rs.log.state.tolist() == [3, 1, 1, 0]
    with pytest.raises(ValueError, match="flag bit 0"):
        rs.epoch_scores()
    assert rs.overflowed() and not rs.overflowed()
    rs.begin_epoch()
    rs.step(IDS[:4])
    assert rs.epoch_scores()["n"] == 4 and not rs.overflowed()
    rows = rs.batches(range(COUNT))
    assert int((rows >= 0).sum()) == COUNT
    rs.check_epoch(list(range(4)))
    G.clear_cache()


@pytest.mark.parametrize("backbone,tasks", [("GIN", None), ("GIN", T)], ids=["GIN", "GIN-multitask"])
def test_epoch_scores_equal_the_oracle_on_what_the_steps_left(dev, backbone, tasks):
    import dp_gsat_amd as G
    graphs, ds, (model, crit, opt) = _setup(dev, backbone, tasks)
    rs = G.ReplayedClfStep(model, crit, opt, ds, BATCH, ragged=True, log=True)
    oracle = co.ClfLogOracle(COUNT, COUNT, tasks or 1, tasks or 1, tasks is not None)
    rs.begin_epoch()
    for ids in ([4], IDS[:5], IDS, list(range(12, 19))):
        loss = rs.step(ids)
        b = len(ids)
        oracle.append(rs.clf_logits[:b].cpu().numpy(), rs.batch.y[:b].cpu().numpy(), float(loss))
    got, want = rs.epoch_scores(), oracle.compute()
    assert got["n"] == want["n"] == 21 and got["loss"] == want["loss"]
    assert abs(got["clf_acc"] - want["clf_acc"]) <= 2 * 2.0 ** -53         # the same hits (below); the device's division may round twice
    if tasks is None:
        assert np.array_equal(got["confusion"], want["confusion"]) and got["bad"] == 0 and got["clf_roc"] == want["clf_roc"]
    else:
        assert np.array_equal(got["task_counts"], want["task_counts"]) and np.array_equal(got["unlabelled"], want["unlabelled"])
        assert np.array_equal(got["clf_roc_tasks"], want["clf_roc_tasks"], equal_nan=True)
        assert abs(got["clf_roc"] - want["clf_roc"]) <= 4 * 2.0 ** -53      # a mean of three values in [0, 1], in either order
    G.clear_cache()


def test_logging_does_not_change_training(dev):
    import dp_gsat_amd as G
    runs = []
    for log in (True, False):
        graphs, ds, (model, crit, opt) = _setup(dev, dropout_p=0.3)
        torch.manual_seed(77)
        from tests.replay import pin_seed_stream
        rs = G.ReplayedClfStep(model, crit, opt, ds, BATCH, ragged=True, log=log)
        pin_seed_stream(dev, 0x5EED)
        rs.begin_epoch()
        losses = [rs.step(row).clone() for row in rs.batches(range(COUNT))]
        torch.cuda.synchronize()
        if log:
            assert rs.epoch_scores()["n"] == COUNT
        else:
            with pytest.raises(ValueError, match="without log=True"):
                rs.epoch_scores()
        runs.append((training_state(model, opt), losses))
    (a, la), (b, lb) = runs
    assert any(k.startswith("adam.") for k in a) and any("running_mean" in k for k in a)
    assert_bitwise(a, b)
    assert len(la) == len(lb) and all(torch.equal(x, y) for x, y in zip(la, lb))
    G.clear_cache()


EVAL_IDS = [21, 5, 12, 0, 7, 23, 8, 19, 2, 10, 11, 1, 22, 14, 16, 9, 13, 3, 15]     # two full batches and a tail of three


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed-count", "ragged"])
def test_replayed_eval_scores_what_the_eager_loops_score(dev, ragged):
    """run() against a ClfLog fed by an eager loop over the same padded batches (exactly), and its loss against the unpadded eager
    evaluation (at TOL)."""
    import dp_gsat_amd as G
    graphs, ds, (model, crit, opt) = _setup(dev, dropout_p=0.3)
    eager_step(model, crit, opt, ds, IDS, dev)                              # running statistics that are not the initial ones
    modes = [m.training for m in model.modules()]
    before = training_state(model, opt)
    ev = G.ReplayedClfEval(model, crit, ds, BATCH, ragged=ragged)
    assert [m.training for m in model.modules()] == modes and not G.graph_index.sync_free()
    assert ev.log.state.tolist() == [0, 0, 0, 0]
    got = ev.run(np.asarray(EVAL_IDS))
    assert model.training and got["n"] == len(EVAL_IDS)
    rows = ev.batches(EVAL_IDS) if ragged else [EVAL_IDS[0:8], EVAL_IDS[8:16]]
    assert ev.log.state.tolist() == [len(EVAL_IDS), len(rows) + (0 if ragged else 1), 0, 0]
    log = G.ClfLog(COUNT, COUNT, 1, device=dev)
    unpadded = []
    model.eval()
    try:
        with torch.no_grad(), sync_free_on():
            for row in rows:
                b = ds.collate_padded(torch.as_tensor(row, device=dev), ev.capacity, ragged=ragged)
                logits, loss = G.replay._clf_forward(model, crit, b)
                log.append(b, logits, loss)
            if not ragged:
                ub, logits, loss = eager_step(model, crit, None, ds, EVAL_IDS[16:], dev, train=False)
                log.append(ub, logits, loss)
        with torch.no_grad():
            for row in rows:
                ids = [i for i in torch.as_tensor(row).tolist() if i >= 0]
                unpadded.append(float(eager_step(model, crit, None, ds, ids, dev, train=False)[2]))
            if not ragged:
                unpadded.append(float(loss))
    finally:
        model.train()
    want = log.compute()
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    mean = float(np.mean(unpadded))
    assert abs(got["loss"] - mean) <= TOL * max(1.0, abs(mean))
    assert_bitwise(training_state(model, opt), before, "evaluation wrote: ")
    G.clear_cache()


def test_evaluation_does_not_change_training(dev):
    import dp_gsat_amd as G
    from tests.replay import pin_seed_stream, seed_state
    runs = []
    for with_eval in (True, False):
        graphs, ds, (model, crit, opt) = _setup(dev, dropout_p=0.3)
        rs = G.ReplayedClfStep(model, crit, opt, ds, BATCH)
        ev = G.ReplayedClfEval(model, crit, ds, BATCH) if with_eval else None
        pin_seed_stream(dev, 0x5EED)
        torch.manual_seed(77)
        for ids in (IDS, IDS[::-1], list(range(8, 16))):
            rs.step(ids)
            if ev is not None:
                assert np.isfinite(ev.run(EVAL_IDS)["loss"]) and model.training
        torch.cuda.synchronize()
        runs.append((training_state(model, opt), seed_state(dev), torch.cuda.get_rng_state(dev).clone(), torch.get_rng_state().clone()))
    (a, sa, ca, ha), (b, sb, cb, hb) = runs
    assert_bitwise(a, b)
    assert sa == sb and torch.equal(ca, cb) and torch.equal(ha, hb)          # no generator moved
    G.clear_cache()


def test_a_tensor_learning_rate_moves_between_replays(dev):
    import dp_gsat_amd as G
    ends = []
    for second_lr in (1e-2, 1e-1):
        graphs, ds, (model, crit, opt) = _setup(dev, lr=torch.tensor(1e-2, device=dev))
        rs = G.ReplayedClfStep(model, crit, opt, ds, BATCH)
        rs.step(IDS)
        opt.param_groups[0]["lr"].fill_(second_lr)
        rs.step(IDS[::-1])
        torch.cuda.synchronize()
        ends.append(training_state(model, opt))
    a, b = ends
    assert any(not torch.equal(a[k], b[k]) for k in a if k.startswith("param."))
    G.clear_cache()


def test_refusals(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd.encoders import BatchNorm1d
    graphs, ds, (model, crit, opt) = _setup(dev)
    eager_step(model, crit, opt, ds, IDS, dev)                              # Adam state exists before the snapshot
    before = training_state(model, opt)
    plain = torch.optim.Adam(model.parameters(), lr=1e-2)
    with pytest.raises(ValueError, match="capturable"):
        G.ReplayedClfStep(model, crit, plain, ds, BATCH)
    with pytest.raises(ValueError, match="capturable=True"):
        G.ReplayedClfStep(model, G.Criterion(T, True), opt, ds, BATCH)
    with pytest.raises(ValueError, match="capturable=True"):
        G.ReplayedClfEval(model, G.Criterion(T, True), ds, BATCH)
    bns = [m for m in model.modules() if isinstance(m, BatchNorm1d)]
    assert bns
    bns[0].sync_group = True
    try:
        with pytest.raises(ValueError, match="sync_group"):
            G.ReplayedClfStep(model, crit, opt, ds, BATCH)
        with pytest.raises(ValueError, match="sync_group"):
            G.ReplayedClfEval(model, crit, ds, BATCH)
    finally:
        del bns[0].sync_group
    unlabelled = clf_graphs()
    for g in unlabelled:
        g.y = None
    no_y = G.PackedDataset.from_data_list(unlabelled, dev)
    with pytest.raises(ValueError, match="y_all"):
        G.ReplayedClfStep(model, crit, opt, no_y, BATCH)
    with pytest.raises(ValueError, match="y_all"):
        G.ReplayedClfEval(model, crit, no_y, BATCH)
    N = sum(g.x.shape[0] for g in graphs[:BATCH])
    E = sum(g.edge_index.shape[1] for g in graphs[:BATCH])
    tight = (N + 1, E)                                                      # one padding node short for the warm-up batch, graphs 0..7
    for make in (lambda: G.ReplayedClfStep(model, crit, opt, ds, BATCH, capacity=tight), lambda: G.ReplayedClfEval(model, crit, ds, BATCH, capacity=tight)):
        with pytest.raises(ValueError, match="do not fit the capacity"):
            make()
    assert_bitwise(training_state(model, opt), before, "a refusal trained: ")
    assert not G.graph_index.sync_free()
    rs = G.ReplayedClfStep(model, crit, opt, ds, BATCH)                      # and the plain model is taken
    with pytest.raises(ValueError, match="captured for 8"):
        rs.step([0, 1, 2])
    G.clear_cache()
