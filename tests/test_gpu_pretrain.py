"""-m gpu: pretrain_clf against an eager restatement of src/pretrain_clf.py:114-143 written here, and the example's --pretrain."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import clf_log_oracle as co
from tests.test_gpu_clf_replay import BATCH, clf_graphs, clf_model, sync_free_on
from tests.util import TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, EPOCHS = 48, 3
SPLITS = {"train": list(range(32)), "valid": list(range(32, 40)), "test": list(range(40, 48))}
KEYS = ("metric/best_clf_epoch", "metric/best_clf_valid_loss", "metric/best_clf_train", "metric/best_clf_valid", "metric/best_clf_test")


def _make(dev):
    import dp_gsat_amd as G
    graphs = clf_graphs(COUNT, seed=9)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    torch.manual_seed(21)
    return ds, clf_model(dev, graphs, dropout_p=0.0)


def _pass(obj, ids):
    """One pass of uncaptured run_once bodies over the ragged batches of ``ids``, scored by the oracle from what every body left."""
    oracle = co.ClfLogOracle(COUNT, COUNT, 1)
    obj.log.reset()
    for row in obj.batches(ids):
        b = int((row >= 0).sum())
        obj._load_ids(row)
        obj.run_once()
        oracle.append(obj.clf_logits[:b].cpu().numpy(), obj.batch.y[:b].cpu().numpy(), float(obj.loss))
    res = oracle.compute()
    return res["clf_acc"], res["loss"]


def test_pretrain_clf_equals_the_eager_loop(dev):
    import dp_gsat_amd as G
    ds, (model, crit, opt) = _make(dev)
    got, history = G.pretrain_clf(model, crit, opt, ds, SPLITS, EPOCHS, BATCH)
    assert tuple(got) == KEYS and [h["epoch"] for h in history] == list(range(EPOCHS)) and model.training
    # the eager loop: the same ragged batches in the same order, the bodies without their graphs, lines 126-129 restated
    ds2, (model2, crit2, opt2) = _make(dev)
    step = G.ReplayedClfStep(model2, crit2, opt2, ds2, BATCH, ragged=True, log=True)
    ev = G.ReplayedClfEval(model2, crit2, ds2, BATCH, ragged=True)
    want = dict.fromkeys(KEYS, 0)
    rows = []
    with sync_free_on():
        for epoch in range(EPOCHS):
            train_res, train_loss = _pass(step, SPLITS["train"])
            valid_res, valid_loss = _pass(ev, SPLITS["valid"])
            test_res, _ = _pass(ev, SPLITS["test"])
            rows.append((train_res, valid_res, test_res, train_loss, valid_loss))
            if valid_res > want["metric/best_clf_valid"] or (valid_res == want["metric/best_clf_valid"] and valid_loss < want["metric/best_clf_valid_loss"]):
                want["metric/best_clf_epoch"] = epoch
                want["metric/best_clf_train"], want["metric/best_clf_valid"], want["metric/best_clf_test"] = train_res, valid_res, test_res
                want["metric/best_clf_valid_loss"] = valid_loss
    print("pretrain_clf:", got, "eager:", want)
    assert got["metric/best_clf_epoch"] == want["metric/best_clf_epoch"]
    for key in KEYS[1:]:
        assert abs(got[key] - want[key]) <= TOL * max(1.0, abs(want[key])), key
    for h, (tr, va, te, trl, val) in zip(history, rows):
        for key, w in (("train", tr), ("valid", va), ("test", te), ("train_loss", trl), ("valid_loss", val)):
            assert abs(h[key] - w) <= TOL * max(1.0, abs(w)), (h["epoch"], key)
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):      # both are left at the last epoch
        assert torch.allclose(p, q, rtol=0, atol=TOL * max(1.0, float(q.abs().max()))), n
    G.clear_cache()


def test_a_scheduler_needs_a_tensor_learning_rate(dev):
    import dp_gsat_amd as G
    ds, (model, crit, opt) = _make(dev)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max", factor=0.5, patience=0)
    with pytest.raises(ValueError, match="device tensor"):
        G.pretrain_clf(model, crit, opt, ds, SPLITS, 1, BATCH, scheduler=sched)
    with pytest.raises(ValueError, match="metric"):
        G.pretrain_clf(model, crit, opt, ds, SPLITS, 1, BATCH, metric="f1")
    graphs = clf_graphs(COUNT, seed=9)
    torch.manual_seed(21)
    model, crit, opt = clf_model(dev, graphs, lr=torch.tensor(1e-2, device=dev))
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max", factor=0.5, patience=0)
    lr = opt.param_groups[0]["lr"]
    got, history = G.pretrain_clf(model, crit, opt, ds, SPLITS, 2, BATCH, metric="roc", scheduler=sched, shuffle=True,
                                  generator=torch.Generator().manual_seed(3))
    assert opt.param_groups[0]["lr"] is lr and lr.is_cuda and len(history) == 2          # the scheduler filled the tensor the graph reads
    assert all(np.isfinite(h["train_loss"]) for h in history)
    G.clear_cache()


def test_example_pretrains_before_gsat(dev):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ba2motifs.py"), "--graph", "--ragged", "--graphs", "200",
                          "--epochs", "2", "--pretrain", "2"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    pre = [i for i, l in enumerate(lines) if l.startswith("pretrain epoch")]
    gsat = [i for i, l in enumerate(lines) if l.startswith("epoch")]
    assert len(pre) == 2 and gsat and max(pre) < min(gsat), out.stdout[-2000:]
