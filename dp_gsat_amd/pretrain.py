"""ERM pre-training of the backbone (src/pretrain_clf.py:114-143) on the replayed classifier classes: no eager batch, two host reads per
pass.  ``run_gsat.py`` with ``from_scratch: false`` pre-trains the classifier this way and starts GSAT from the model of the LAST epoch
(``epoch_{pretrain_epochs - 1}``), which is where ``pretrain_clf`` leaves ``model``."""
from __future__ import annotations

from typing import Optional

import torch

from .replay import ReplayedClfEval, ReplayedClfStep

METRIC_KEYS = ("metric/best_clf_epoch", "metric/best_clf_valid_loss", "metric/best_clf_train", "metric/best_clf_valid",
               "metric/best_clf_test")


def init_clf_metric_dict() -> dict:
    """The classifier entries of the reference's ``init_metric_dict`` (src/utils/utils.py:13-14): all 0."""
    return {key: 0 for key in METRIC_KEYS}


def update_best_clf(metric_dict: dict, epoch: int, train_res: float, valid_res: float, test_res: float, valid_loss: float) -> bool:
    """The best-epoch rule of src/pretrain_clf.py:126-129, in place: the epoch is recorded when its validation metric is greater than the
    recorded one, or equal to it with a smaller validation loss.  The dict starts at 0 everywhere, so a first epoch whose validation
    metric is 0 is not recorded.  Returns whether the epoch was recorded."""
    better = valid_res > metric_dict["metric/best_clf_valid"]
    tie_won = valid_res == metric_dict["metric/best_clf_valid"] and valid_loss < metric_dict["metric/best_clf_valid_loss"]
    if not (better or tie_won):
        return False
    metric_dict["metric/best_clf_epoch"] = epoch
    metric_dict["metric/best_clf_train"], metric_dict["metric/best_clf_valid"], metric_dict["metric/best_clf_test"] = train_res, valid_res, test_res
    metric_dict["metric/best_clf_valid_loss"] = valid_loss
    return True


def _lr_on_device(optimizer) -> bool:
    return all(isinstance(g["lr"], torch.Tensor) and g["lr"].is_cuda for g in optimizer.param_groups)


def pretrain_clf(model, criterion, optimizer, dataset, splits, epochs: int, batch_size: int, capacity: Optional[tuple] = None,
                 ragged: bool = True, metric: str = "acc", scheduler=None, shuffle: bool = False, generator=None):
    """The loop of src/pretrain_clf.py:114-143 over ``splits`` = {"train": ids, "valid": ids, "test": ids} of ``dataset`` (a
    PackedDataset with ``y_all``).  Per epoch: a training pass through ``ReplayedClfStep(log=True)`` scored from its own log (the
    training-mode logits each step produced, as the reference scores them), then a validation and a test pass through one
    ``ReplayedClfEval``.  ``metric``: "acc" (``clf_acc``) or "roc" (``clf_roc``, the ogb datasets).  ``scheduler.step(valid_metric)`` follows
    every epoch; a scheduler is refused unless every ``lr`` of the optimizer is a device tensor -- the captured step reads the
    learning rate where it lives, and a float would be frozen at capture (torch's ``ReduceLROnPlateau`` fills a tensor ``lr`` in place).
    The best epoch follows ``update_best_clf``.  ``shuffle`` (default False: the reference's loaders do not shuffle,
    src/utils/get_data_loaders.py:133,141) permutes the training ids every epoch with ``torch.randperm(generator=)``.

    A fixed-count run (``ragged=False``) trains on the full batches only and leaves the training tail of fewer than ``batch_size``
    graphs out of the epoch; the evaluation passes run their tail eagerly.

    Returns ``(metric_dict, history)``: the reference's keys ``metric/best_clf_epoch``, ``best_clf_valid_loss``, ``best_clf_train``,
    ``best_clf_valid``, ``best_clf_test``, and one dict per epoch (``epoch``, ``train`` / ``valid`` / ``test`` metric, the three mean
    losses, ``recorded``).  ``model`` is left at the last epoch."""
    if metric not in ("acc", "roc"):
        raise ValueError('metric must be "acc" or "roc"')
    if int(epochs) < 0:
        raise ValueError("epochs must not be negative")
    if scheduler is not None and not _lr_on_device(optimizer):
        raise ValueError("pretrain_clf: a scheduler needs the optimizer's lr as a device tensor, e.g. Adam(params, "
                         "lr=torch.tensor(1e-3, device=dev), capturable=True, fused=True): a float lr is frozen into the captured step")
    key = "clf_acc" if metric == "acc" else "clf_roc"
    ids = {name: torch.as_tensor(splits[name]).reshape(-1).to(torch.int64) for name in ("train", "valid", "test")}
    if any(int(v.numel()) == 0 for v in ids.values()):
        raise ValueError("pretrain_clf: every split needs at least one graph")
    step = ReplayedClfStep(model, criterion, optimizer, dataset, batch_size, capacity=capacity, ragged=ragged, log=True)
    ev = ReplayedClfEval(model, criterion, dataset, batch_size, capacity=step.capacity, ragged=ragged)
    metric_dict, history = init_clf_metric_dict(), []
    B = step.batch_size
    for epoch in range(int(epochs)):
        train_ids = ids["train"]
        if shuffle:
            train_ids = train_ids[torch.randperm(int(train_ids.numel()), generator=generator)]
        step.begin_epoch()
        rows = step.batches(train_ids) if ragged else [train_ids[s:s + B] for s in range(0, int(train_ids.numel()) - B + 1, B)]
        for row in rows:
            step.step(row)
        if step.overflowed():
            raise RuntimeError("pretrain_clf: a training batch overflowed the capacity")
        train = step.epoch_scores()
        valid, test = ev.run(ids["valid"]), ev.run(ids["test"])
        if scheduler is not None:
            scheduler.step(valid[key])
        recorded = update_best_clf(metric_dict, epoch, train[key], valid[key], test[key], valid["loss"])
        history.append({"epoch": epoch, "train": train[key], "valid": valid[key], "test": test[key], "train_loss": train["loss"],
                        "valid_loss": valid["loss"], "test_loss": test["loss"], "recorded": recorded})
    return metric_dict, history
