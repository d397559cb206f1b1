"""Evaluation scores on the device: classifier ROC-AUC and accuracy, attention histograms, the PR curve.

The second half of the reference's get_eval_score (src/run_gsat.py:746-781): ``clf_acc`` (:748, multi-label form
src/pretrain_clf.py:97), ``clf_roc`` = the ogb ``Evaluator``'s rocauc (:756-759, src/pretrain_clf.py:104), the two attention
histograms (:767-768) and the PR curve (:776).  The reference computes them from host copies of every logit and every edge's
attention; here the per-task ROC-AUC and the histogram are HIP kernels (csrc/evaluate.hip), the rest is a few torch operations on
``[R, T]`` / ``[2, bins]`` device tensors, and nothing is copied to the host until :meth:`EvaluationMeter.compute`.

Conventions of :mod:`dp_gsat_amd.explain`: ROCm tensors only (``GsatHipError`` on CPU tensors), ``ValueError`` on bad shapes,
``-0.0 == +0.0``, NaN scores / attention unsupported by the ROC-AUC (the histogram counts NaN attention in ``outside``).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from ._lib import GsatHipError, call, ptr, stream
from .explain import ExplanationMeter, _att, _labels
from .get_model import get_preds
from .graph_index import call_size

MAX_BINS = 4096


class AttentionHistogram(NamedTuple):
    """counts int64[2, bins]: row 0 = unlabelled (background) edges, row 1 = labelled (signal) edges, ``bins`` equal bins over the
    closed range [lo, hi]; outside int64[2]: per class, the entries below lo, above hi or NaN."""
    counts: torch.Tensor
    outside: torch.Tensor
    lo: float
    hi: float


def _scores(logits, labels):
    """(logits fp32[R,T], labels fp32[R,T]) contiguous, NaN labels kept; ``[R]`` inputs are one task."""
    for t in (logits, labels):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise GsatHipError("dp_gsat_amd.evaluate needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    if logits.dim() not in (1, 2):
        raise ValueError("logits must have shape [R] or [R, T]")
    lg = logits.detach().reshape(-1, 1) if logits.dim() == 1 else logits.detach()
    if labels.numel() != lg.numel() or (labels.dim() == 2 and tuple(labels.shape) != tuple(lg.shape)) or labels.dim() > 2:
        raise ValueError(f"labels of shape {tuple(labels.shape)} for logits of shape {tuple(logits.shape)}")
    return lg.to(torch.float32).contiguous(), labels.detach().reshape(lg.shape).to(torch.float32).contiguous()


def task_auroc_counts(logits, labels) -> torch.Tensor:
    """int64[T, 3] on the device: per task (column) the integers (U2, P, Nn) of :func:`dp_gsat_amd.explain.attention_auroc_counts`
    over the rows whose label is not NaN (0 = negative, anything else = positive); ROC-AUC of a task = U2 / (2 P Nn).  Integer
    arithmetic: bitwise repeatable."""
    lg, lab = _scores(logits, labels)
    R, T = lg.shape
    out = torch.empty((T, 3), dtype=torch.int64, device=lg.device)
    if T == 0:
        return out
    ws_bytes = call_size("gsat_auroc_tasks_workspace_bytes", R, T)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=lg.device)
    call("gsat_auroc_tasks", ptr(lg) if R else None, ptr(lab) if R else None, R, T, ptr(out), ptr(ws), ws_bytes, stream())
    return out


def classifier_rocauc(logits, labels) -> torch.Tensor:
    """The ogb ``Evaluator``'s rocauc as a 0-dim float64 device tensor: the mean of the exact, tie-aware per-task ROC-AUC over the
    tasks that have at least one positive and one negative labelled row; NaN labels are skipped.  When NO task can be scored ogb
    raises a RuntimeError; this function returns NaN instead, because finding out on the host would be a sync."""
    return classifier_rocauc_tasks(logits, labels)[0]


def classifier_rocauc_tasks(logits, labels):
    """``(classifier_rocauc(logits, labels), per_task)`` from ONE ``task_auroc_counts`` call: ``per_task`` float64[T] on the device, the
    ROC-AUC of every task, NaN for a task without both classes among its labelled rows."""
    c = task_auroc_counts(logits, labels)
    den = 2 * c[:, 1] * c[:, 2]
    ok = den > 0
    per_task = torch.where(ok, c[:, 0].double() / den.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=c.device))
    mean = per_task.sum() / ok.sum().double()                          # 0 / 0 = NaN: no scorable task
    return mean, torch.where(ok, per_task, torch.full((), float("nan"), dtype=torch.float64, device=c.device))


def classifier_accuracy(logits, labels, multi_label: bool = False) -> torch.Tensor:
    """0-dim float64 device tensor.  Single label: ``(get_preds(logits) == labels).sum() / R`` (src/run_gsat.py:748); multi label:
    the matches over all R * T entries, a NaN (unlabelled) entry never matching (src/pretrain_clf.py:97).  Plain torch."""
    for t in (logits, labels):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise GsatHipError("dp_gsat_amd.evaluate needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    if logits.dim() != 2:
        raise ValueError("logits must have shape [R, C]")
    preds = get_preds(logits.detach(), multi_label)
    if labels.numel() != preds.numel():
        raise ValueError(f"labels of shape {tuple(labels.shape)} for predictions of shape {tuple(preds.shape)}")
    hits = (preds == labels.detach().reshape(preds.shape).to(preds.dtype)).sum().double()
    return hits / float(preds.numel() if multi_label else preds.shape[0])


def attention_histogram(att, exp_labels=None, bins: int = 64, range=(0.0, 1.0), out: Optional[AttentionHistogram] = None) -> AttentionHistogram:
    """Two-class histogram of the attention, integer counts on the device.  ``exp_labels=None``: every edge is background.  The bin of
    a value ``a`` is ``min(floor((float64(a) - lo) * (bins / (hi - lo))), bins - 1)`` evaluated in fp64 -- ``hi`` itself falls into the
    last bin, like numpy's; values outside [lo, hi] and NaN are counted per class in ``outside``.  With ``out=`` the batch is ADDED to
    that histogram (its bins and range are used, ``bins`` / ``range`` are ignored) and ``out`` is returned: an epoch accumulates
    exactly, in O(bins) memory, without keeping its batches."""
    a = _att(att)
    E = a.shape[0]
    lab = _labels(exp_labels, E) if exp_labels is not None else None
    if out is None:
        bins, (lo, hi) = int(bins), (float(range[0]), float(range[1]))
        if not (1 <= bins <= MAX_BINS) or not lo < hi:
            raise ValueError(f"need 1 <= bins <= {MAX_BINS} and range[0] < range[1]")
        out = AttentionHistogram(torch.zeros((2, bins), dtype=torch.int64, device=a.device),
                                 torch.zeros(2, dtype=torch.int64, device=a.device), lo, hi)
    else:
        c, o = out.counts, out.outside
        if not (c.is_cuda and o.is_cuda):
            raise GsatHipError("dp_gsat_amd.evaluate needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
        if c.dtype != torch.int64 or o.dtype != torch.int64 or c.dim() != 2 or c.shape[0] != 2 or tuple(o.shape) != (2,) \
                or not (1 <= c.shape[1] <= MAX_BINS) or not out.lo < out.hi:
            raise ValueError("out must be an AttentionHistogram with counts int64[2, bins] and outside int64[2]")
    if E:
        call("gsat_att_histogram", ptr(a), ptr(lab), E, int(out.counts.shape[1]), float(out.lo), float(out.hi), ptr(out.counts),
             ptr(out.outside), stream())
    return out


def pr_curve(hist) -> dict:
    """Precision / recall at ``bins`` thresholds from a two-class histogram (an :class:`AttentionHistogram` or its ``counts``
    int64[2, B]); device tensors ``tp, fp, tn, fn`` (int64[B]) and ``precision, recall`` (float64[B]).  Threshold ``i`` predicts
    positive what fell into a bin ``>= i``, i.e. attention ``>= lo + i (hi - lo) / B``; the counts are suffix sums of the two rows,
    ``precision = tp / max(tp + fp, 1)``, ``recall = tp / max(tp + fn, 1)``.  Entries in ``outside`` take no part.

    Correspondence with TensorBoard's ``add_pr_curve`` (src/run_gsat.py:776; ``num_thresholds = 127``): TensorBoard buckets a
    prediction ``p`` in [0, 1] by ``floor(p * 126)`` into 127 buckets (``p == 1`` alone in the last) and forms the same suffix sums
    with ``max(., 1e-7)`` in the denominators, which gives the same quotients on integer counts.  ``range=(0, 1), bins=127`` here
    buckets by ``floor(p * 127)`` (``p == 1`` joins the last bucket): the same construction on thresholds ``i / 127`` instead of
    ``i / 126``.  The curves are therefore not equal point by point, and nothing more is claimed."""
    counts = hist.counts if isinstance(hist, AttentionHistogram) else hist
    if not isinstance(counts, torch.Tensor) or not counts.is_cuda:
        raise GsatHipError("dp_gsat_amd.evaluate needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    if counts.dim() != 2 or counts.shape[0] != 2:
        raise ValueError("counts must have shape [2, bins]")
    suffix = counts.to(torch.int64).flip(1).cumsum(1).flip(1)
    fp, tp = suffix[0], suffix[1]
    total = suffix[:, :1] if counts.shape[1] else suffix.new_zeros((2, 1))
    tn, fn = total[0] - fp, total[1] - tp
    return {"tp": tp, "fp": fp, "tn": tn, "fn": fn, "precision": tp.double() / (tp + fp).clamp(min=1).double(),
            "recall": tp.double() / (tp + fn).clamp(min=1).double()}


class EvaluationMeter:
    """One epoch of get_eval_score (src/run_gsat.py:746-781) on the device.  ``update`` feeds an inner
    :class:`~dp_gsat_amd.explain.ExplanationMeter`, adds the batch's attention to one running histogram over [0, 1] and keeps device
    copies of the classifier logits and ``data.y``; it never syncs when ``data.num_graphs`` is given.  ``compute`` returns the inner
    meter's dict plus ``clf_acc``, ``clf_roc`` (:func:`classifier_rocauc` for every dataset, not only the ogb ones), ``bkg_att_hist``
    / ``signal_att_hist`` (numpy int64[bins]), ``att_outside`` (numpy int64[2]) and ``pr_curve`` (numpy arrays), with ONE host read on
    top of the inner meter's."""

    def __init__(self, k: int, bins: int = 64, multi_label: bool = False):
        if not 1 <= int(bins) <= MAX_BINS:
            raise ValueError(f"need 1 <= bins <= {MAX_BINS}")
        self.inner = ExplanationMeter(k)
        self.bins, self.multi_label = int(bins), bool(multi_label)
        self.reset()

    def reset(self):
        self.inner.reset()
        self._hist, self._logits, self._y = None, [], []

    def update(self, att, data, clf_logits) -> None:
        """``data``: a collated batch with ``edge_index``, ``batch``, ``edge_label``, ``y`` and ``num_graphs``."""
        if not isinstance(clf_logits, torch.Tensor) or not clf_logits.is_cuda or not data.y.is_cuda:
            raise GsatHipError("dp_gsat_amd.evaluate needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
        if clf_logits.dim() != 2 or data.y.shape[0] != clf_logits.shape[0]:
            raise ValueError("clf_logits must have shape [G, C] with one row per entry of data.y")
        self.inner.update(att, data)
        self._hist = attention_histogram(att, data.edge_label, bins=self.bins, out=self._hist)
        self._logits.append(clf_logits.detach().clone())         # the caller may refill its (static) buffers between batches
        self._y.append(data.y.clone())

    def compute(self) -> dict:
        res = self.inner.compute()                               # raises before any update()
        logits, y = torch.cat(self._logits), torch.cat(self._y)
        scores = [classifier_accuracy(logits, y, self.multi_label).view(1)]
        binary = self.multi_label or logits.shape[1] == 1
        # the score of a C-class softmax head has no single ROC-AUC: 0, like the reference outside the (binary) ogb sets
        scores.append(classifier_rocauc(logits, y).view(1) if binary else torch.zeros(1, dtype=torch.float64, device=logits.device))
        pr = pr_curve(self._hist)
        names = ("tp", "fp", "tn", "fn")
        packed = torch.cat([self._hist.counts.view(-1), self._hist.outside] + [pr[n] for n in names] +
                           [t.view(torch.int64) for t in scores + [pr["precision"], pr["recall"]]]).cpu().numpy()   # the one host read
        B = self.bins
        ints, floats = packed[:6 * B + 2], packed[6 * B + 2:].view(np.float64)
        res.update(clf_acc=float(floats[0]), clf_roc=float(floats[1]), bkg_att_hist=ints[:B].copy(), signal_att_hist=ints[B:2 * B].copy(),
                   att_outside=ints[2 * B:2 * B + 2].copy())
        curve = {n: ints[2 * B + 2 + i * B:2 * B + 2 + (i + 1) * B].copy() for i, n in enumerate(names)}
        curve.update(precision=floats[2:2 + B].copy(), recall=floats[2 + B:2 + 2 * B].copy())
        res["pr_curve"] = curve
        return res
