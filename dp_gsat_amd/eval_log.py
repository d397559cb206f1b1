"""A device-resident log of one evaluation epoch, scored once at its end.

The meters of :mod:`dp_gsat_amd.explain` / :mod:`dp_gsat_amd.evaluate` keep Python lists of cloned tensors and launch their ranking
and delta-KL kernels batch by batch: neither survives a captured hipGraph, whose every replay would write to the same addresses.
:class:`EpochLog` allocates everything once and ``append`` is two launches of csrc/eval_log.hip that find their offsets in a counter
block ON THE DEVICE, so an evaluation batch -- collation, forward, append -- replays as one graph (``ReplayedEval``).  The log is itself
one big collated batch whose edges already lie graph by graph: ``compute`` ranks all its graphs in one ``gsat_rank_edges`` call with
the identity as edge order, and scores the rest with the kernels the meters use plus the per-segment delta-KL.

Layout after the appends (prefix lengths in ``state`` = edges, graphs, batches, flags):
  att fp32[edges], label uint8[edges]      attention / 0-1 label, graph by graph; inside a graph by ascending edge id of its batch
  graph_edge_ptr int32[graphs + 1]          first edge of every logged graph
  logits fp32[graphs, logit_cols], y fp32[graphs, y_cols]      (NaN = unlabelled)
  batch_edge_ptr int64[batches + 1]         first edge of every logged batch
  loss_sums float64[3]                      sums of the (loss, pred, info) triples; NaN once a batch came without one
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import GsatHipError, call, ptr, stream
from .evaluate import MAX_BINS, attention_histogram, classifier_accuracy, classifier_rocauc, classifier_rocauc_tasks, pr_curve
from .explain import _att, _labels, attention_auroc, check_levels, check_rankings, delta_kl_stats, rank_edges_lds_cap
from .graph_index import call_size, get_index

FLAG_OVERFLOW, FLAG_FULL = 1, 2


def delta_kl_segments_chunk() -> int:
    """Entries of a segment that one workgroup of ``gsat_delta_kl_segments`` handles; longer segments are cut into chunks of it."""
    return call_size("gsat_delta_kl_segments_chunk")


def delta_kl_segments(att, exp_labels, seg_ptr, max_seg_len: Optional[int] = None, eps: float = 1e-6) -> torch.Tensor:
    """float32[S, 3] on the device: row s = ``delta_kl_stats(att[seg_ptr[s]:seg_ptr[s+1]], exp_labels[...])``, every segment with its own
    r.  ``seg_ptr``: int64[S + 1] on the device.  ``max_seg_len``: a bound on the longest segment when the host knows one (it sizes the
    grid; default: all of ``att``); a longer segment gives a NaN row.  Bitwise repeatable."""
    a = _att(att)
    E = a.shape[0]
    lab = _labels(exp_labels, E)
    if not isinstance(seg_ptr, torch.Tensor) or not seg_ptr.is_cuda:
        raise GsatHipError("dp_gsat_amd.eval_log needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    if seg_ptr.dtype != torch.int64 or seg_ptr.dim() != 1 or seg_ptr.numel() < 1:
        raise ValueError("seg_ptr must be an int64 vector of S + 1 entries")
    sp = seg_ptr.contiguous()
    S = int(sp.shape[0]) - 1
    out = torch.empty((S, 3), dtype=torch.float32, device=a.device)
    if S == 0:
        return out
    bound = E if max_seg_len is None else min(max(int(max_seg_len), 0), E)
    ws_bytes = call_size("gsat_delta_kl_segments_workspace_bytes", S, bound)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
    call("gsat_delta_kl_segments", ptr(a) if E else None, ptr(lab) if E else None, ptr(sp), S, E, bound, float(eps), ptr(out), ptr(ws),
         ws_bytes, stream())
    return out


class EpochLog:
    """``EpochLog(k, max_graphs, max_edges, max_batches, logit_cols, y_cols=1, bins=64, multi_label=False, device=None)``: the arrays of the
    module docstring, allocated once (plain attributes: their addresses never change).  ``append`` issues kernels only; ``compute`` reads
    the device twice.  An append that cannot be taken -- a padded batch whose overflow word is set (flag bit 0), or one that would
    exceed ``max_edges``, ``max_graphs`` or ``max_batches`` (flag bit 1) -- writes nothing and is reported by ``compute``."""

    def __init__(self, k: int, max_graphs: int, max_edges: int, max_batches: int, logit_cols: int, y_cols: int = 1, bins: int = 64,
                 multi_label: bool = False, device=None):
        if int(k) <= 0:
            raise ValueError("k must be positive")
        if not 1 <= int(bins) <= MAX_BINS:
            raise ValueError(f"need 1 <= bins <= {MAX_BINS}")
        if min(int(max_graphs), int(max_edges), int(max_batches)) < 0 or int(logit_cols) < 1 or int(y_cols) < 1:
            raise ValueError("EpochLog needs non-negative capacities and at least one logit and one label column")
        if int(max_edges) >= 2 ** 31 or int(max_graphs) >= 2 ** 31:
            raise ValueError("EpochLog: max_edges and max_graphs must be below 2**31 (the ranking kernels carry int32 edge ids)")
        self.k, self.bins, self.multi_label = int(k), int(bins), bool(multi_label)
        self.max_graphs, self.max_edges, self.max_batches = int(max_graphs), int(max_edges), int(max_batches)
        self.logit_cols, self.y_cols = int(logit_cols), int(y_cols)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise GsatHipError("dp_gsat_amd.eval_log needs a ROCm (cuda) device: the HIP path has no CPU fallback")
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        self.att, self.label = new(self.max_edges, torch.float32), new(self.max_edges, torch.uint8)
        self.graph_edge_ptr = new(self.max_graphs + 1, torch.int32)
        self.logits, self.y = new((self.max_graphs, self.logit_cols), torch.float32), new((self.max_graphs, self.y_cols), torch.float32)
        self.batch_edge_ptr = new(self.max_batches + 1, torch.int64)
        self.loss_sums = torch.zeros(3, dtype=torch.float64, device=dev)
        self.state = torch.zeros(4, dtype=torch.int64, device=dev)
        self._graph_ids = torch.arange(self.max_graphs, dtype=torch.int64, device=dev)
        self._batch_ids = torch.arange(self.max_batches, dtype=torch.int64, device=dev)

    def reset(self) -> None:
        """Empty the log: ``state`` and ``loss_sums`` are zeroed on the device, nothing is read."""
        self.state.zero_()
        self.loss_sums.zero_()

    def append(self, att, data, clf_logits, losses=None) -> None:
        """Log one batch.  ``data``: a collated batch with ``edge_index``, ``batch``, ``edge_label``, ``y`` and ``num_graphs``; for a
        ``PaddedBatch`` the real graphs and edges are counted by ``data.valid`` on the device, and ``att`` / ``clf_logits`` have capacity
        shape.  ``losses``: a device float32[3] (loss, pred, info), or None.  Never reads back (given ``data.num_graphs``)."""
        a = _att(att)
        E_cap, dev = int(a.shape[0]), a.device
        if getattr(data, "edge_label", None) is None:
            raise ValueError("EpochLog.append needs data.edge_label")
        lab = _labels(data.edge_label, E_cap)
        if not isinstance(clf_logits, torch.Tensor) or not clf_logits.is_cuda or not data.y.is_cuda:
            raise GsatHipError("dp_gsat_amd.eval_log needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
        seg = get_index(data.edge_index, int(data.batch.shape[0])).graphs(data.batch, getattr(data, "num_graphs", None))
        if seg.index.E != E_cap:
            raise ValueError(f"attention has {E_cap} entries for {seg.index.E} edges")
        G_cap = seg.G
        if clf_logits.dim() != 2 or tuple(clf_logits.shape) != (G_cap, self.logit_cols):
            raise ValueError(f"clf_logits must have shape [{G_cap}, {self.logit_cols}], one row per graph of the batch")
        if data.y.shape[0] != G_cap or data.y.numel() != G_cap * self.y_cols:
            raise ValueError(f"data.y must have {G_cap} rows of {self.y_cols} labels")
        logits = clf_logits.detach().to(torch.float32).contiguous()
        y = data.y.detach().reshape(G_cap, self.y_cols).to(torch.float32).contiguous()
        valid = getattr(data, "valid", None)
        if valid is not None and (valid.dtype != torch.int32 or valid.numel() < 4 or not valid.is_cuda):
            raise ValueError("data.valid must be an int32 ROCm tensor (N_real, E_real, B, overflow)")
        if losses is not None:
            if not isinstance(losses, torch.Tensor) or not losses.is_cuda or losses.numel() != 3:
                raise ValueError("losses must be a ROCm tensor of three entries (loss, pred, info)")
            losses = losses.detach().reshape(3).to(torch.float32).contiguous()
        eptr, eorder = seg.edge_segments[:2]
        some = lambda t: ptr(t) if t.numel() else None
        call("gsat_eval_log_append", some(a), some(lab), ptr(eptr), some(eorder), some(logits), some(y),
             ptr(valid.contiguous()) if valid is not None else None, ptr(losses) if losses is not None else None,
             E_cap, G_cap, self.logit_cols, self.y_cols, some(self.att), some(self.label), ptr(self.graph_edge_ptr), some(self.logits),
             some(self.y), ptr(self.batch_edge_ptr), ptr(self.loss_sums), ptr(self.state), self.max_edges, self.max_graphs,
             self.max_batches, stream())

    def _counts(self):
        """The first host read: ``state`` and, from the same copy, the largest logged graph and the largest logged batch (in edges)."""
        st = self.state
        zero = torch.zeros((), dtype=torch.int64, device=st.device)
        parts = [st]
        for ptr_arr, ids, count in ((self.graph_edge_ptr, self._graph_ids, st[1]), (self.batch_edge_ptr, self._batch_ids, st[2])):
            if ids.numel():
                sizes = (ptr_arr[1:] - ptr_arr[:-1]).to(torch.int64)               # beyond the count: unwritten memory, masked out
                parts.append(torch.where(ids < count, sizes, zero).max().view(1))
            else:
                parts.append(zero.view(1))
        return torch.cat(parts).tolist()

    def compute(self) -> dict:
        """Score everything logged since ``reset``: the keys of ``EvaluationMeter.compute()`` with the same meaning -- one global
        attention ROC-AUC, the mean over all graphs of hits / k, the mean over the batches of the per-batch delta-KL, class means,
        histograms and PR curve over all edges, accuracy and ROC-AUC over all graphs -- plus ``loss``, ``pred``, ``info``, the means
        over the batches (NaN when a batch was appended without ``losses``).  With ``multi_label`` also ``clf_roc_tasks``: numpy
        float64[T], the per-task ROC-AUCs whose mean over the scorable tasks ``clf_roc`` is (one ``task_auroc_counts`` call gives both), NaN
        for a task without both classes among its labelled rows.  Exactly two host reads: the counts, then the packed results.
        ValueError when an append was refused, or nothing was appended."""
        E, Gn, nb, flags, max_graph_edges, max_batch_edges = self._counts()
        if flags & FLAG_OVERFLOW:
            raise ValueError("EpochLog: flag bit 0 is set -- a padded batch did not fit its capacity (valid[3]) and was not logged")
        if flags & FLAG_FULL:
            raise ValueError("EpochLog: flag bit 1 is set -- an append would have exceeded max_edges, max_graphs or max_batches "
                             f"({self.max_edges}, {self.max_graphs}, {self.max_batches}) and was not logged")
        if nb == 0:
            raise ValueError("EpochLog.compute() before any append()")
        dev = self.state.device
        a, lab = self.att[:E], self.label[:E]
        logits, y = self.logits[:Gn], self.y[:Gn]
        f64 = lambda v: torch.full((1,), float(v), dtype=torch.float64, device=dev)
        # precision@k: the log is one collated batch whose edge order is the identity
        if Gn and E:
            hits = torch.empty(Gn, dtype=torch.int32, device=dev)
            identity = torch.arange(E, dtype=torch.int32, device=dev)
            fused = max_graph_edges <= rank_edges_lds_cap()
            ws, ws_bytes = None, 0
            if not fused:
                ws_bytes = call_size("gsat_rank_edges_workspace_bytes", E)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            call("gsat_rank_edges", ptr(a), ptr(self.graph_edge_ptr), ptr(identity), ptr(lab), E, Gn, self.k, int(max_graph_edges), 0,
                 None, None, None, ptr(hits), ptr(ws), ws_bytes, stream())
            prec = (hits.to(torch.float64).mean() / float(self.k)).view(1)
        else:
            prec = f64(0.0 if Gn else float("nan"))
        dkl = delta_kl_segments(a, lab, self.batch_edge_ptr[:nb + 1], max_batch_edges)[:, 0].double().mean().view(1)
        means = delta_kl_stats(a, lab)[1:].double()
        hist = attention_histogram(a, lab, bins=self.bins)
        acc = classifier_accuracy(logits, y, self.multi_label).view(1) if Gn else f64(float("nan"))
        binary = self.multi_label or self.logit_cols == 1
        roc_tasks = []
        if self.multi_label:            # the per-task scores ride in the same read, behind everything else
            roc, per_task = classifier_rocauc_tasks(logits, y)
            roc, roc_tasks = roc.view(1), [per_task]
        else:
            roc = classifier_rocauc(logits, y).view(1) if binary else f64(0.0)
        pr = pr_curve(hist)
        names = ("tp", "fp", "tn", "fn")
        floats = [attention_auroc(a, lab).view(1), prec, dkl, means, acc, roc, self.loss_sums / float(nb), pr["precision"], pr["recall"]] + roc_tasks
        packed = torch.cat([hist.counts.view(-1), hist.outside] + [pr[n] for n in names] +
                           [t.view(torch.int64) for t in floats]).cpu().numpy()                   # the second host read
        B = self.bins
        ints, fl = packed[:6 * B + 2], packed[6 * B + 2:].view(np.float64)
        res = {"att_auroc": float(fl[0]), f"precision@{self.k}": float(fl[1]), "delta_kl": float(fl[2]),
               "avg_signal_att_weights": float(fl[3]), "avg_bkg_att_weights": float(fl[4]), "clf_acc": float(fl[5]), "clf_roc": float(fl[6]),
               "loss": float(fl[7]), "pred": float(fl[8]), "info": float(fl[9]),
               "bkg_att_hist": ints[:B].copy(), "signal_att_hist": ints[B:2 * B].copy(), "att_outside": ints[2 * B:2 * B + 2].copy()}
        curve = {n: ints[2 * B + 2 + i * B:2 * B + 2 + (i + 1) * B].copy() for i, n in enumerate(names)}
        curve.update(precision=fl[10:10 + B].copy(), recall=fl[10 + B:10 + 2 * B].copy())
        res["pr_curve"] = curve
        if self.multi_label:
            res["clf_roc_tasks"] = fl[10 + 2 * B:].copy()
        return res


class FidelityLog:
    """``FidelityLog(max_graphs, classes, device=None)``: the device log of explanation fidelity (csrc/fidelity.hip), allocated once.
    ``append`` takes the logits of the backbone on the full batch, on the explanation alone and on the batch without the explanation and
    keeps, per graph, the three predicted classes (``cls int32[max_graphs, 3]``) and the probabilities of the class predicted from the
    full batch (``p float64[max_graphs, 3]``); ``state`` int64[4] = (graphs, batches, flags, 0) lives on the device.  ``append`` is two
    kernel launches and reads nothing, so it replays inside a captured graph (``ReplayedFidelity``).  An append that cannot be taken -- a
    padded batch whose overflow word is set (flag bit 0), or one that would exceed ``max_graphs`` (flag bit 1) -- writes nothing but
    its flag and is reported by ``compute``."""

    def __init__(self, max_graphs: int, classes: int, device=None):
        if int(max_graphs) < 0 or int(classes) < 1:
            raise ValueError("FidelityLog needs a non-negative capacity and at least one logit column")
        if int(max_graphs) >= 2 ** 31:
            raise ValueError("FidelityLog: max_graphs must be below 2**31")
        self.max_graphs, self.classes = int(max_graphs), int(classes)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise GsatHipError("dp_gsat_amd.eval_log needs a ROCm (cuda) device: the HIP path has no CPU fallback")
        self.cls = torch.empty((self.max_graphs, 3), dtype=torch.int32, device=dev)
        self.p = torch.empty((self.max_graphs, 3), dtype=torch.float64, device=dev)
        self.state = torch.zeros(4, dtype=torch.int64, device=dev)
        self._out = torch.empty(10, dtype=torch.int64, device=dev)

    def reset(self) -> None:
        """Empty the log: one kernel zeroes ``state`` (no memset node, so a captured graph may hold it), nothing is read."""
        call("gsat_fidelity_reset", ptr(self.state), stream())

    def append(self, logits_full, logits_keep, logits_drop, valid=None) -> None:
        """Log one batch: three fp32 blocks ``[G_rows, classes]``.  ``valid``: the int32[4] word of a padded batch -- the first
        ``clamp(valid[2], 0, G_rows)`` rows are logged and the others never loaded; without it every row."""
        blocks = []
        for t in (logits_full, logits_keep, logits_drop):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise GsatHipError("dp_gsat_amd.eval_log needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
            if t.dim() != 2 or int(t.shape[1]) != self.classes:
                raise ValueError(f"logits must have shape [G, {self.classes}]")
            blocks.append(t.detach().to(torch.float32).contiguous())
        rows = int(blocks[0].shape[0])
        if any(int(t.shape[0]) != rows for t in blocks):
            raise ValueError("the three logit blocks must have one row per graph of the same batch")
        if valid is not None:
            if not isinstance(valid, torch.Tensor) or valid.dtype != torch.int32 or valid.numel() < 4 or not valid.is_cuda:
                raise ValueError("valid must be an int32 ROCm tensor (N_real, E_real, B, overflow)")
            valid = valid.contiguous()
        some = lambda t: ptr(t) if t.numel() else None
        call("gsat_fidelity_append", some(blocks[0]), some(blocks[1]), some(blocks[2]), rows, self.classes,
             ptr(valid) if valid is not None else None, some(self.cls), some(self.p), ptr(self.state), self.max_graphs, stream())

    def compute(self) -> dict:
        """Score everything logged since ``reset``, with ONE reduction launch and ONE host read: ``fidelity_plus = mean(p_full - p_drop)``,
        ``fidelity_minus = mean(p_full - p_keep)``, the means ``p_full / p_keep / p_drop``, the exact flip rates ``flip_plus = #(cls_drop !=
        cls_full) / n`` and ``flip_minus = #(cls_keep != cls_full) / n``, and ``n``.  fp64 sums in a fixed order: two runs over the same log
        are bitwise equal.  ValueError when an append was refused, or nothing was appended."""
        some = lambda t: ptr(t) if t.numel() else None
        call("gsat_fidelity_reduce", some(self.cls), some(self.p), ptr(self.state), self.max_graphs, ptr(self._out), stream())
        packed = self._out.cpu().numpy()                                                        # the one host read
        n, batches, flags, flips_plus, flips_minus = (int(v) for v in packed[:5])
        if flags & FLAG_OVERFLOW:
            raise ValueError("FidelityLog: flag bit 0 is set -- a padded batch did not fit its capacity (valid[3]) and was not logged")
        if flags & FLAG_FULL:
            raise ValueError(f"FidelityLog: flag bit 1 is set -- an append would have exceeded max_graphs ({self.max_graphs}) and was "
                             "not logged")
        if batches == 0 or n == 0:
            raise ValueError("FidelityLog.compute() before any append()")
        sums = packed[5:10].view(np.float64)
        return {"fidelity_plus": float(sums[0]) / n, "fidelity_minus": float(sums[1]) / n, "p_full": float(sums[2]) / n,
                "p_keep": float(sums[3]) / n, "p_drop": float(sums[4]) / n, "flip_plus": flips_plus / n, "flip_minus": flips_minus / n,
                "n": n}


class FidelityCurveLog:
    """``FidelityCurveLog(max_graphs, classes, ks=None, ratios=None, device=None)``: :class:`FidelityLog` with a level axis, for the
    logits of a stacked batch (``dp_gsat_amd.subgraph.explanation_stack``: ``V = 2 S + 1`` blocks -- the batch, level s alone, the batch
    without level s).  ``append`` keeps, per graph, the class predicted from every block (``cls int32[max_graphs, V]``) and every block's
    probability of the class predicted from the full batch (``p float64[max_graphs, V]``); ``state`` int64[20] = (graphs, batches, flags,
    real edges, kept edges of level 0 .. 15) lives on the device.  ``append`` is two kernel launches and reads nothing, so it replays inside
    a captured graph (``ReplayedFidelityCurve``).  An append that cannot be taken -- an overflowed batch or stack (flag bit 0), or one that
    would exceed ``max_graphs`` (flag bit 1) -- writes nothing but its flag and is reported by ``compute``.

    ``rankings=R`` (``R * S`` at most 16): the log of a multi-ranking stack (``explanation_stack_multi``, ``V = 1 + 2 R S`` blocks).  The
    same kernels run with ``R * S`` flat levels -- flat level ``r * S + s`` is ranking ``r``, level ``s`` -- and ``compute`` returns the
    per-level entries as ``[R][S]`` nested lists under the same keys.  With ``rankings=1`` everything is as without it.

    ``tasks=T`` (``classes == T``, 1 to 1024; not with ``rankings > 1``): the log of a multi-label head, whose every (graph, task) is a
    binary decision of its own -- class ``z >= 0``, probability ``sigmoid(+-z)``.  ``cls`` and ``p`` become ``[max_graphs, T, V]`` (``state[0]``
    still counts graphs), ``append`` / ``compute`` go through ``gsat_fidelity_curve_append_tasks`` / ``_reduce_tasks``, and ``compute`` adds
    the per-task curves (see there).  Without ``tasks`` everything is as before."""

    def __init__(self, max_graphs: int, classes: int, ks=None, ratios=None, device=None, rankings: int = 1, tasks: Optional[int] = None):
        ks, ratios = check_levels(ks, ratios)
        self.levels, self.by_ratio = tuple(ks if ks is not None else ratios), ratios is not None
        self.rankings = check_rankings(rankings, len(self.levels))
        S = self._flat = self.rankings * len(self.levels)
        self.variants = 2 * S + 1
        if int(max_graphs) < 0 or int(classes) < 1:
            raise ValueError("FidelityCurveLog needs a non-negative capacity and at least one logit column")
        self.tasks = None
        if tasks is not None:
            if isinstance(tasks, bool) or int(tasks) != tasks or not 1 <= int(tasks) <= 1024:
                raise ValueError("FidelityCurveLog: tasks must be an int between 1 and 1024")
            if self.rankings > 1:
                raise ValueError("FidelityCurveLog: a task axis together with rankings > 1 is not covered")
            if int(classes) != int(tasks):
                raise ValueError("FidelityCurveLog: a multi-label head has one logit column per task (classes == tasks)")
            self.tasks = int(tasks)
        if int(max_graphs) * self.variants * (self.tasks or 1) >= 2 ** 31:
            raise ValueError("FidelityCurveLog: max_graphs * variants (* tasks) must be below 2**31")
        self.max_graphs, self.classes = int(max_graphs), int(classes)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise GsatHipError("dp_gsat_amd.eval_log needs a ROCm (cuda) device: the HIP path has no CPU fallback")
        shape = (self.max_graphs, self.variants) if self.tasks is None else (self.max_graphs, self.tasks, self.variants)
        self.cls = torch.empty(shape, dtype=torch.int32, device=dev)
        self.p = torch.empty(shape, dtype=torch.float64, device=dev)
        self.state = torch.zeros(20, dtype=torch.int64, device=dev)
        out_words = 5 + 7 * S if self.tasks is None else 4 + S + self.tasks * (1 + 6 * S)
        self._out = torch.empty(out_words, dtype=torch.int64, device=dev)

    def reset(self) -> None:
        """Empty the log: one kernel zeroes ``state`` (no memset node, so a captured graph may hold it), nothing is read."""
        call("gsat_fidelity_curve_reset", ptr(self.state), stream())

    def append(self, logits, stack_valid, valid=None) -> None:
        """Log one stacked batch: ``logits`` fp32 ``[V * graphs_per_variant, classes]``, ``stack_valid`` the stack's int32[V, 4].
        ``valid``: the int32[4] word of the padded batch the stack was made of -- ``clamp(valid[2], 0, graphs_per_variant)`` graphs are
        logged; without it ``stack_valid[0, 2]``.  Rows of other graphs are never loaded."""
        if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
            raise GsatHipError("dp_gsat_amd.eval_log needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
        if logits.dim() != 2 or int(logits.shape[1]) != self.classes or int(logits.shape[0]) % self.variants:
            raise ValueError(f"logits must have shape [{self.variants} * graphs_per_variant, {self.classes}]")
        z = logits.detach().to(torch.float32).contiguous()
        words = [stack_valid] + ([valid] if valid is not None else [])
        for t, n in zip(words, (4 * self.variants, 4)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.numel() < n or not t.is_cuda:
                raise ValueError("valid words must be int32 ROCm tensors: (N_real, E_real, B, overflow), one row per variant for the stack")
        entry = "gsat_fidelity_curve_append" if self.tasks is None else "gsat_fidelity_curve_append_tasks"
        call(entry, ptr(z) if z.numel() else None, int(z.shape[0]) // self.variants, self.classes, self._flat,
             ptr(valid.contiguous()) if valid is not None else None, ptr(stack_valid.contiguous()), ptr(self.cls) if self.cls.numel() else None,
             ptr(self.p) if self.p.numel() else None, ptr(self.state), self.max_graphs, stream())

    def compute(self) -> dict:
        """Score everything logged since ``reset``, with ONE reduction launch and ONE host read.  ``levels`` (the ``ks`` or ``ratios``);
        per level, as lists: ``fidelity_plus = mean(p_full - p_drop)``, ``fidelity_minus = mean(p_full - p_keep)``, ``p_keep``, ``p_drop``,
        the exact flip rates ``flip_plus = #(cls_drop != cls_full) / n`` and ``flip_minus = #(cls_keep != cls_full) / n`` and
        ``kept_fraction`` = kept edges / real edges (integer sums); ``p_full`` and ``n``.  fp64 sums in a fixed order: two runs over the same
        log are bitwise equal.  ValueError when an append was refused, or nothing was appended.

        With ``tasks=T`` every graph counts for every task.  ``fidelity_plus_tasks``, ``fidelity_minus_tasks``, ``p_keep_tasks``,
        ``p_drop_tasks``, ``flip_plus_tasks`` and ``flip_minus_tasks`` are ``[S][T]`` nested lists and ``p_full_tasks`` is ``[T]``: the means
        over the ``n`` logged graphs of one task, each from its own fixed-order fp64 sum on the device.  The keys above are then DEFINED as
        the fp64 mean over the tasks of these per-task means (``numpy.mean``, on the host after the read): the flat mean over all (graph,
        task) pairs up to rounding."""
        S = self._flat
        if self.tasks is not None:
            return self._compute_tasks(S, self.tasks)
        call("gsat_fidelity_curve_reduce", ptr(self.cls) if self.cls.numel() else None, ptr(self.p) if self.p.numel() else None,
             ptr(self.state), self.max_graphs, S, ptr(self._out), stream())
        packed = self._out.cpu().numpy()                                                        # the one host read
        n, real_edges = self._counters(packed)
        ints = packed[4:4 + 3 * S].reshape(3, S)
        sums = packed[4 + 3 * S:].view(np.float64)
        per_level = sums[1:].reshape(4, S)
        res = {"levels": list(self.levels),
               "fidelity_plus": [float(v) / n for v in per_level[2]], "fidelity_minus": [float(v) / n for v in per_level[3]],
               "p_full": float(sums[0]) / n, "p_keep": [float(v) / n for v in per_level[0]], "p_drop": [float(v) / n for v in per_level[1]],
               "flip_plus": [int(v) / n for v in ints[1]], "flip_minus": [int(v) / n for v in ints[2]],
               "kept_fraction": [int(v) / real_edges if real_edges else 0.0 for v in ints[0]], "n": n}
        if self.rankings > 1:           # flat level r * S + s is ranking r, level s
            per = len(self.levels)
            for key in ("fidelity_plus", "fidelity_minus", "p_keep", "p_drop", "flip_plus", "flip_minus", "kept_fraction"):
                res[key] = [res[key][r * per:(r + 1) * per] for r in range(self.rankings)]
        return res

    def _counters(self, packed):
        """(n, real edges) of a packed result; raises what ``compute`` raises."""
        n, batches, flags, real_edges = (int(v) for v in packed[:4])
        if flags & FLAG_OVERFLOW:
            raise ValueError("FidelityCurveLog: flag bit 0 is set -- a padded batch or a variant of its stack did not fit its capacity "
                             "(valid[3]) and was not logged")
        if flags & FLAG_FULL:
            raise ValueError(f"FidelityCurveLog: flag bit 1 is set -- an append would have exceeded max_graphs ({self.max_graphs}) and "
                             "was not logged")
        if batches == 0 or n == 0:
            raise ValueError("FidelityCurveLog.compute() before any append()")
        return n, real_edges

    def _compute_tasks(self, S, T):
        """``compute`` of a log with a task axis: one launch of T workgroups, one host read (layout: include/gsat_hip.h)."""
        call("gsat_fidelity_curve_reduce_tasks", ptr(self.cls) if self.cls.numel() else None, ptr(self.p) if self.p.numel() else None,
             ptr(self.state), self.max_graphs, S, T, ptr(self._out), stream())
        packed = self._out.cpu().numpy()                                                        # the one host read
        n, real_edges = self._counters(packed)
        A = 4 + S
        D = A + 2 * T * S
        flips = packed[A:D].reshape(2, T, S).astype(np.float64) / n                             # counts below 2^31: exact
        sums = packed[D:].view(np.float64)
        full = sums[:T] / n
        per = sums[T:].reshape(4, T, S) / n                                                     # p_keep, p_drop, p_full - p_drop, p_full - p_keep
        tasks = {"fidelity_plus": per[2], "fidelity_minus": per[3], "p_keep": per[0], "p_drop": per[1], "flip_plus": flips[0],
                 "flip_minus": flips[1]}
        res = {"levels": list(self.levels), "p_full": float(np.mean(full)), "p_full_tasks": [float(v) for v in full],
               "kept_fraction": [int(v) / real_edges if real_edges else 0.0 for v in packed[4:A]], "n": n}
        for key, a in tasks.items():                                                            # a: [T, S]
            res[key + "_tasks"] = [[float(a[t, s]) for t in range(T)] for s in range(S)]
            res[key] = [float(np.mean(np.array(row, dtype=np.float64))) for row in res[key + "_tasks"]]
        return res


def _clf_mode(multi_label: bool, logit_cols: int) -> int:
    """The mode of ``criterion_valid``: 0 binary (one logit), 1 multi-class, 2 multi-label."""
    return 2 if multi_label else (0 if logit_cols == 1 else 1)


class ClfLog:
    """``ClfLog(max_graphs, max_batches, logit_cols, y_cols=1, multi_label=False, device=None)``: the device log of a classifier epoch
    (csrc/clf_log.hip) -- what the ERM loop of src/pretrain_clf.py keeps per batch -- allocated once (plain attributes: their addresses
    never change): ``logits`` fp32[max_graphs, logit_cols], ``y`` fp32[max_graphs, y_cols] (NaN = unlabelled), ``loss_sum`` float64[1] and
    ``state`` int64[4] = (graphs, batches, flags, 0) on the device.  ``append`` is two kernel launches and reads nothing, so it replays
    inside a captured graph (``ReplayedClfStep``, ``ReplayedClfEval``); ``compute`` reads the device twice.  An append that cannot be
    taken -- a padded batch whose overflow word is set (flag bit 0), or one whose count is outside its own rows or that would exceed
    ``max_graphs`` or ``max_batches`` (flag bit 1) -- writes nothing but its flag and is reported by ``compute``.

    The predicted class is ``z > 0`` for one logit column and for a multi-label head, and the argmax (lowest index on ties) for several
    classes.  ``z > 0`` differs from ``get_preds``'s ``sigmoid(z) > 0.5`` only where the fp32 sigmoid of a non-zero ``z`` rounds to exactly
    0.5, which is ``|z|`` below about 1e-7."""

    def __init__(self, max_graphs: int, max_batches: int, logit_cols: int, y_cols: int = 1, multi_label: bool = False, device=None):
        if min(int(max_graphs), int(max_batches)) < 0 or int(logit_cols) < 1 or int(y_cols) < 1:
            raise ValueError("ClfLog needs non-negative capacities and at least one logit and one label column")
        if int(max_graphs) >= 2 ** 31:
            raise ValueError("ClfLog: max_graphs must be below 2**31")
        self.max_graphs, self.max_batches = int(max_graphs), int(max_batches)
        self.logit_cols, self.y_cols, self.multi_label = int(logit_cols), int(y_cols), bool(multi_label)
        self.mode = _clf_mode(self.multi_label, self.logit_cols)
        if self.mode == 2 and self.y_cols != self.logit_cols:
            raise ValueError("ClfLog: a multi-label head has one label column per logit column")
        if self.mode != 2 and self.y_cols != 1:
            raise ValueError("ClfLog: a single-label head has one label column")
        if (self.mode == 1 and self.logit_cols > 32) or (self.mode == 2 and self.logit_cols > 256):
            raise ValueError("ClfLog: the counting kernel takes at most 32 classes or 256 tasks")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise GsatHipError("dp_gsat_amd.eval_log needs a ROCm (cuda) device: the HIP path has no CPU fallback")
        self.logits = torch.empty((self.max_graphs, self.logit_cols), dtype=torch.float32, device=dev)
        self.y = torch.empty((self.max_graphs, self.y_cols), dtype=torch.float32, device=dev)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        self.state = torch.zeros(4, dtype=torch.int64, device=dev)
        self._words = call_size("gsat_clf_log_counts_words", self.logit_cols, self.y_cols, self.mode)
        self._out = torch.empty(self._words, dtype=torch.int64, device=dev)

    def reset(self) -> None:
        """Empty the log: ``state`` and ``loss_sum`` are zeroed on the device, nothing is read."""
        self.state.zero_()
        self.loss_sum.zero_()

    def append(self, data, clf_logits, loss=None) -> None:
        """Log one batch.  ``data``: a collated batch with ``y`` and ``num_graphs``; for a ``PaddedBatch`` the real graphs are counted by
        ``data.valid`` on the device and ``clf_logits`` has capacity shape ``[num_graphs, logit_cols]``.  ``loss``: one float on the
        device, or None (the epoch's mean loss is then NaN).  Kernels only: nothing is read back."""
        if not isinstance(clf_logits, torch.Tensor) or not clf_logits.is_cuda or not data.y.is_cuda:
            raise GsatHipError("dp_gsat_amd.eval_log needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
        G_cap = int(data.num_graphs)
        if clf_logits.dim() != 2 or tuple(clf_logits.shape) != (G_cap, self.logit_cols):
            raise ValueError(f"clf_logits must have shape [{G_cap}, {self.logit_cols}], one row per graph of the batch")
        if data.y.shape[0] != G_cap or data.y.numel() != G_cap * self.y_cols:
            raise ValueError(f"data.y must have {G_cap} rows of {self.y_cols} labels")
        logits = clf_logits.detach().to(torch.float32).contiguous()
        y = data.y.detach().reshape(G_cap, self.y_cols).to(torch.float32).contiguous()
        valid = getattr(data, "valid", None)
        if valid is not None and (valid.dtype != torch.int32 or valid.numel() < 4 or not valid.is_cuda):
            raise ValueError("data.valid must be an int32 ROCm tensor (N_real, E_real, B, overflow)")
        if loss is not None:
            if not isinstance(loss, torch.Tensor) or not loss.is_cuda or loss.numel() != 1:
                raise ValueError("loss must be a ROCm tensor of one entry")
            loss = loss.detach().reshape(1).to(torch.float32).contiguous()
        some = lambda t: ptr(t) if t.numel() else None
        call("gsat_clf_log_append", some(logits), some(y), ptr(valid.contiguous()) if valid is not None else None,
             ptr(loss) if loss is not None else None, G_cap, self.logit_cols, self.y_cols, some(self.logits), some(self.y),
             ptr(self.loss_sum), ptr(self.state), self.max_graphs, self.max_batches, stream())

    def compute(self) -> dict:
        """Score everything logged since ``reset``.  ``n``; ``clf_acc`` -- single label: trace of the confusion matrix / n; multi-label:
        ``(tn + tp)`` over all tasks / ``(n * T)``, an unlabelled entry never matching (src/pretrain_clf.py:97); ``clf_roc`` --
        ``classifier_rocauc`` on the logged rows, 0.0 for multi-class as in ``EpochLog``; ``loss`` = ``loss_sum`` / batches (NaN when a
        batch came without a loss).  Single label: ``confusion`` numpy int64[C, C] (rows the label, columns the prediction; C = 2 for one
        logit) and ``bad``, the rows with a label that is no class or a NaN logit (they match nothing).  Multi-label: ``task_counts``
        int64[T, 4] = (tn, fp, fn, tp) per task, ``unlabelled`` int64[T] and ``clf_roc_tasks`` float64[T] (NaN for a task without both
        classes).  Exactly two host reads: the counts in ``state``, then the packed results.  ValueError when an append was refused,
        or nothing was appended."""
        n, nb, flags, _ = self.state.tolist()                                                   # the first host read
        if flags & FLAG_OVERFLOW:
            raise ValueError("ClfLog: flag bit 0 is set -- a padded batch did not fit its capacity (valid[3]) and was not logged")
        if flags & FLAG_FULL:
            raise ValueError("ClfLog: flag bit 1 is set -- an append had a count outside its own rows or would have exceeded max_graphs "
                             f"or max_batches ({self.max_graphs}, {self.max_batches}) and was not logged")
        if nb == 0:
            raise ValueError("ClfLog.compute() before any append()")
        dev = self.state.device
        some = lambda t: ptr(t) if t.numel() else None
        call("gsat_clf_log_counts", some(self.logits), some(self.y), ptr(self.state), self.max_graphs, self.logit_cols, self.y_cols,
             self.mode, ptr(self._out), stream())
        logits, y = self.logits[:n], self.y[:n]
        nan = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
        # the accuracy is formed where classifier_accuracy forms it -- integer hits, one fp64 division on the device -- so the two agree
        # bit for bit on the same rows
        C = 2 if self.mode == 0 else self.logit_cols
        hits = self._out.view(C, 5)[:, (0, 3)].sum() if self.mode == 2 else self._out[:C * C].view(C, C).diagonal().sum()
        total = n * (C if self.mode == 2 else 1)
        floats = [self.loss_sum / float(nb), (hits.double() / float(total)).view(1) if total else nan]
        if self.mode == 2:
            roc, per_task = classifier_rocauc_tasks(logits, y) if n else (nan, nan.repeat(self.logit_cols))
            floats += [roc.view(1), per_task]
        elif self.mode == 0:
            floats.append(classifier_rocauc(logits, y).view(1) if n else nan)
        else:
            floats.append(torch.zeros(1, dtype=torch.float64, device=dev))
        packed = torch.cat([self._out] + [t.view(torch.int64) for t in floats]).cpu().numpy()   # the second host read
        counts, fl = packed[:self._words], packed[self._words:].view(np.float64)
        res = {"n": int(n), "loss": float(fl[0]), "clf_acc": float(fl[1]), "clf_roc": float(fl[2])}
        if self.mode == 2:
            c = counts.reshape(C, 5)
            res.update(task_counts=c[:, :4].copy(), unlabelled=c[:, 4].copy(), clf_roc_tasks=fl[3:3 + C].copy())
        else:
            res.update(confusion=counts[:C * C].reshape(C, C).copy(), bad=int(counts[C * C]))
        return res
