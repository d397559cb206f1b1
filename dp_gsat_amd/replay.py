"""A training step over a real dataset as replays of ONE captured hipGraph.

A captured step bakes N, E and G into every launch, and real batches differ in N and E from step to step.  ``ReplayedStep`` collates
every batch to a fixed capacity (PackedDataset.collate_padded) inside the captured graph, so that a step is: copy the graph ids, set
r, replay.  The padding is arithmetically inert.

The public classes say what their graphs hold (``run_once``) and what they refuse; the protocol around it -- static inputs, warm-up
on a side stream, capture, putting everything back, ``step`` -- is ``_Replayed`` and the module's functions, each written once.
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from typing import Optional

import torch

from . import explain as _explain
from ._lib import call, ptr, stream
from .collate import collate_padded_pair
from .eval_log import ClfLog, EpochLog, FidelityCurveLog, FidelityLog
from .evaluate import MAX_BINS
from .graph_index import clear_cache, get_index, set_sync_free, sync_free
from .gsat import get_r
from .ops import edge_tensor
from .padding import padded
from .subgraph import edge_subgraph_padded, explanation_stack, explanation_stack_multi, explanation_stack_nodes

_MULTI_LABEL = "a padded batch cannot take the multi-label criterion (its boolean indexing is not capturable)"
_MULTI_LABEL_HINT = _MULTI_LABEL + "; construct it as Criterion(num_class, True, capturable=True)"
_MULTI_LABEL_SINGLE = ("ReplayedFidelity does not cover the multi-label criterion; a single level of a multi-task model is "
                       "ReplayedFidelityCurve(ks=(k,)) or ReplayedFidelityCurve(ratios=(r,)) with a capturable criterion")


def _multi_label(criterion):
    return bool(getattr(criterion, "multi_label", False))


def _refuse_uncapturable(criterion):
    """The multi-label criterion is taken only when constructed as capturable."""
    if _multi_label(criterion) and not getattr(criterion, "capturable", False):
        raise ValueError(_MULTI_LABEL_HINT)


# ---- what capturing changes, and what puts it back -------------------------------------------------------------------------------------------
@contextmanager
def _kept_training_state(model, optimizers):
    """Whatever trains inside the block is undone on exit, normal or by exception: parameters, buffers and every tensor of the
    optimizers' state are copied back in place (a captured graph holds their addresses), and state tensors that did not exist on entry
    are zeroed."""
    tensors = list(model.parameters()) + list(model.buffers())
    saved = [t.detach().clone() for t in tensors]
    had_state = {id(p): {k: v.clone() for k, v in opt.state[p].items() if isinstance(v, torch.Tensor)}
                 for opt in optimizers for grp in opt.param_groups for p in grp["params"] if p in opt.state}
    try:
        yield
    finally:
        with torch.no_grad():
            for t, s in zip(tensors, saved):
                t.copy_(s)
            for opt in optimizers:
                for grp in opt.param_groups:
                    for p in grp["params"]:
                        for k, v in opt.state.get(p, {}).items():
                            if isinstance(v, torch.Tensor):
                                old = had_state.get(id(p), {}).get(k)
                                v.copy_(old) if old is not None else v.zero_()


@contextmanager
def _forward_mode(model, evaluating):
    """``sync_loss_dict`` off (the loss dict stays on the device) and, ``evaluating``, every module in ``eval()``; both are put back on
    exit.  What an evaluator's eager tail runs under."""
    modes = [(m, m.training) for m in model.modules()] if evaluating else []
    has_loss_dict = hasattr(model, "sync_loss_dict")          # a bare backbone (the classifier classes) has no loss dict
    was_loss_dict = model.sync_loss_dict if has_loss_dict else None
    if evaluating:
        model.eval()
    if has_loss_dict:
        model.sync_loss_dict = False
    try:
        yield
    finally:
        for m, t in modes:
            m.training = t
        if has_loss_dict:
            model.sync_loss_dict = was_loss_dict


@contextmanager
def _capture_mode(model, evaluating=False):
    """What warm-up and capture run under: ``sync_free`` on and ``_forward_mode``.  On exit all of it is put back and the index cache is
    emptied."""
    was_sync_free = sync_free()
    set_sync_free(True)
    try:
        with _forward_mode(model, evaluating):
            yield
    finally:
        set_sync_free(was_sync_free)
        clear_cache()


# ---- refusals, and what the two pair classes share ------------------------------------------------------------------------------------------
def _need_capturable(opt, what):
    if opt is None or not all(g.get("capturable", False) for g in opt.param_groups):
        raise ValueError(f"{what}, e.g. torch.optim.Adam(params, capturable=True, fused=True)")


def _refuse_sync_group(model):
    if any(getattr(m, "sync_group", None) for m in model.modules()):
        raise ValueError("a padded batch cannot take sync_group BatchNorm (its statistics are reduced over ranks on the host's schedule)")


def _mix_epoch(m, mixed):
    """The epoch a captured pair body passes on.  Only the mix reads it: r comes from db.r."""
    return m.mix_after_epoch + (1 if mixed else 0)


def _padded_pair_setup(obj, m, primal_ds, dual_ds, batch_size, capacity, graphs, ragged=False):
    """The refusals of a replayed padded pair (those ``DualGSAT._pair_forward_pass`` makes, before anything is captured), then the
    static inputs of the pair on ``obj``."""
    if m.primal_criterion.multi_label or m.dual_criterion.multi_label:
        raise ValueError(_MULTI_LABEL)
    if m.primal_learn_edge_att or m.dual_learn_edge_att:
        raise ValueError("a padded pair takes node attention on both sides (the MUTAG configs), not edge attention")
    primal_ds.check_pair(dual_ds)
    obj.model, obj.primal_ds, obj.dual_ds = m, primal_ds, dual_ds
    obj._setup(m, (primal_ds, dual_ds), batch_size, capacity, graphs, ragged)


def _first_budget_row(dataset, capacity, batch_size, dual=None):
    """The ids a ragged instance warms up and captures on: the first batch budget batching cuts from the dataset in storage order (of a
    pair: under its three budgets)."""
    return dataset.budget_batches(torch.arange(dataset.num_graphs), capacity, batch_size, dual=dual)[0].contiguous()


class _Replayed:
    """What the replay classes share: the static inputs of the captured graphs (``graph_ids``, ``r``), the warm-up-and-capture driver and
    ``step``.  A class with one graph is the pair (unmixed, mixed) without its mixed half.  A subclass gives ``run_once`` -- the body a
    graph holds, which ends in ``_publish`` -- and says in its constructor what it refuses."""

    def _setup(self, model, datasets, batch_size, capacity, graphs, ragged=False):
        """Validate ``batch_size`` and ``capacity`` and make the static inputs.  ``datasets``: (dataset,) for one graph (``graphs`` is
        that graph or None), (primal, dual) for the unmixed/mixed pair (``graphs`` is the pair or None)."""
        ds = datasets[0]
        self._model, self._datasets, self._pair = model, datasets, len(datasets) == 2
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= ds.num_graphs:
            raise ValueError("batch_size must be between 1 and the dataset's graph count")
        if capacity is None:
            capacity = ds.pair_capacity_for(datasets[1], self.batch_size) if self._pair else ds.capacity_for(self.batch_size)
        self.capacity = tuple(int(c) for c in capacity)
        if self._pair and len(self.capacity) != 3:
            raise ValueError("capacity is (N_cap, E_cap, E_dual_cap)")
        dev = ds.x_all.device
        self.ragged = bool(ragged)
        if self.ragged:
            self.graph_ids = _first_budget_row(ds, self.capacity, self.batch_size, datasets[1] if self._pair else None)
        else:
            self.graph_ids = torch.arange(self.batch_size, dtype=torch.int64, device=dev)
        self.r = torch.full((1,), float(self._r_of(0)), dtype=torch.float32, device=dev)
        if self._pair:
            unmixed, mixed = graphs if graphs is not None else (torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph())
            self.graphs = self._graphs = {False: unmixed, True: mixed}
        else:
            self.graph = graphs if graphs is not None else torch.cuda.CUDAGraph()
            self._graphs = {False: self.graph}
        self._outputs, self._current = {}, None

    def _r_of(self, epoch):
        m = self._model
        if not self._pair:
            return get_r(m.decay_interval, m.decay_r, epoch, final_r=m.final_r)
        return m.dual_fix_r if m.dual_fix_r else get_r(m.dual_decay_interval, m.dual_decay_r, epoch, final_r=m.dual_final_r,
                                                       init_r=m.dual_init_r)

    def _body(self, mixed):
        if self._pair:
            self.run_once(mixed)
        else:
            self.run_once()

    def _publish(self, mixed, **outputs):
        """The end of ``run_once``: ``outputs`` are what the graph ``mixed`` leaves behind, and become attributes."""
        self._outputs[mixed] = outputs
        self._select(mixed)

    def _select(self, mixed):
        for key, v in self._outputs[mixed].items():
            setattr(self, key, v)
        self._current = mixed

    def _warm_up_and_capture(self, setup=None, before_capture=None):
        """Three eager runs on a side stream -- of the one body, or unmixed, mixed, unmixed: both bodies run eagerly before either is
        captured -- after ``setup()`` on that stream; the one host read that tells whether the warm-up batch fit; ``before_capture()``;
        then one capture per graph, with no reseeding in between: both graphs draw from the one device seed stream."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            if setup is not None:
                setup()
            for mixed in ((False, True, False) if self._pair else (False, False, False)):
                self._body(mixed)
        torch.cuda.current_stream().wait_stream(side)
        if int(self.batch.valid[3]) != 0:
            raise ValueError(f"{type(self).__name__}: graphs 0..{self.batch_size - 1} do not fit the capacity {self.capacity}")
        if before_capture is not None:
            before_capture()
        for mixed, graph in self._graphs.items():
            with torch.cuda.graph(graph):
                self._body(mixed)

    def _load_ids(self, graph_ids):
        """Copy ``graph_ids`` into the static id buffer.  Ragged: 1 .. batch_size ids (or a row of ``budget_batches`` with its -1s), the
        remaining slots are emptied with -1; else exactly batch_size ids."""
        ids = torch.as_tensor(graph_ids).reshape(-1)
        n = int(ids.numel())
        if self.ragged:
            if not 1 <= n <= self.batch_size:
                raise ValueError(f"{type(self).__name__} was captured for 1 to {self.batch_size} graphs per step, got {n}")
            if n < self.batch_size:
                self.graph_ids[n:].fill_(-1)
            self.graph_ids[:n].copy_(ids, non_blocking=True)
            return
        if n != self.batch_size:
            raise ValueError(f"{type(self).__name__} was captured for {self.batch_size} graphs per step, got {n}")
        self.graph_ids.copy_(ids, non_blocking=True)

    def step(self, graph_ids, epoch: int) -> Optional[torch.Tensor]:
        """One replay on the graphs ``graph_ids`` (exactly ``batch_size`` ids -- ragged: 1 to ``batch_size``, or a row of ``batches``;
        tensor, array or list) with r = get_r(epoch); of a pair, the dual r follows its schedule and the mixed graph runs when ``epoch >
        mix_after_epoch``.  Nothing is read back.  A training class returns the device loss; an evaluator appends to its log(s) -- a dual
        one with the seed stream's next word -- and returns None.  The attributes the class docstring lists hold the replay's outputs
        until the next replay of the same graph."""
        self._load_ids(graph_ids)
        self.r.fill_(float(self._r_of(epoch)))
        mixed = self._pair and bool(epoch > self._model.mix_after_epoch)
        self._graphs[mixed].replay()
        if self._current is not mixed:          # the other graph of the pair ran last: its outputs are published
            self._select(mixed)
        return self._outputs[mixed].get("loss")

    def batches(self, perm) -> torch.Tensor:
        """``dataset.budget_batches(perm, self.capacity, self.batch_size)``: the rows to feed ``step`` of a ragged instance -- of a pair
        the three-budget rows, ``primal_ds.budget_batches(perm, self.capacity, self.batch_size, dual=dual_ds)``."""
        return self._datasets[0].budget_batches(perm, self.capacity, self.batch_size, dual=self._datasets[1] if self._pair else None)

    def check_epoch(self, perm) -> None:
        """Raise ValueError if a full batch of the epoch ``perm`` (graph ids in visiting order) exceeds the capacity -- in nodes, edges
        or, of a pair, dual edges: the totals of every ``perm[k * batch_size : (k + 1) * batch_size]`` are taken on the device and read
        back once."""
        ds, B = self._datasets[0], self.batch_size
        p = torch.as_tensor(perm).to(ds.x_all.device, torch.int64).reshape(-1)
        full = int(p.numel()) // B
        if full == 0:
            return
        p = p[: full * B].view(full, B)
        counts = [ds.node_counts, ds.edge_counts] + [d.edge_counts for d in self._datasets[1:]]
        n, *e = torch.stack([c[p].sum(1).max() for c in counts]).tolist()
        if n + 2 > self.capacity[0] or any(v > c for v, c in zip(e, self.capacity[1:])):
            names = ", ".join(("N", "E", "E_dual")[:len(counts)])
            raise ValueError(f"a batch of this epoch needs ({names}) = ({n} + 2 padding nodes, {', '.join(map(str, e))}), above the "
                             f"capacity {self.capacity}")


# ---- the training classes ---------------------------------------------------------------------------------------------------------------------
def _capture_training(rs, optimizers):
    """Make the overflow flag of a training class and capture its graphs; nothing has trained afterwards."""
    rs._overflow = torch.zeros(1, dtype=torch.int32, device=rs.r.device)
    try:
        with _kept_training_state(rs._model, optimizers), _capture_mode(rs._model):
            rs._warm_up_and_capture(None, lambda: _reset_logs(rs))      # the warm-up runs appended: the logs are empty afterwards
    finally:
        _reset_logs(rs)
    rs._overflow.zero_()


def _take_overflow(rs):
    seen = bool(int(rs._overflow))
    rs._overflow.zero_()
    return seen


def _training_log_setup(rs, log_k, bins, max_graphs, max_edges):
    """``log_k`` None: no log.  Else the sizes of the training-pass log(s) on ``rs``, refused here -- before anything is captured -- where
    ``EpochLog`` or its ``append`` would refuse them.  The logs themselves are made by the first warm-up run, which knows the logits."""
    rs.log = rs.dual_log = None
    rs._log_sizes = None
    if log_k is None:
        return
    ds = rs._datasets[0]
    if ds.edge_label_all is None or ds.y_all is None:
        raise ValueError(f"{type(rs).__name__}(log_k=) needs a dataset with edge labels and graph labels")
    rs._log_sizes = (int(log_k), int(bins), max_graphs, max_edges)


def _append_training(rs, att, dual_att, b, logits, loss_dict):
    """The end of a logging step body: append this step's training-mode attention on the edges, its logits and its (loss, pred, info) to
    ``rs.log`` -- and, where ``dual_att`` is given, the same with the dual attention to ``rs.dual_log``.  Kernels that read the step's
    outputs and write the logs' own arrays: nothing is drawn and nothing that trains is written.  Returns the [3] loss tensor."""
    with torch.no_grad():
        att, logits = edge_tensor(att).detach(), logits.detach()
        if rs.log is None:          # the first warm-up run
            logs = _new_logs(rs, 1 if dual_att is None else 2, logits, *rs._log_sizes)
            rs.log, rs.dual_log = logs[0], logs[1] if dual_att is not None else None
        losses = _loss_triple(loss_dict)
        rs.log.append(att, b, logits, losses)
        if dual_att is not None:
            rs.dual_log.append(dual_att, b, logits, losses)
    return losses


class _TrainingLog:
    """``begin_epoch`` / ``epoch_scores`` of the two training classes (constructed with ``log_k``)."""

    def begin_epoch(self) -> None:
        """Empty the training-pass log(s) on the device; nothing is read.  Without ``log_k`` there is nothing to empty."""
        _reset_logs(self)

    def epoch_scores(self) -> dict:
        """``log.compute()`` -- two host reads -- over the steps since ``begin_epoch()``: the keys ``ReplayedEval.run`` returns (with
        ``score_dual`` also the ``dual_`` keys of ``ReplayedDualEval.run``), scored on the training-mode (sampled) attention and logits each
        step produced; ``loss``, ``pred`` and ``info`` are the means over the steps.  ValueError without ``log_k``, before any step, and
        when a step since ``begin_epoch()`` did not fit the capacity (it appended nothing; ``overflowed()`` still reports it)."""
        if self.log is None:
            raise ValueError(f"{type(self).__name__} was constructed without log_k: it keeps no log of the training pass")
        return _scores(self)


class ReplayedStep(_Replayed, _TrainingLog):
    """``ReplayedStep(gsat, dataset, batch_size, capacity=None)``: captures clear_cache, collate_padded, forward_pass,
    zero_grad(set_to_none=True), backward and optimizer.step() of ``gsat`` on ``dataset`` (a PackedDataset) once, after three warm-up
    runs on a side stream.  ``gsat.optimizer`` must be capturable (``torch.optim.Adam(..., capturable=True)``).  The warm-up runs
    train on graphs 0 .. batch_size-1; parameters, buffers and optimizer state are put back afterwards, so capturing does not train.

    ``capacity`` defaults to ``dataset.capacity_for(batch_size)``, which no batch of distinct graphs exceeds; with a tighter one,
    ``check_epoch`` tells (one host read) whether an epoch's batches fit.  A tail batch of fewer than ``batch_size`` graphs is the
    caller's to run eagerly with ``dataset.collate``.

    A batch that does not fit the capacity is NOT skipped: the kernel turns it into an all-padding batch and the replay still runs,
    which pulls the BatchNorm running statistics towards 0 and takes an optimizer step on the gradients of empty graphs.  Nothing is
    read back per step, so the overflow word of every replay is OR-ed into one device flag: ``overflowed()`` (one host read, e.g. once
    per epoch) tells whether any step since the last call overflowed.  ``check_epoch`` before the epoch avoids it altogether.

    After a step: ``loss`` (device scalar), ``clf_logits`` [B + 1, C], ``batch`` (the PaddedBatch, ``batch.valid`` holds the counts) and,
    with ``keep_edge_att=True``, ``edge_att`` [E_cap, 1] -- all of capacity shape and overwritten by the next replay.
    ``graph``: an own ``torch.cuda.CUDAGraph`` to capture into (one with debug mode on, to dump it).

    ``ragged=True``: ``batch_size`` is a number of graph SLOTS.  The graph holds ``collate_padded(..., ragged=True)`` and the criterion
    reads the number of filled slots on the device, so ``step`` takes 1 to ``batch_size`` ids and no tail batch is left to run eagerly.
    ``batches(perm)`` packs an epoch into batches that fit the capacity (``PackedDataset.budget_batches``), which is what lets the
    capacity be sized near the mean batch instead of the worst one.  Warm-up and capture run on the first such batch of the dataset in
    storage order, so a capacity that graphs 0 .. batch_size-1 exceed is fine.  An overflow batch has no filled slot: its loss is exactly
    0 and neither loss term produces a gradient (the optimizer still steps on the weight decay, and BatchNorm still sees an empty
    batch).

    ``log_k=k`` (with ``bins``, ``max_graphs``, ``max_edges`` as in ``ReplayedEval``): the training pass logs itself.  ``log`` is an
    :class:`~dp_gsat_amd.eval_log.EpochLog` (the dataset needs edge labels and graph labels) and the captured body ends in
    ``log.append`` of the step's training-mode (sampled) attention on the edges, the padded batch, the logits and the (loss, pred, info)
    of its loss dict -- two more launches per replay, also kept in ``losses`` [3].  ``begin_epoch()`` empties the log and
    ``epoch_scores()`` scores the steps since: what the reference's ``run_one_epoch(..., 'train')`` returns, without a second pass over
    the training ids and without eager work per step::

        rs.begin_epoch()
        for row in rs.batches(perm):                  # ragged: every batch is a replay
            rs.step(row, epoch)
        train_res = rs.epoch_scores()                 # att_auroc, precision@k, clf_acc, clf_roc, loss, pred, info, ...

    A fixed-count instance leaves the tail batch to the caller, and so its append: after the eager step on ``b = dataset.collate(tail)``,
    ``rs.log.append(att, b, logits, torch.stack([ld["loss"], ld["pred"], ld["info"]]))`` (with ``gsat.sync_loss_dict = False``, or
    ``torch.tensor([...], device=...)`` of the floats).  Warm-up and capture leave the log empty.  Logging reads the step's outputs and
    writes only the log: it draws nothing from the device seed stream or torch's generators and touches no parameter, buffer or
    optimizer state, so a run with ``log_k`` trains bit for bit like one without.  A step that did not fit the capacity appends nothing
    and makes ``epoch_scores()`` raise.  Without ``log_k`` the captured graph is the one described above, launch for launch.

    Multi-task datasets: a model whose criterion is ``Criterion(T, True, capturable=True)`` is taken, ``ragged`` or not (without
    ``capturable=True`` the multi-label criterion stays refused, with a ValueError that names the keyword).  The criterion kernels count
    the labelled entries of the real graphs on the device; an overflow batch counts none, so its prediction loss is exactly 0.  With
    ``log_k`` the log is made with the criterion's ``multi_label`` and ``epoch_scores()`` adds ``clf_roc_tasks``.  An OGB-style dataset
    has no edge labels, and ``log_k`` needs some: pack it with ``edge_label_all = zeros(E)`` -- the reference zero-fills ``edge_label``
    (src/utils/utils.py:31-32) -- and ``att_auroc`` and ``precision@k`` are then 0 by the one-class rule, as the reference reports them."""

    def __init__(self, gsat, dataset, batch_size: int, capacity: Optional[tuple] = None, keep_edge_att: bool = False, graph=None,
                 ragged: bool = False, log_k: Optional[int] = None, bins: int = 64, max_graphs: Optional[int] = None,
                 max_edges: Optional[int] = None):
        _check_log_sizes(log_k, bins)
        _need_capturable(gsat.optimizer, "ReplayedStep needs a capturable optimizer")
        _refuse_uncapturable(gsat.criterion)
        self.gsat, self.dataset = gsat, dataset
        self._setup(gsat, (dataset,), batch_size, capacity, graph, ragged)
        _training_log_setup(self, log_k, bins, max_graphs, max_edges)
        self.keep_edge_att = bool(keep_edge_att)
        self.batch = self.loss = self.clf_logits = self.edge_att = self.losses = None
        _capture_training(self, (gsat.optimizer,))

    def run_once(self):
        """The step body (what the graph holds), run on the current stream."""
        gsat = self.gsat
        clear_cache()
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        b.r = self.r
        self._overflow.bitwise_or_(b.valid[3:4])
        att, loss, loss_dict, logits = gsat.forward_pass(b, 0, True)
        gsat.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        gsat.optimizer.step()
        extra = {} if self._log_sizes is None else {"losses": _append_training(self, att, None, b, logits, loss_dict)}
        self._publish(False, batch=b, loss=loss.detach(), clf_logits=logits.detach(),
                      edge_att=edge_tensor(att).detach() if self.keep_edge_att else None, **extra)

    def overflowed(self) -> bool:
        """True if a step since the last call (or since capture) got a batch that did not fit the capacity.  One host read; clears
        the flag."""
        return _take_overflow(self)


class ReplayedDualStep(_Replayed, _TrainingLog):
    """``ReplayedDualStep(dual_gsat, primal_ds, dual_ds, batch_size, capacity=None)``: the dual/primal training step (DualGSAT) over a
    dataset and its dual (``primal_ds.line_graph_dataset()``) as replays of captured hipGraphs.  One replay holds clear_cache,
    collate_padded_pair, dual_forward_pass, both zero_grad(set_to_none=True), the backward and both optimizer steps.  Both optimizers
    must be capturable.  Whether the dual attention is mixed into the primal one (``epoch > mix_after_epoch``) is a host branch, so TWO
    graphs are captured -- unmixed and mixed -- over the same parameters and optimizer state, and ``step(ids, epoch)`` picks one; the
    unmixed graph is arithmetically the eager step (and keeps PNA's lazy lift).  Three warm-up runs on a side stream precede the
    captures; parameters, buffers and both optimizers' state are put back afterwards, so capturing does not train.

    ``capacity = (N_cap, E_cap, E_dual_cap)`` defaults to ``primal_ds.pair_capacity_for(dual_ds, batch_size)``.  Overflow is joint
    (collate_padded_pair) and handled as in ``ReplayedStep``: ``overflowed()`` / ``check_epoch``.

    ``pinned=True``: the graphs read their randomness from static capacity-shaped buffers instead of drawing it -- ``primal_noise``
    [N_cap, 1] and ``dual_noise`` [E_cap + 2, 1] (uniform), ``primal_masks`` / ``dual_masks`` (the extractors' two dropout keep-masks) --
    which the caller may overwrite between steps.  The default draws fresh noise inside the graph on every replay.

    After a step: ``loss`` (device scalar), ``clf_logits`` [B + 1, C] (primal), ``batch`` / ``dual_batch`` (the padded pair) and, with
    ``keep_edge_att=True``, ``edge_att`` [E_cap, 1]; all overwritten by the next replay of the same graph.  ``p.grad`` of every
    parameter points at the gradients of the graph that ran last.  ``graphs``: an own pair of ``torch.cuda.CUDAGraph`` (unmixed, mixed) to
    capture into (with debug mode on, to dump them).

    ``ragged=True``: as in ``ReplayedStep`` -- ``batch_size`` graph slots; both graphs hold ``collate_padded_pair(..., ragged=True)`` and
    both criteria read the number of filled slots on the device, so ``step`` takes 1 to ``batch_size`` ids (or a row of ``batches``) and no
    tail batch is left to run eagerly.  ``batches(perm)`` packs an epoch under the three budgets (nodes, edges, dual edges), which lets
    the capacity be sized near the mean batch.  Warm-up and capture run on the first such batch of the dataset in storage order.  An
    overflow pair has no filled slot: both criteria give 0, the f1 term its constant 1.

    ``log_k=k``: as in ``ReplayedStep`` -- both graphs end in ``log.append`` of what ``dual_train_one_batch`` returns and
    ``ReplayedDualEval`` logs: the primal attention on the edges (mixed, in the mixed graph), the primal logits and the loss dict, whose
    ``pred`` and ``info`` are the dual model's.  ``score_dual=True`` keeps a second log, ``dual_log``, of the dual attention on the primal
    edge slots (``dual_att`` [E_cap, 1] after a step), and ``epoch_scores()`` adds its attention scores under the ``dual_`` prefix of
    ``ReplayedDualEval.run``.  ``begin_epoch()`` empties both logs."""

    def __init__(self, dual_gsat, primal_ds, dual_ds, batch_size: int, capacity: Optional[tuple] = None, pinned: bool = False,
                 keep_edge_att: bool = False, graphs=None, ragged: bool = False, log_k: Optional[int] = None, score_dual: bool = False,
                 bins: int = 64, max_graphs: Optional[int] = None, max_edges: Optional[int] = None):
        m = dual_gsat
        _check_log_sizes(log_k, bins)
        if score_dual and log_k is None:
            raise ValueError("score_dual scores a second training-pass log: it needs log_k")
        for side, opt in (("primal", m.primal_optimizer), ("dual", m.dual_optimizer)):
            _need_capturable(opt, f"ReplayedDualStep needs a capturable {side} optimizer")
        _padded_pair_setup(self, m, primal_ds, dual_ds, batch_size, capacity, graphs, ragged)
        _training_log_setup(self, log_k, bins, max_graphs, max_edges)
        self.score_dual = bool(score_dual)
        dev = primal_ds.x_all.device
        self.keep_edge_att, self.pinned = bool(keep_edge_att), bool(pinned)
        self.primal_noise = self.dual_noise = self.primal_masks = self.dual_masks = None
        if self.pinned:
            N_cap, E_cap, _ = self.capacity
            self.primal_noise = torch.empty(N_cap, 1, device=dev).uniform_(1e-10, 1 - 1e-10)
            self.dual_noise = torch.rand(E_cap + 2, 1, device=dev)
            self.primal_masks = self._keep_masks(m.primal_extractor, N_cap, dev)
            self.dual_masks = self._keep_masks(m.dual_extractor, E_cap + 2, dev)
        self.batch = self.dual_batch = self.loss = self.clf_logits = self.edge_att = self.losses = self.dual_att = None
        self._grads = {}
        _capture_training(self, (m.primal_optimizer, m.dual_optimizer))

    @staticmethod
    def _keep_masks(extractor, rows, dev):
        l1, l2, _ = extractor.mlp.linears()
        keep = 1.0 - float(extractor.mlp.dropout_p)
        return [(torch.rand(rows, int(l.weight.shape[0]), device=dev) < keep).float() for l in (l1, l2)]

    def run_once(self, mixed: bool):
        """The step body (what one graph holds), run on the current stream."""
        m = self.model
        clear_cache()
        pb, db = collate_padded_pair(self.primal_ds, self.dual_ds, self.graph_ids, self.capacity, ragged=self.ragged)
        db.r = self.r
        self._overflow.bitwise_or_(pb.valid[3:4])
        kept = m.keep_dual_att
        m.keep_dual_att = kept or self.score_dual
        try:
            att, loss, loss_dict, logits = m.dual_forward_pass(pb, db, _mix_epoch(m, mixed), True, self.primal_noise, self.dual_noise,
                                                               self.primal_masks, self.dual_masks)
            dual_att = m.dual_att[:self.capacity[1]] if self.score_dual else None
        finally:
            if self.score_dual:
                m.keep_dual_att, m.dual_att = kept, None
        m.primal_optimizer.zero_grad(set_to_none=True)
        m.dual_optimizer.zero_grad(set_to_none=True)
        loss.backward()
        m.primal_optimizer.step()
        m.dual_optimizer.step()
        self._grads[mixed] = [(p, p.grad) for opt in (m.primal_optimizer, m.dual_optimizer) for grp in opt.param_groups
                              for p in grp["params"]]
        extra = {} if self._log_sizes is None else {"losses": _append_training(self, att, dual_att, pb, logits, loss_dict),
                                                    "dual_att": dual_att}
        self._publish(mixed, batch=pb, dual_batch=db, loss=loss.detach(), clf_logits=logits.detach(),
                      edge_att=edge_tensor(att).detach() if self.keep_edge_att else None, **extra)

    def _select(self, mixed):
        for p, g in self._grads[mixed]:          # each graph wrote the gradients into tensors of its own
            p.grad = g
        super()._select(mixed)

    def overflowed(self) -> bool:
        """True if a step since the last call (or since capture) got a pair that did not fit the capacity.  One host read; clears the flag."""
        return _take_overflow(self)


# ---- the evaluators ---------------------------------------------------------------------------------------------------------------------------
def _new_logs(ev, count, logits, k, bins, max_graphs, max_edges):
    """``count`` EpochLogs for the evaluator ``ev``, whose forward gives ``logits``.  ``max_graphs`` / ``max_edges`` default to the
    dataset's totals."""
    ds = ev._datasets[0]
    y_cols = int(ds.y_all.numel() // max(int(ds.y_all.shape[0]), 1))
    mg = ds.num_graphs if max_graphs is None else int(max_graphs)
    me = int(ds.edge_local_all.shape[1]) if max_edges is None else int(max_edges)
    # budget batching may close a batch after any graph: at worst one graph per batch
    most = mg if ev.ragged else -(-mg // ev.batch_size)
    multi = _multi_label(getattr(ev._model, "criterion", None))           # a DualGSAT has refused its multi-label criteria
    return [EpochLog(k, mg, me, max(most, 1), int(logits.shape[1]), y_cols, bins, multi, ds.x_all.device) for _ in range(count)]


def _check_log_sizes(k, bins):
    """What ``EpochLog`` refuses of ``log_k`` (None: no log) and ``bins``, said before anything is captured."""
    if k is None:
        return
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("log_k must be a positive int (the k of precision@k), or None for no log")
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f"need 1 <= bins <= {MAX_BINS}")


def _loss_triple(loss_dict):
    return torch.stack([loss_dict[key].reshape(()) for key in ("loss", "pred", "info")]).to(torch.float32)


_DUAL_SCORES = ("att_auroc", "precision@{k}", "delta_kl", "avg_signal_att_weights", "avg_bkg_att_weights")


def _reset_logs(ev):
    for log in (ev.log, getattr(ev, "dual_log", None)):
        if log is not None:
            log.reset()
    if getattr(ev, "components", None) is not None:
        _explain.level_components_reset(ev.components)


def _max_seg_nodes(dataset, what):
    """The dataset's largest node count for a captured ``level_components`` (one host read); ValueError above its cap."""
    n = int(dataset.node_counts.max()) if dataset.num_graphs else 0
    if n > _explain.components_lds_cap():
        raise ValueError(f"{what}'s largest graph has {n} nodes, above components_lds_cap() = {_explain.components_lds_cap()}: "
                         "connectivity=True cannot take it")
    return n


def _components(b, level, S, max_seg_nodes, out):
    """``level_components`` of the level row ``level`` on the real batch ``b`` (padded: without its padding graph) into ``out``."""
    valid = getattr(b, "valid", None)
    G = int(b.num_graphs)
    _explain.level_components(b.edge_index, b.batch, level, S, num_graphs=G, max_seg_nodes=max_seg_nodes,
                              ranked_graphs=G - 1 if valid is not None else None, valid=valid, out=out)


def _scores(ev):
    """``log.compute()`` and, from a second log of the dual attention, its attention scores under a ``dual_`` prefix."""
    res = ev.log.compute()
    if getattr(ev, "dual_log", None) is not None:
        dual = ev.dual_log.compute()
        for key in _DUAL_SCORES:
            key = key.format(k=ev.log.k)
            res["dual_" + key] = dual[key]
    return res


def _capture_evaluator(ev, make_logs):
    """Capture the graphs of the evaluator ``ev`` in eval mode; ``make_logs()`` runs on the side stream ahead of the warm-up.  The logs
    are empty afterwards."""
    try:
        with _capture_mode(ev._model, evaluating=True):
            ev._warm_up_and_capture(make_logs, lambda: _reset_logs(ev))
    finally:
        _reset_logs(ev)


def _run_epoch(ev, graph_ids, epoch):
    """Reset the logs, replay every full batch (ragged: every row of ``batches``), run the tail eagerly in eval mode, compute."""
    ids = torch.as_tensor(graph_ids).reshape(-1)
    B, n = ev.batch_size, int(ids.numel())
    _reset_logs(ev)
    rows, left = (ev.batches(ids), 0) if ev.ragged else ([ids[s:s + B] for s in range(0, n - B + 1, B)], n % B)
    for row in rows:
        ev.step(row, epoch)
    if left:
        with _forward_mode(ev._model, True):
            tail = ids[n - left:].to(ev.graph_ids.device, torch.int64)
            ev._forward(*[ds.collate(tail) for ds in ev._datasets], epoch)
    return _scores(ev)


class ReplayedEval(_Replayed):
    """``ReplayedEval(gsat, dataset, batch_size, k, capacity=None, bins=64, max_graphs=None, max_edges=None)``: an evaluation epoch over
    ``dataset`` (a PackedDataset with ``edge_label_all``) as replays of ONE captured hipGraph that holds clear_cache, collate_padded,
    ``gsat.forward_pass(b, 0, False)`` under ``torch.no_grad()`` with every module in ``eval()`` mode, and ``log.append`` into an
    :class:`~dp_gsat_amd.eval_log.EpochLog` (``log``).  Three warm-up runs on a side stream precede the capture; the modules' training
    flags, ``sync_free`` and ``sync_loss_dict`` are put back afterwards and the log is reset.  No optimizer is needed.

    The graph reads the parameters and the BatchNorm running statistics where they live, so a replay after ``ReplayedStep.step`` (or an
    eager optimizer step) scores the new weights.  It writes none of them, draws no noise and no dropout mask, and leaves the device seed
    stream alone: evaluating between training steps does not change the training run.

    ``max_graphs`` / ``max_edges`` (the log's capacities) default to the dataset's totals; a batch that does not fit ``capacity``, or an
    append that does not fit the log, is refused on the device and raised by ``run`` / ``log.compute()``; ``check_epoch`` tells beforehand
    whether an epoch's full batches fit ``capacity``.

    After a step: ``edge_att`` [E_cap, 1], ``clf_logits`` [B + 1, C], ``losses`` [3] and ``batch`` hold the replay's outputs until the next.

    Refused with ValueError, like the padded path: a multi-label criterion that was not constructed with ``capturable=True``,
    ``sync_group`` BatchNorm, and ``DualGSAT`` (see ``ReplayedDualEval``).

    Multi-task datasets: with ``Criterion(T, True, capturable=True)`` the log is an ``EpochLog(..., multi_label=True)`` whose ``y_cols``
    is the dataset's label width, and ``run`` adds ``clf_roc_tasks`` (numpy float64[T], NaN for a task without both classes among its
    labelled rows) to ``clf_roc``, the ogb mean over the scorable tasks.  A dataset without edge labels -- the OGB sets -- is packed with
    ``edge_label_all = zeros(E)``, as the reference zero-fills ``edge_label`` (src/utils/utils.py:31-32): ``att_auroc`` and
    ``precision@k`` are then 0 by the one-class rule, as the reference reports them (run_gsat.py:761-763).

    ``ragged=True``: as in ``ReplayedStep`` -- ``batch_size`` graph slots, ``step`` takes 1 to ``batch_size`` ids, and ``run`` packs its ids
    with ``budget_batches`` and replays EVERY batch: there is no eager tail.  The log then has room for one batch per graph."""

    def __init__(self, gsat, dataset, batch_size: int, k: int, capacity: Optional[tuple] = None, bins: int = 64,
                 max_graphs: Optional[int] = None, max_edges: Optional[int] = None, graph=None, ragged: bool = False):
        if hasattr(gsat, "dual_forward_pass") or not hasattr(gsat, "forward_pass"):
            raise ValueError("ReplayedEval replays GSAT.forward_pass; the dual/primal evaluation (DualGSAT) is ReplayedDualEval's")
        _refuse_uncapturable(gsat.criterion)
        _refuse_sync_group(gsat)
        if dataset.edge_label_all is None or dataset.y_all is None:
            raise ValueError("ReplayedEval needs a dataset with edge labels and graph labels")
        self.gsat, self.dataset = gsat, dataset
        self._setup(gsat, (dataset,), batch_size, capacity, graph, ragged)
        self.log = self.batch = self.clf_logits = self.edge_att = self.losses = None
        sizes = (int(k), int(bins), max_graphs, max_edges)
        _capture_evaluator(self, lambda: self._make_log(sizes))

    def _make_log(self, sizes):
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        with torch.no_grad():
            logits = self.gsat.forward_pass(b, 0, False)[3]
        self.log, = _new_logs(self, 1, logits, *sizes)

    def _forward(self, b, epoch):
        """Append the eval-mode forward of batch ``b`` to the log; the modules are in eval mode and sync_loss_dict is off."""
        with torch.no_grad():
            att, _, ld, logits = self.gsat.forward_pass(b, epoch, False)
            losses = _loss_triple(ld)
            att = edge_tensor(att)
            self.log.append(att, b, logits, losses)
        return att, logits, losses

    def run_once(self):
        """The body of the captured graph, run on the current stream."""
        clear_cache()
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        b.r = self.r
        att, logits, losses = self._forward(b, 0)
        self._publish(False, edge_att=att, clf_logits=logits, losses=losses, batch=b)

    def run(self, graph_ids, epoch: int) -> dict:
        """One evaluation epoch over ``graph_ids`` (any number, in visiting order): the log is reset, every full batch is a replay, the
        tail of fewer than ``batch_size`` graphs runs eagerly (``dataset.collate``, the same eval-mode forward, the same append), and
        ``log.compute()`` -- two host reads -- gives the scores.  Ragged: the ids are packed by ``batches`` and every batch is a replay."""
        return _run_epoch(self, graph_ids, epoch)


# The (base, counter) states of every ReplayedDualEval: a captured graph holds its state's address in a gsat_seed_next node, so a state
# is written in place and lives as long as the process.
_EVAL_SEED_STATES = []


class ReplayedDualEval(_Replayed):
    """``ReplayedDualEval(dual_gsat, primal_ds, dual_ds, batch_size, k, capacity=None, bins=64, max_graphs=None, max_edges=None,
    score_dual=False, seed=None, graphs=None)``: a dual/primal evaluation epoch (``dual_eval_one_batch`` over a dataset and its dual) as
    replays of captured hipGraphs.  One replay holds clear_cache, collate_padded_pair, one gsat_seed_next, ``dual_forward_pass(pb, db,
    epoch, False, dual_seed=word)`` under ``torch.no_grad()`` with every module in ``eval()`` mode, and ``log.append`` of the primal
    attention, the primal logits and the (loss, pred, info) triple of the returned loss dict into an
    :class:`~dp_gsat_amd.eval_log.EpochLog` (``log``).  As in ``ReplayedDualStep`` the mix is a host branch: TWO graphs (unmixed, mixed)
    over the same parameters, and ``step`` / ``run`` pick one by ``epoch > mix_after_epoch``.  Three warm-up runs on a side stream
    precede the captures; training flags, ``sync_free`` and ``sync_loss_dict`` are put back afterwards and the logs are reset.

    The dual attention is Gumbel-sampled in eval mode too (``gumbel_noise_in_eval``).  Its uniform is drawn inside the sampler kernel
    (``gumbel_sigmoid(seed=)``) from a seed stream of the evaluator's own: ``seed_state`` = int64[2] (base, counter); ``base`` is ``seed``,
    or derived from ``torch.initial_seed()`` without drawing from any generator.  ``run(ids, epoch)`` restarts it at ``(base, epoch <<
    32)``, so batch j of the run uses the word gsat_seed_next gives for the counter ``(epoch << 32) + j`` and an evaluation epoch is a
    function of the weights, the ids, the epoch and the base alone.  Neither ``device_seed()``'s stream nor torch's CUDA or CPU generator
    is touched: evaluating between ``ReplayedDualStep`` steps leaves the training run bitwise unchanged.  With
    ``gumbel_noise_in_eval=False`` nothing is drawn and the counter does not move.

    ``score_dual=True``: a second log, ``dual_log``, takes the same primal batches with the dual attention on the primal edge slots in
    place of the primal attention (dual node row k is primal edge slot k), and ``run`` adds its attention scores under a ``dual_`` prefix.

    After a step: ``edge_att`` [E_cap, 1], ``dual_att`` [E_cap, 1], ``clf_logits`` [B + 1, C], ``losses`` [3], ``batch`` and ``dual_batch``
    hold the replay's outputs until the next replay of the same graph.

    Refused with ValueError before anything is captured: what a padded pair refuses (the multi-label criterion, edge attention,
    ``check_pair``, a capacity that is no triple), ``sync_group`` BatchNorm, a model without ``dual_forward_pass`` and a dataset without
    edge labels or graph labels.  Overflow of the joint capacity sets the log's flag bit 0 and is raised by ``run``; ``check_epoch``
    tells beforehand.

    ``ragged=True``: as in ``ReplayedEval`` -- ``batch_size`` graph slots, ``step`` takes 1 to ``batch_size`` ids, and ``run`` packs its ids
    under the three budgets (``batches``) and replays EVERY batch: no eager tail, no ``collate``.  The logs then have room for one batch
    per graph.  The seed stream advances by one word per batch as before, so batch j of a run is the j-th row of ``batches``."""

    def __init__(self, dual_gsat, primal_ds, dual_ds, batch_size: int, k: int, capacity: Optional[tuple] = None, bins: int = 64,
                 max_graphs: Optional[int] = None, max_edges: Optional[int] = None, score_dual: bool = False, seed: Optional[int] = None,
                 graphs=None, ragged: bool = False):
        m = dual_gsat
        if not hasattr(m, "dual_forward_pass"):
            raise ValueError("ReplayedDualEval replays DualGSAT.dual_forward_pass; ReplayedEval covers a plain GSAT")
        _refuse_sync_group(m)
        if primal_ds.edge_label_all is None or primal_ds.y_all is None or dual_ds.y_all is None:
            raise ValueError("ReplayedDualEval needs datasets with edge labels (primal) and graph labels")
        _padded_pair_setup(self, m, primal_ds, dual_ds, batch_size, capacity, graphs, ragged)
        if seed is None:        # a fixed mix of torch.initial_seed(): follows torch.manual_seed, draws nothing
            seed = (torch.initial_seed() * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & 0x7FFFFFFFFFFFFFFF
        self.base = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.seed_state = torch.empty(2, dtype=torch.int64, device=primal_ds.x_all.device)
        _EVAL_SEED_STATES.append(self.seed_state)
        self._set_seed_state(0)
        self.score_dual = bool(score_dual)
        self.log = self.dual_log = None
        self.batch = self.dual_batch = self.edge_att = self.clf_logits = self.losses = self.dual_att = None
        sizes = (int(k), int(bins), max_graphs, max_edges)
        try:
            _capture_evaluator(self, lambda: self._make_logs(sizes))
        finally:
            self._set_seed_state(0)

    def _set_seed_state(self, counter):
        signed = lambda v: v - (1 << 64) if v >= 1 << 63 else v
        self.seed_state.copy_(torch.tensor([signed(self.base), signed(int(counter) & 0xFFFFFFFFFFFFFFFF)], dtype=torch.int64))

    def _make_logs(self, sizes):
        pb, db = collate_padded_pair(self.primal_ds, self.dual_ds, self.graph_ids, self.capacity, ragged=self.ragged)
        with torch.no_grad():
            logits = self.model.dual_forward_pass(pb, db, 0, False, dual_seed=0)[3]
        logs = _new_logs(self, 2 if self.score_dual else 1, logits, *sizes)
        self.log, self.dual_log = logs[0], logs[1] if self.score_dual else None

    def _forward(self, pb, db, epoch):
        """Append the eval-mode forward of the pair (padded or not) to the log(s), with the stream's next seed word when noise is drawn;
        the modules are in eval mode and sync_loss_dict is off.  Returns (primal attention, logits, losses, dual attention on the primal
        edges, seed word)."""
        m = self.model
        word = None
        if m.gumbel_noise_in_eval:
            word = torch.empty(1, dtype=torch.int64, device=self.seed_state.device)
            call("gsat_seed_next", ptr(self.seed_state), ptr(word), stream())
        kept = m.keep_dual_att
        m.keep_dual_att = True
        try:
            with torch.no_grad():
                att, _, ld, logits = m.dual_forward_pass(pb, db, epoch, False, dual_seed=word)
                losses = _loss_triple(ld)
                att = edge_tensor(att)
                dual_att = m.dual_att[:att.shape[0]]
                self.log.append(att, pb, logits, losses)
                if self.dual_log is not None:
                    self.dual_log.append(dual_att, pb, logits, losses)
        finally:
            m.keep_dual_att, m.dual_att = kept, None
        return att, logits, losses, dual_att, word

    def run_once(self, mixed: bool):
        """The body of one captured graph, run on the current stream."""
        clear_cache()
        pb, db = collate_padded_pair(self.primal_ds, self.dual_ds, self.graph_ids, self.capacity, ragged=self.ragged)
        db.r = self.r
        att, logits, losses, dual_att, word = self._forward(pb, db, _mix_epoch(self.model, mixed))
        self._publish(mixed, batch=pb, dual_batch=db, edge_att=att, clf_logits=logits, losses=losses, dual_att=dual_att, _word=word)

    def run(self, graph_ids, epoch: int) -> dict:
        """One evaluation epoch over ``graph_ids`` (any number, in visiting order) at ``epoch``: the seed stream restarts at (base, epoch <<
        32) and the logs are reset; every full batch is a replay, the tail of fewer than ``batch_size`` graphs runs eagerly (both
        datasets' ``collate``, the same eval-mode forward with the next seed word, the same appends), and ``log.compute()`` gives the
        scores -- with ``score_dual`` also ``dual_att_auroc``, ``dual_precision@k``, ``dual_delta_kl``, ``dual_avg_signal_att_weights`` and
        ``dual_avg_bkg_att_weights`` of the dual attention.  Ragged: the ids are packed by ``batches`` and every batch is a replay."""
        self._set_seed_state(int(epoch) << 32)
        return _run_epoch(self, graph_ids, epoch)


# ---- the classifier alone: ERM pre-training and its evaluation ------------------------------------------------------------------------------
@contextmanager
def _module_modes(model, training):
    """Every module of ``model`` in ``train()`` or ``eval()`` mode inside the block; the flags are put back on exit."""
    modes = [(m, m.training) for m in model.modules()]
    model.train(training)
    try:
        yield
    finally:
        for m, t in modes:
            m.training = t


def _clf_forward(model, criterion, b):
    """``model(x, edge_index, batch, edge_attr)`` -- no attention -- and the criterion, on a collated batch.  A padded batch runs inside
    ``padded(b.valid, capacity)`` and its criterion follows the rule of ``GSAT._forward_pass``: the static slice ``[:B]``; ragged, or with a
    ``capturable`` criterion, the count of real graphs from ``valid`` on the device.  Returns (logits, loss)."""
    valid = getattr(b, "valid", None)
    if valid is None:
        logits = model(b.x, b.edge_index, b.batch, edge_attr=b.edge_attr)
        return logits, criterion(logits, b.y)
    N = int(b.x.shape[0])
    with padded(valid, (N, int(b.edge_index.shape[1]))):
        get_index(b.edge_index, N).graphs(b.batch, int(b.num_graphs))       # primes the segment cache without batch.max() (a sync)
        logits = model(b.x, b.edge_index, b.batch, edge_attr=b.edge_attr)
        B = int(b.num_graphs) - 1                                           # the padding graph is the last one
        g_valid = valid[2:3] if getattr(b, "ragged", False) else None
        if g_valid is None and getattr(criterion, "capturable", False):
            g_valid = valid[2:3] * (1 - valid[3:4])                         # a fixed-count batch keeps B in valid[2] when it overflows
        loss = criterion(logits[:B], b.y[:B]) if g_valid is None else criterion(logits[:B], b.y[:B], g_valid=g_valid)
    return logits, loss


def _new_clf_log(rs, logits, max_graphs, max_batches):
    """The ``ClfLog`` of a classifier class whose forward gives ``logits``; the capacities default to the dataset's graph count and to
    the most batches an epoch over it can have (budget batching may close a batch after any graph)."""
    ds = rs._datasets[0]
    y_cols = int(ds.y_all.numel() // max(int(ds.y_all.shape[0]), 1))
    mg = ds.num_graphs if max_graphs is None else int(max_graphs)
    most = (mg if rs.ragged else -(-mg // rs.batch_size)) if max_batches is None else int(max_batches)
    return ClfLog(mg, max(most, 1), int(logits.shape[1]), y_cols, _multi_label(rs.criterion), ds.x_all.device)


def _clf_refusals(name, model, criterion, dataset):
    if hasattr(model, "forward_pass"):
        raise ValueError(f"{name} replays a bare backbone (get_model); a GSAT model is ReplayedStep's / ReplayedEval's")
    _refuse_uncapturable(criterion)
    _refuse_sync_group(model)
    if getattr(dataset, "y_all", None) is None:
        raise ValueError(f"{name} needs a dataset with graph labels (y_all)")


class _ReplayedClf(_Replayed):
    """``_Replayed`` for a bare classifier: no attention, so no r schedule -- the static ``r`` stays 0 and nothing reads it."""

    def _r_of(self, epoch):
        return 0.0

    def step(self, graph_ids, epoch: int = 0) -> Optional[torch.Tensor]:
        """One replay on the graphs ``graph_ids`` (exactly ``batch_size`` ids -- ragged: 1 to ``batch_size``, or a row of ``batches``).
        ``epoch`` is accepted and ignored: the classifier has no schedule.  Nothing is read back; returns the device loss."""
        return super().step(graph_ids, 0)


class ReplayedClfStep(_ReplayedClf):
    """``ReplayedClfStep(model, criterion, optimizer, dataset, batch_size, capacity=None, graph=None, ragged=False, log=False,
    max_graphs=None, max_batches=None)``: the ERM training step of src/pretrain_clf.py (``train_one_batch``) on a bare backbone
    (``get_model``) as replays of ONE captured hipGraph.  The graph holds clear_cache, ``collate_padded(..., ragged=)``, inside
    ``padded(b.valid, capacity)`` the forward ``model(b.x, b.edge_index, b.batch, edge_attr=b.edge_attr)`` in training mode, the
    criterion, ``zero_grad(set_to_none=True)``, backward and ``optimizer.step()``.  The criterion sees the static slice ``[:B]`` of a
    fixed-count batch; ragged, or when it is ``capturable``, it reads the count of real graphs from ``valid`` on the device.  Three
    warm-up runs on a side stream precede the capture; parameters, buffers and optimizer state are put back afterwards, so
    constructing it does not train.  The modules' training flags are those of the caller outside ``run_once``.

    The learning rate: ``torch.optim.Adam(params, lr=torch.tensor(1e-3, device=dev), capturable=True, fused=True)`` keeps it in a device
    tensor that the graph reads on every replay, so filling it between replays (an LR scheduler does) changes the update.  A float
    ``lr`` is frozen into the graph at capture.

    ``ragged``, ``capacity``, ``batches``, ``check_epoch``, ``overflowed()``: as in ``ReplayedStep``.  An overflow batch of a ragged
    instance has no filled slot: its loss is exactly 0.

    ``log=True``: the body ends in ``log.append`` (a :class:`~dp_gsat_amd.eval_log.ClfLog`, ``max_graphs`` / ``max_batches`` default to
    the dataset's graph count and the most batches an epoch can have) of the step's logits and loss -- two more launches.
    ``begin_epoch()`` empties the log and ``epoch_scores()`` is ``log.compute()``: the training accuracy / ROC-AUC and mean loss of
    ``run_one_epoch(..., 'train')`` without a second pass.  Logging writes only the log: a run with ``log=True`` trains bit for bit
    like one without.

    After a step: ``loss`` (device scalar), ``clf_logits`` [B + 1, C] and ``batch`` (the PaddedBatch), overwritten by the next replay.

    Refused with ValueError before anything is captured: an optimizer that is not capturable, a multi-label criterion not constructed
    with ``capturable=True``, ``sync_group`` BatchNorm, a dataset without ``y_all``, a GSAT model, and a capacity the warm-up batch
    does not fit."""

    def __init__(self, model, criterion, optimizer, dataset, batch_size: int, capacity: Optional[tuple] = None, graph=None,
                 ragged: bool = False, log: bool = False, max_graphs: Optional[int] = None, max_batches: Optional[int] = None):
        _need_capturable(optimizer, "ReplayedClfStep needs a capturable optimizer")
        _clf_refusals("ReplayedClfStep", model, criterion, dataset)
        self.model, self.criterion, self.optimizer, self.dataset = model, criterion, optimizer, dataset
        self._setup(model, (dataset,), batch_size, capacity, graph, ragged)
        self._log_sizes = (max_graphs, max_batches) if log else None
        self.log = self.batch = self.loss = self.clf_logits = None
        _capture_training(self, (optimizer,))

    def run_once(self):
        """The step body (what the graph holds), run on the current stream."""
        clear_cache()
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        self._overflow.bitwise_or_(b.valid[3:4])
        with _module_modes(self.model, True):
            logits, loss = _clf_forward(self.model, self.criterion, b)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        if self._log_sizes is not None:
            with torch.no_grad():
                if self.log is None:            # the first warm-up run
                    self.log = _new_clf_log(self, logits, *self._log_sizes)
                self.log.append(b, logits.detach(), loss.detach())
        self._publish(False, batch=b, loss=loss.detach(), clf_logits=logits.detach())

    def overflowed(self) -> bool:
        """True if a step since the last call (or since capture) got a batch that did not fit the capacity.  One host read; clears
        the flag."""
        return _take_overflow(self)

    def begin_epoch(self) -> None:
        """Empty the training-pass log on the device; nothing is read.  Without ``log=True`` there is nothing to empty."""
        _reset_logs(self)

    def epoch_scores(self) -> dict:
        """``log.compute()`` -- two host reads -- over the steps since ``begin_epoch()``.  ValueError without ``log=True``, before any
        step, and when a step since ``begin_epoch()`` did not fit the capacity."""
        if self.log is None:
            raise ValueError("ReplayedClfStep was constructed without log=True: it keeps no log of the training pass")
        return self.log.compute()


class ReplayedClfEval(_ReplayedClf):
    """``ReplayedClfEval(model, criterion, dataset, batch_size, capacity=None, ragged=False, max_graphs=None, max_batches=None,
    graph=None)``: an evaluation epoch of a bare backbone (``eval_one_batch`` of src/pretrain_clf.py) as replays of ONE captured
    hipGraph that holds clear_cache, collate_padded, the eval-mode forward and the criterion under ``torch.no_grad()``, and
    ``log.append`` into a :class:`~dp_gsat_amd.eval_log.ClfLog` (``log``).  The graph reads parameters and running statistics where
    they live, writes none of them and draws from no generator: evaluating between training steps does not change the training run.
    After a step: ``clf_logits``, ``loss`` and ``batch``.  Refusals: those of ``ReplayedClfStep`` that do not concern an optimizer."""

    def __init__(self, model, criterion, dataset, batch_size: int, capacity: Optional[tuple] = None, ragged: bool = False,
                 max_graphs: Optional[int] = None, max_batches: Optional[int] = None, graph=None):
        _clf_refusals("ReplayedClfEval", model, criterion, dataset)
        self.model, self.criterion, self.dataset = model, criterion, dataset
        self._setup(model, (dataset,), batch_size, capacity, graph, ragged)
        self.log = self.batch = self.loss = self.clf_logits = None
        _capture_evaluator(self, lambda: self._make_log(max_graphs, max_batches))

    def _make_log(self, max_graphs, max_batches):
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        with torch.no_grad():
            logits = _clf_forward(self.model, self.criterion, b)[0]
        self.log = _new_clf_log(self, logits, max_graphs, max_batches)

    def _forward(self, b, epoch=0):
        """Append the eval-mode forward of batch ``b`` (padded or not) to the log; the modules are in eval mode."""
        with torch.no_grad():
            logits, loss = _clf_forward(self.model, self.criterion, b)
            self.log.append(b, logits, loss)
        return logits, loss

    def run_once(self):
        """The body of the captured graph, run on the current stream."""
        clear_cache()
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        with _module_modes(self.model, False):
            logits, loss = self._forward(b)
        self._publish(False, clf_logits=logits, loss=loss, batch=b)

    def run(self, graph_ids, epoch: int = 0) -> dict:
        """One evaluation epoch over ``graph_ids`` (any number, in visiting order): the log is reset, every full batch is a replay, the
        tail of fewer than ``batch_size`` graphs runs eagerly (``dataset.collate``, the same eval-mode forward, the same append), and
        ``log.compute()`` -- two host reads -- gives the scores.  Ragged: the ids are packed by ``batches`` and every batch is a
        replay."""
        return _run_epoch(self, graph_ids, 0)


# ---- explanation fidelity ---------------------------------------------------------------------------------------------------------------------
def keep_capacity(E_cap: int, batch_size: int, k: Optional[int] = None, ratio: Optional[float] = None) -> int:
    """The edge capacity of the explanation side of a fidelity batch, derived and not tuned: ``k * batch_size`` for a top-k of ``k`` edges
    per graph; ``min(E_cap, ceil(ratio * E_cap) + batch_size)`` for a ratio, because ``sum_g ceil(ratio * E_g) <= ratio * sum_g E_g +
    batch_size``.  A batch that fits ``E_cap`` can therefore never overflow the explanation side."""
    if (k is None) == (ratio is None):
        raise ValueError("give exactly one of k and ratio")
    if k is not None:
        return int(k) * int(batch_size)
    return min(int(E_cap), int(math.ceil(float(ratio) * int(E_cap))) + int(batch_size))


class ReplayedFidelity(_Replayed):
    """``ReplayedFidelity(gsat, dataset, batch_size, k=None, ratio=None, capacity=None, max_graphs=None, graph=None, ragged=False)``: the
    fidelity of the top-k (or top-ratio) explanation over ``dataset`` -- the one explanation score that needs no edge labels -- as replays of
    ONE captured hipGraph.  A replay holds clear_cache; ``collate_padded``; the eval-mode attention on the edges, ``gsat.forward_pass(b, 0,
    False)[0]``, under ``torch.no_grad()`` with every module in ``eval()`` mode; ``topk_edge_mask`` on the fused one-launch path over the
    ``batch_size`` real graphs with the dataset's largest edge count as its bound; two padded extractions -- ``keep =
    edge_subgraph_padded(b, mask, (N_cap, E_keep_cap))`` and ``drop = edge_subgraph_padded(b, ~mask, (N_cap, E_cap))`` --; three
    ``gsat.clf`` forwards WITHOUT ``edge_atten``, each inside ``padded(valid, capacity)`` of its own batch; and ``log.append`` into a
    :class:`~dp_gsat_amd.eval_log.FidelityLog` (``log``).  Nothing is read back per batch.

    ``E_keep_cap`` is ``keep_capacity(E_cap, batch_size, k, ratio)``: derived, so that a batch that fits ``capacity`` never overflows the
    explanation side, and tight, so that the padding graph of the explanation batch stays small.

    ``run(graph_ids)`` resets the log, replays every full batch -- ragged: every row of ``batches``, no eager batch --, runs a fixed-count
    tail eagerly through the same code on ``dataset.collate`` output, and returns ``log.compute()``: ``fidelity_plus``, ``fidelity_minus``,
    ``p_full``, ``p_keep``, ``p_drop``, ``flip_plus``, ``flip_minus``, ``n``.

    After a step: ``edge_att`` [E_cap, 1], ``topk`` bool[E_cap] (arbitrary at the padding slots), ``keep_batch``, ``drop_batch``,
    ``logits_full`` / ``logits_keep`` / ``logits_drop`` [B + 1, C] and ``batch``.  ``overflowed()`` tells (one host read) whether a batch or
    an extraction since the last call did not fit; ``check_epoch`` tells beforehand.

    The graph writes no parameter, buffer or optimizer state and draws from neither the device seed stream nor torch's generators: a
    fidelity epoch between ``ReplayedStep`` steps leaves the training run bitwise unchanged.

    Refused with ValueError before anything is captured: both or neither of ``k`` and ``ratio``; a dataset without graph labels (edge
    labels are NOT needed); ``DualGSAT``; ``sync_group`` BatchNorm; the multi-label criterion, capturable or not; a dataset whose largest
    graph has more edges than ``rank_edges_lds_cap()`` (the radix ranking is not captured); a capacity the first batch does not fit.

    This single-level class keeps no task axis.  A single level of a multi-task model is ``ReplayedFidelityCurve(..., ks=(k,))`` or
    ``ReplayedFidelityCurve(..., ratios=(r,))``, whose log has one."""

    def __init__(self, gsat, dataset, batch_size: int, k: Optional[int] = None, ratio: Optional[float] = None,
                 capacity: Optional[tuple] = None, max_graphs: Optional[int] = None, graph=None, ragged: bool = False):
        if (k is None) == (ratio is None):
            raise ValueError("give exactly one of k and ratio")
        if k is not None and (isinstance(k, bool) or int(k) != k or int(k) < 1):
            raise ValueError("k must be a positive int")
        if ratio is not None and not 0.0 < float(ratio) <= 1.0:
            raise ValueError("ratio must lie in (0, 1]")
        if hasattr(gsat, "dual_forward_pass") or not hasattr(gsat, "forward_pass"):
            raise ValueError("ReplayedFidelity replays GSAT.forward_pass and its backbone; DualGSAT fidelity is not covered")
        if _multi_label(gsat.criterion):
            raise ValueError(_MULTI_LABEL_SINGLE)
        _refuse_sync_group(gsat)
        if dataset.y_all is None:
            raise ValueError("ReplayedFidelity needs a dataset with graph labels (the eval-mode forward takes them); edge labels are not needed")
        self.max_seg_edges = int(dataset.edge_counts.max()) if dataset.num_graphs else 0          # one host read, here
        if self.max_seg_edges > _explain.rank_edges_lds_cap():
            raise ValueError(f"the dataset's largest graph has {self.max_seg_edges} edges, above rank_edges_lds_cap() = "
                             f"{_explain.rank_edges_lds_cap()}: the captured top-k takes the fused ranking only")
        self.gsat, self.dataset = gsat, dataset
        self.k, self.ratio = (None if k is None else int(k)), (None if ratio is None else float(ratio))
        self._setup(gsat, (dataset,), batch_size, capacity, graph, ragged)
        N_cap, E_cap = self.capacity
        self.keep_capacity = (N_cap, keep_capacity(E_cap, self.batch_size, self.k, self.ratio))
        self._max_graphs = dataset.num_graphs if max_graphs is None else int(max_graphs)
        self._overflow = torch.zeros(1, dtype=torch.int32, device=dataset.x_all.device)
        self.log = self.batch = self.edge_att = self.topk = self.keep_batch = self.drop_batch = None
        self.logits_full = self.logits_keep = self.logits_drop = None
        try:
            _capture_evaluator(self, self._make_log)
        finally:
            self._overflow.zero_()

    def _make_log(self):
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        with torch.no_grad(), padded(b.valid, b.capacity):
            get_index(b.edge_index, int(b.x.shape[0])).graphs(b.batch, int(b.num_graphs))
            logits = self.gsat.clf(b.x, b.edge_index, b.batch, getattr(b, "edge_attr", None))
        self.log = FidelityLog(self._max_graphs, int(logits.shape[1]), self.dataset.x_all.device)

    def _forward(self, b, epoch=0):
        """Attention, top-k, the two extractions, the three backbone forwards and the append for batch ``b`` -- a ``PaddedBatch`` (the
        captured body) or ``collate`` output (the eager tail); the modules are in eval mode."""
        clf = self.gsat.clf
        with torch.no_grad():
            att = edge_tensor(self.gsat.forward_pass(b, epoch, False)[0]).detach()
            valid = getattr(b, "valid", None)
            real = int(b.num_graphs) - (1 if valid is not None else 0)
            mask = _explain.topk_edge_mask(att, b.edge_index, b.batch, k=self.k, ratio=self.ratio, num_graphs=int(b.num_graphs),
                                           max_seg_edges=self.max_seg_edges, ranked_graphs=real)
            keep = edge_subgraph_padded(b, mask, self.keep_capacity)
            drop = edge_subgraph_padded(b, ~mask, self.capacity)
            logits = []
            for d in (b, keep, drop):
                get_index(d.edge_index, int(d.x.shape[0])).graphs(d.batch, int(d.num_graphs))
                if getattr(d, "valid", None) is None:
                    logits.append(clf(d.x, d.edge_index, d.batch, getattr(d, "edge_attr", None)))
                else:
                    with padded(d.valid, d.capacity):
                        logits.append(clf(d.x, d.edge_index, d.batch, getattr(d, "edge_attr", None)))
            over = keep.valid[3:4] | drop.valid[3:4]
            self._overflow.bitwise_or_(over if valid is None else over | valid[3:4])
            if valid is None:       # the eager tail: its extractions have raised if they did not fit; the padding graph's row is cut off
                logits = [z[:real] for z in logits]
            self.log.append(*logits, valid)
        return att, mask, keep, drop, logits

    def run_once(self):
        """The body of the captured graph, run on the current stream."""
        clear_cache()
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        b.r = self.r
        att, mask, keep, drop, logits = self._forward(b, 0)
        self._publish(False, batch=b, edge_att=att, topk=mask, keep_batch=keep, drop_batch=drop, logits_full=logits[0],
                      logits_keep=logits[1], logits_drop=logits[2])

    def run(self, graph_ids, epoch: int = 0) -> dict:
        """One fidelity epoch over ``graph_ids`` (any number, in visiting order): the log is reset, every full batch is a replay, a
        fixed-count tail of fewer than ``batch_size`` graphs runs eagerly through the same code (``dataset.collate``, then the padded
        extractions at the captured capacities), and ``log.compute()`` -- one reduction launch, one host read -- gives the scores.
        Ragged: the ids are packed by ``batches`` and every batch is a replay."""
        return _run_epoch(self, graph_ids, epoch)

    def overflowed(self) -> bool:
        """True if a batch or an extraction since the last call (or since capture) did not fit its capacity.  One host read; clears the
        flag."""
        return _take_overflow(self)


class ReplayedFidelityCurve(_Replayed):
    """``ReplayedFidelityCurve(gsat, dataset, batch_size, ks=None, ratios=None, capacity=None, max_graphs=None, graph=None,
    ragged=False)``: the fidelity of the explanation at ``S`` sparsity levels at once -- a curve over ``ks`` (top-k per graph) or ``ratios``
    (top-ratio), 1 to 16 strictly increasing values -- as replays of ONE captured hipGraph.  Where ``S`` ``ReplayedFidelity`` instances
    repeat the collation, the attention, the ranking and the full-graph forward and run ``2 S`` extractions and backbone forwards, a replay
    here holds clear_cache; ``collate_padded``; the eval-mode attention ``gsat.forward_pass(b, 0, False)[0]`` under ``torch.no_grad()``
    with every module in ``eval()`` mode; ``explanation_levels`` -- ONE fused ranking over the ``batch_size`` real graphs --;
    ``explanation_stack``: the ``2 S + 1`` variants of the batch side by side, in a launch count that does not depend on ``S``; ONE
    ``gsat.clf`` forward WITHOUT ``edge_atten`` on the stack, outside ``padded()`` (eval-mode BatchNorm takes no batch statistics, and the
    padding rows of every variant sit in that variant's padding graph); and ``log.append`` into a
    :class:`~dp_gsat_amd.eval_log.FidelityCurveLog` (``log``).  Nothing is read back per batch.

    ``run(graph_ids)`` resets the log, replays every full batch -- ragged: every row of ``batches``, no eager batch --, runs a fixed-count
    tail eagerly through the same code on ``dataset.collate`` output, and returns ``log.compute()``: ``levels``, ``fidelity_plus``,
    ``fidelity_minus``, ``p_keep``, ``p_drop``, ``flip_plus``, ``flip_minus``, ``kept_fraction`` (lists over the levels), ``p_full``, ``n``.

    After a step: ``edge_att`` [E_cap, 1], ``edge_level`` uint8[E_cap] (arbitrary at the padding slots), ``stack`` (the
    ``StackedExplanationBatch``), ``logits`` [(2 S + 1) * (B + 1), C] and ``batch``.  ``overflowed()`` tells (one host read) whether a batch
    or a variant since the last call did not fit; ``check_epoch`` tells beforehand.

    The graph writes no parameter, buffer or optimizer state and draws from neither the device seed stream nor torch's generators: a curve
    epoch between ``ReplayedStep`` steps leaves the training run bitwise unchanged.

    Refused with ValueError before anything is captured: what ``ReplayedFidelity`` refuses -- a dataset without graph labels, ``DualGSAT``,
    ``sync_group`` BatchNorm, a dataset whose largest graph has more edges than ``rank_edges_lds_cap()``, a capacity the first batch does
    not fit --, a multi-label criterion that was not constructed with ``capturable=True``, and bad levels: neither or both of ``ks`` and
    ``ratios``, values that are not strictly increasing, more than 16.

    Multi-task models (``Criterion(T, True, capturable=True)``): the log is a ``FidelityCurveLog(..., tasks=T)`` -- every (graph, task) is
    a binary decision of its own -- and ``run`` adds ``fidelity_plus_tasks``, ``fidelity_minus_tasks``, ``p_keep_tasks``, ``p_drop_tasks``,
    ``flip_plus_tasks``, ``flip_minus_tasks`` (``[S][T]``) and ``p_full_tasks`` (``[T]``); the per-level keys are the means over the tasks.

    ``unit="edge"`` (the default) is all of the above.  ``unit="node"`` is the curve over NODES for a node-attention model
    (``learn_edge_att=False``): a replay ranks ``forward_pass(...)[0].node_att`` inside every graph (``node_levels``, the fused ranking with
    the dataset's largest node count as its bound), stacks the ``2 S + 1`` node-induced variants with ``explanation_stack_nodes`` -- a
    variant deletes node rows, relabels its endpoints and keeps an edge only when both ends survive --, runs the one ``clf`` forward and
    appends to the same ``FidelityCurveLog`` (multi-task ``tasks=T`` included).  It publishes ``node_att`` [N_cap, 1], ``node_level``
    uint8[N_cap], ``stack``, ``logits`` and ``batch``.  ``run`` adds ``kept_node_fraction``, per level the kept nodes over the nodes of the
    graphs ``graph_ids``: computed on the host from the dataset's node counts and the level rule (``min(k, N_g)``, or the same fp64
    ``ceil(N_g * ratio)``), exact, with no device read per batch; ``kept_fraction`` stays the fraction of edges.  Refused besides the above:
    a model that learns edge attention, and a dataset whose largest graph has more NODES than ``rank_edges_lds_cap()`` (its edge counts
    are not ranked and not bounded).

    ``connectivity=True`` (``unit="edge"`` only; with ``unit="node"`` a ValueError before capture): the captured body ends in ONE
    ``level_components`` launch on the real batch -- ``stack.edge_level``, the batch's ``valid``, ``ranked_graphs = num_graphs - 1`` and the
    dataset's largest node count as ``max_seg_nodes`` (one host read of ``dataset.node_counts`` at construction; above
    ``components_lds_cap()`` a ValueError there) -- into ``components`` int64[S, 8], which ``run`` resets next to the log and reads once
    more at the end: it adds ``components``, ``largest_edge_share``, ``largest_node_share`` and ``connected_fraction`` (lists over the
    levels, ``connectivity_scores``).  Every other returned value is bitwise what it is without the keyword."""

    def __init__(self, gsat, dataset, batch_size: int, ks=None, ratios=None, capacity: Optional[tuple] = None,
                 max_graphs: Optional[int] = None, graph=None, ragged: bool = False, unit: str = "edge", connectivity: bool = False):
        self.ks, self.ratios = _explain.check_levels(ks, ratios)
        if unit not in ("edge", "node"):
            raise ValueError("unit must be 'edge' or 'node'")
        if connectivity and unit != "edge":
            raise ValueError("connectivity=True scores the kept EDGES of an edge ranking: it goes with unit='edge' only (node-induced "
                             "variants are a different question)")
        self.unit, self.connectivity, self.components = unit, bool(connectivity), None
        if hasattr(gsat, "dual_forward_pass") or not hasattr(gsat, "forward_pass"):
            raise ValueError("ReplayedFidelityCurve replays GSAT.forward_pass and its backbone; DualGSAT fidelity is not covered")
        if unit == "node" and gsat.learn_edge_att:
            raise ValueError("ReplayedFidelityCurve(unit='node') ranks the node attention of a node-attention model (learn_edge_att=False); "
                             "this model learns edge attention: use unit='edge'")
        _refuse_uncapturable(gsat.criterion)
        _refuse_sync_group(gsat)
        if dataset.y_all is None:
            raise ValueError("ReplayedFidelityCurve needs a dataset with graph labels (the eval-mode forward takes them); edge labels are "
                             "not needed")
        if unit == "node":
            self._host_nodes = dataset.node_counts.cpu().numpy().astype("int64")                   # one host read, here
            self.max_seg_nodes = int(self._host_nodes.max()) if dataset.num_graphs else 0
            if self.max_seg_nodes > _explain.rank_edges_lds_cap():
                raise ValueError(f"the dataset's largest graph has {self.max_seg_nodes} nodes, above rank_edges_lds_cap() = "
                                 f"{_explain.rank_edges_lds_cap()}: the captured ranking takes the fused path only")
        else:
            self.max_seg_edges = int(dataset.edge_counts.max()) if dataset.num_graphs else 0      # one host read, here
            if self.max_seg_edges > _explain.rank_edges_lds_cap():
                raise ValueError(f"the dataset's largest graph has {self.max_seg_edges} edges, above rank_edges_lds_cap() = "
                                 f"{_explain.rank_edges_lds_cap()}: the captured ranking takes the fused path only")
        if self.connectivity:
            self._cc_nodes = _max_seg_nodes(dataset, "the dataset")                                # one host read, here
            S = len(self.ks if self.ks is not None else self.ratios)
            self.components = torch.zeros((S, 8), dtype=torch.int64, device=dataset.x_all.device)
        self.gsat, self.dataset = gsat, dataset
        self._setup(gsat, (dataset,), batch_size, capacity, graph, ragged)
        self._max_graphs = dataset.num_graphs if max_graphs is None else int(max_graphs)
        self._overflow = torch.zeros(1, dtype=torch.int32, device=dataset.x_all.device)
        self.log = self.batch = self.edge_att = self.edge_level = self.node_att = self.node_level = self.stack = self.logits = None
        try:
            _capture_evaluator(self, self._make_log)
        finally:
            self._overflow.zero_()

    def _make_log(self):
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        with torch.no_grad(), padded(b.valid, b.capacity):
            get_index(b.edge_index, int(b.x.shape[0])).graphs(b.batch, int(b.num_graphs))
            logits = self.gsat.clf(b.x, b.edge_index, b.batch, getattr(b, "edge_attr", None))
        tasks = int(logits.shape[1]) if _multi_label(self.gsat.criterion) else None
        self.log = FidelityCurveLog(self._max_graphs, int(logits.shape[1]), self.ks, self.ratios, self.dataset.x_all.device, tasks=tasks)

    def _forward(self, b, epoch=0):
        """Attention, levels, the stack, the one backbone forward and the append for batch ``b`` -- a ``PaddedBatch`` (the captured body)
        or ``collate`` output (the eager tail, stacked at the captured batch size); the modules are in eval mode."""
        with torch.no_grad():
            att = self.gsat.forward_pass(b, epoch, False)[0]
            valid = getattr(b, "valid", None)
            if self.unit == "node":
                att = att.node_att.detach()
                stack = explanation_stack_nodes(b, att, ks=self.ks, ratios=self.ratios, batch_size=self.batch_size,
                                                max_seg_nodes=self.max_seg_nodes)
            else:
                att = edge_tensor(att).detach()
                stack = explanation_stack(b, att, ks=self.ks, ratios=self.ratios, batch_size=self.batch_size, max_seg_edges=self.max_seg_edges)
            logits = self.gsat.clf(stack.x, stack.edge_index, stack.batch, stack.edge_attr)
            over = stack.valid[:, 3].amax().view(1)
            self._overflow.bitwise_or_(over if valid is None else over | valid[3:4])
            self.log.append(logits, stack.valid, valid)
            if self.connectivity:
                _components(b, stack.edge_level, self.components.shape[0], self._cc_nodes, self.components)
        return att, stack, logits

    def run_once(self):
        """The body of the captured graph, run on the current stream."""
        clear_cache()
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        b.r = self.r
        att, stack, logits = self._forward(b, 0)
        if self.unit == "node":
            self._publish(False, batch=b, node_att=att, node_level=stack.node_level, stack=stack, logits=logits)
        else:
            self._publish(False, batch=b, edge_att=att, edge_level=stack.edge_level, stack=stack, logits=logits)

    def run(self, graph_ids, epoch: int = 0) -> dict:
        """One curve epoch over ``graph_ids`` (any number, in visiting order): the log is reset, every full batch is a replay, a
        fixed-count tail of fewer than ``batch_size`` graphs runs eagerly through the same code, and ``log.compute()`` -- one reduction
        launch, one host read -- gives the scores.  Ragged: the ids are packed by ``batches`` and every batch is a replay.
        ``unit="node"`` adds ``kept_node_fraction`` (see the class)."""
        res = _run_epoch(self, graph_ids, epoch)
        if self.unit == "node":
            res["kept_node_fraction"] = self._kept_node_fraction(graph_ids)
        if self.connectivity:
            scores = _explain.connectivity_scores(self.components.tolist())                       # the read of the components block
            res.update({key: scores[key] for key in _explain.CONNECTIVITY_KEYS})
        return res

    def _kept_node_fraction(self, graph_ids) -> list:
        """Per level, kept nodes / nodes over the graphs ``graph_ids``, on the host: the level rule of ``node_levels`` -- ``min(k, N_g)`` or
        the fp64 ``ceil(N_g * ratio)`` -- on the dataset's node counts, in integers."""
        import numpy as np
        n = self._host_nodes[torch.as_tensor(graph_ids).reshape(-1).cpu().numpy().astype(np.int64)]
        total = int(n.sum())
        if self.ks is not None:
            kept = [int(np.minimum(n, k).sum()) for k in self.ks]
        else:
            kept = [int(np.ceil(n.astype(np.float64) * r).astype(np.int64).sum()) for r in self.ratios]
        return [k / total if total else 0.0 for k in kept]

    def overflowed(self) -> bool:
        """True if a batch or a variant of its stack since the last call (or since capture) did not fit its capacity.  One host read;
        clears the flag."""
        return _take_overflow(self)


class ReplayedDualFidelityCurve(_Replayed):
    """``ReplayedDualFidelityCurve(dual_gsat, primal_ds, dual_ds, batch_size, ks=None, ratios=None, capacity=None, max_graphs=None,
    seed=None, graphs=None, ragged=False)``: the fidelity curves of the TWO explanations a dual/primal model gives of the same primal edges
    -- ranking 0: the primal edge attention, mixed with the dual one once ``epoch > mix_after_epoch``; ranking 1: the dual node attention
    read on the primal edge slots (dual node row k is primal edge slot k) -- with their agreement, over ``S`` levels (``ks`` or
    ``ratios``, ``2 S`` at most 16), as replays of captured hipGraphs.  Which of the two the classifier relies on, without edge labels.

    One replay holds clear_cache; ``collate_padded_pair``; one gsat_seed_next from a private ``seed_state`` (the rules of
    ``ReplayedDualEval``: ``run`` restarts it at ``(base, epoch << 32)``); ``dual_forward_pass(pb, db, epoch, False, dual_seed=word)``
    under ``torch.no_grad()`` with every module in ``eval()`` mode; the fused ranking and gsat_fidelity_levels of both attentions on
    the primal batch; ONE ``explanation_stack_multi`` -- the ``1 + 4 S`` variants around one copy of the batch --; ONE ``primal_clf``
    forward WITHOUT ``edge_atten`` on the stack, as in ``ReplayedFidelityCurve``; ``log.append`` into a ``FidelityCurveLog(...,
    rankings=2)``; and ``level_overlap`` of the two level rows into ``overlap`` int64[S, 3].  The mix is a host branch: TWO graphs
    (unmixed, mixed), picked by ``epoch > mix_after_epoch``.  Nothing is read back per batch.

    ``run(graph_ids, epoch)`` resets the log and the overlap block, replays every full batch -- ragged: every row of ``batches``, no eager
    batch --, runs a fixed-count tail eagerly through the same code, and returns ``primal`` and ``dual`` (each the dict of
    ``ReplayedFidelityCurve.run``), ``jaccard`` and ``overlap`` (lists over the levels: ``both / (a + b - both)`` and ``both / min(a,
    b)`` of the kept edge sets, 0.0 where the denominator is 0), ``p_full`` and ``n``: one reduction launch and one host read, plus one
    read of the overlap block.

    After a step: ``edge_att`` and ``dual_att`` [E_cap, 1], ``edge_level`` uint8[2, E_cap], ``stack``, ``logits``, ``batch`` and
    ``dual_batch``.  ``overflowed()`` / ``check_epoch`` as elsewhere.

    The graphs write no parameter, buffer or optimizer state and draw from neither the device seed stream nor torch's generators: a curve
    epoch between ``ReplayedDualStep`` steps leaves the training run bitwise unchanged.

    Refused with ValueError before anything is captured: bad levels or ``2 * S > 16``; what a padded pair refuses (edge attention, the
    multi-label criterion, ``check_pair``, a capacity that is no triple); ``sync_group`` BatchNorm; a model without ``dual_forward_pass``;
    a primal dataset without graph labels or without ``edge_label`` (the f1 term of ``dual_forward_pass`` needs it); a largest primal
    graph above ``rank_edges_lds_cap()``.

    ``connectivity=True``: two more launches per replay, ``level_components`` of each row of ``stack.edge_level`` on the primal batch, into
    ``components`` int64[2, S, 8] (reset with the overlap block, read once more by ``run``); the ``primal`` and ``dual`` dicts gain
    ``components``, ``largest_edge_share``, ``largest_node_share`` and ``connected_fraction`` -- which of the two explanations is the more
    connected one.  Refused when the primal dataset's largest graph has more nodes than ``components_lds_cap()``.  Every other returned
    value is bitwise what it is without the keyword."""

    def __init__(self, dual_gsat, primal_ds, dual_ds, batch_size: int, ks=None, ratios=None, capacity: Optional[tuple] = None,
                 max_graphs: Optional[int] = None, seed: Optional[int] = None, graphs=None, ragged: bool = False,
                 connectivity: bool = False):
        self.ks, self.ratios = _explain.check_levels(ks, ratios)
        self.levels = tuple(self.ks if self.ks is not None else self.ratios)
        _explain.check_rankings(2, len(self.levels))
        self.connectivity, self.components = bool(connectivity), None
        m = dual_gsat
        if not hasattr(m, "dual_forward_pass"):
            raise ValueError("ReplayedDualFidelityCurve replays DualGSAT.dual_forward_pass; ReplayedFidelityCurve covers a plain GSAT")
        _refuse_sync_group(m)
        if primal_ds.y_all is None or dual_ds.y_all is None or primal_ds.edge_label_all is None:
            raise ValueError("ReplayedDualFidelityCurve needs datasets with graph labels and a primal dataset with edge_label (the f1 "
                             "term of dual_forward_pass takes it)")
        self.max_seg_edges = int(primal_ds.edge_counts.max()) if primal_ds.num_graphs else 0          # one host read, here
        if self.max_seg_edges > _explain.rank_edges_lds_cap():
            raise ValueError(f"the primal dataset's largest graph has {self.max_seg_edges} edges, above rank_edges_lds_cap() = "
                             f"{_explain.rank_edges_lds_cap()}: the captured ranking takes the fused path only")
        _padded_pair_setup(self, m, primal_ds, dual_ds, batch_size, capacity, graphs, ragged)
        dev = primal_ds.x_all.device
        if seed is None:        # the mix of ReplayedDualEval: follows torch.manual_seed, draws nothing
            seed = (torch.initial_seed() * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & 0x7FFFFFFFFFFFFFFF
        self.base = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.seed_state = torch.empty(2, dtype=torch.int64, device=dev)
        _EVAL_SEED_STATES.append(self.seed_state)
        self._set_seed_state(0)
        self._max_graphs = primal_ds.num_graphs if max_graphs is None else int(max_graphs)
        self._overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        self.overlap = torch.zeros((len(self.levels), 3), dtype=torch.int64, device=dev)
        if self.connectivity:
            self._cc_nodes = _max_seg_nodes(primal_ds, "the primal dataset")                       # one host read, here
            self.components = torch.zeros((2, len(self.levels), 8), dtype=torch.int64, device=dev)
        self.log = self.batch = self.dual_batch = self.edge_att = self.dual_att = self.edge_level = self.stack = self.logits = None
        try:
            with _capture_mode(m, evaluating=True):
                self._warm_up_and_capture(self._make_log, self._reset)
        finally:
            self._reset()
            self._set_seed_state(0)
            self._overflow.zero_()

    _set_seed_state = ReplayedDualEval._set_seed_state

    def _reset(self):
        if self.log is not None:
            self.log.reset()
        _explain.level_overlap_reset(self.overlap)
        if self.components is not None:
            for block in self.components:
                _explain.level_components_reset(block)

    def _make_log(self):
        pb, _ = collate_padded_pair(self.primal_ds, self.dual_ds, self.graph_ids, self.capacity, ragged=self.ragged)
        with torch.no_grad(), padded(pb.valid, pb.capacity):
            get_index(pb.edge_index, int(pb.x.shape[0])).graphs(pb.batch, int(pb.num_graphs))
            logits = self.model.primal_clf(pb.x, pb.edge_index, pb.batch, getattr(pb, "edge_attr", None))
        self.log = FidelityCurveLog(self._max_graphs, int(logits.shape[1]), self.ks, self.ratios, self.primal_ds.x_all.device, rankings=2)

    def _forward(self, pb, db, epoch):
        """The pair's eval-mode forward with the stream's next seed word, both rankings, the stack, the one backbone forward, the append
        and the overlap for the pair ``pb, db`` -- padded (the captured body) or ``collate`` output (the eager tail, stacked at the captured
        batch size); the modules are in eval mode and sync_loss_dict is off."""
        m = self.model
        word = None
        if m.gumbel_noise_in_eval:
            word = torch.empty(1, dtype=torch.int64, device=self.seed_state.device)
            call("gsat_seed_next", ptr(self.seed_state), ptr(word), stream())
        kept = m.keep_dual_att
        m.keep_dual_att = True
        try:
            with torch.no_grad():
                att = edge_tensor(m.dual_forward_pass(pb, db, epoch, False, dual_seed=word)[0]).detach()
                dual_att = m.dual_att[:att.shape[0]]
                stack, logits = self._score(pb, att, dual_att)
        finally:
            m.keep_dual_att, m.dual_att = kept, None
        return att, dual_att, stack, logits, word

    def _score(self, pb, att, dual_att):
        """Both rankings of the primal batch ``pb`` in one stack, the one backbone forward, the append and the overlap."""
        valid = getattr(pb, "valid", None)
        stack = explanation_stack_multi(pb, [att, dual_att], ks=self.ks, ratios=self.ratios, batch_size=self.batch_size,
                                        max_seg_edges=self.max_seg_edges)
        logits = self.model.primal_clf(stack.x, stack.edge_index, stack.batch, stack.edge_attr)
        over = stack.valid[:, 3].amax().view(1)
        self._overflow.bitwise_or_(over if valid is None else over | valid[3:4])
        self.log.append(logits, stack.valid, valid)
        _explain.level_overlap(stack.edge_level[0], stack.edge_level[1], len(self.levels), valid=valid, out=self.overlap)
        if self.connectivity:
            for r in range(2):
                _components(pb, stack.edge_level[r], len(self.levels), self._cc_nodes, self.components[r])
        return stack, logits

    def run_once(self, mixed: bool):
        """The body of one captured graph, run on the current stream."""
        clear_cache()
        pb, db = collate_padded_pair(self.primal_ds, self.dual_ds, self.graph_ids, self.capacity, ragged=self.ragged)
        db.r = self.r
        att, dual_att, stack, logits, word = self._forward(pb, db, _mix_epoch(self.model, mixed))
        self._publish(mixed, batch=pb, dual_batch=db, edge_att=att, dual_att=dual_att, edge_level=stack.edge_level, stack=stack,
                      logits=logits, _word=word)

    def run(self, graph_ids, epoch: int) -> dict:
        """One curve epoch over ``graph_ids`` (any number, in visiting order) at ``epoch``: the seed stream restarts at (base, epoch << 32),
        the log and the overlap block are reset, every full batch is a replay of the graph ``epoch > mix_after_epoch`` picks, a tail of
        fewer than ``batch_size`` graphs runs eagerly through the same code on both datasets' ``collate``, and ``log.compute()`` -- one
        reduction launch, one host read -- plus one read of ``overlap`` give the result.  Ragged: the ids are packed by ``batches`` and
        every batch is a replay."""
        self._set_seed_state(int(epoch) << 32)
        ids = torch.as_tensor(graph_ids).reshape(-1)
        B, n = self.batch_size, int(ids.numel())
        self._reset()
        rows, left = (self.batches(ids), 0) if self.ragged else ([ids[s:s + B] for s in range(0, n - B + 1, B)], n % B)
        for row in rows:
            self.step(row, epoch)
        if left:
            with _forward_mode(self.model, True):
                tail = ids[n - left:].to(self.graph_ids.device, torch.int64)
                self._forward(*[ds.collate(tail) for ds in self._datasets], epoch)
        res = self.log.compute()
        counts = self.overlap.tolist()                                                          # the read of the overlap block
        per_level = ("fidelity_plus", "fidelity_minus", "p_keep", "p_drop", "flip_plus", "flip_minus", "kept_fraction")
        out = {name: dict({key: res[key][r] for key in per_level}, levels=res["levels"], p_full=res["p_full"], n=res["n"])
               for r, name in enumerate(("primal", "dual"))}
        out["jaccard"] = [c[0] / (c[1] + c[2] - c[0]) if c[1] + c[2] - c[0] else 0.0 for c in counts]
        out["overlap"] = [c[0] / min(c[1], c[2]) if min(c[1], c[2]) else 0.0 for c in counts]
        out["p_full"], out["n"] = res["p_full"], res["n"]
        if self.connectivity:
            for name, counts in zip(("primal", "dual"), self.components.tolist()):                 # the read of the components block
                scores = _explain.connectivity_scores(counts)
                out[name].update({key: scores[key] for key in _explain.CONNECTIVITY_KEYS})
        return out

    def overflowed(self) -> bool:
        """True if a batch or a variant of its stack since the last call (or since capture) did not fit its capacity.  One host read;
        clears the flag."""
        return _take_overflow(self)


# ---- a post-hoc baseline: the batched GNNExplainer ------------------------------------------------------------------------------------------
class ReplayedGNNExplainer(_ReplayedClf):
    """``ReplayedGNNExplainer(clf, criterion, dataset, batch_size, k, steps=100, lr=0.01, betas=(0.9, 0.999), eps=1e-8, size_coef=0.005,
    ent_coef=1.0, symmetric=True, target="model", capacity=None, ragged=False, bins=64, max_graphs=None, max_edges=None, graphs=None)``: an
    explanation epoch of :class:`~dp_gsat_amd.baselines.GNNExplainer` on the bare backbone ``clf`` over ``dataset`` (a PackedDataset
    with ``edge_label_all``), scored like GSAT's attention.  It holds THREE captured hipGraphs (``graphs``):

      begin   clear_cache, ``collate_padded``, the unmasked eval-mode forward, the targets, ``gsat_mask_init``
      step    the masked forward, the criterion, the backward to the mask, ``gsat_mask_step``
      end     one masked forward under ``no_grad`` for the objective of the final mask, then ``log.append`` (an
              :class:`~dp_gsat_amd.eval_log.EpochLog`) of the symmetrised mask, the unmasked logits and the triple (objective, its
              prediction term, its regulariser)

    and ``step(ids)`` replays begin, ``steps`` times step, then end: the step counter of the mask's Adam lives on the device, so ONE
    captured step serves every iteration.  The step and end graphs read the batch, its index and the mask state at the addresses the
    begin graph writes them to.  ``run(ids)`` resets the log, replays every full batch (ragged: every row of ``batches``), runs a
    fixed-count tail eagerly through the same three phases and returns ``log.compute()`` -- the keys of ``ReplayedEval.run``, with
    ``loss`` / ``pred`` / ``info`` the means over the batches of the triple above.

    The graphs read the parameters and running statistics where they live and write none of them; no noise is drawn and the device seed
    stream is left alone, so an explanation epoch between training steps does not change the training run.  Parameters are frozen
    (``requires_grad``) while the graphs are captured and while a tail runs, and every flag is put back.

    After ``step`` / ``run``: ``batch``, ``edge_att`` [E_cap, 1], ``mask_logits`` [E_cap], ``clf_logits`` [B + 1, C] and ``losses`` [3] of
    the last replayed batch, for ``explanation_fidelity_curve`` or ``explanation_connectivity``.  A replay rewrites ``batch`` in place,
    which the index cache cannot see: call ``clear_cache()`` before handing a replayed batch to an eager function.

    Refused with ValueError before anything is captured: what ``ReplayedClfEval`` and ``GNNExplainer`` refuse, and a dataset without
    ``edge_label_all``."""

    _PHASES = ("begin", "step", "end")

    def __init__(self, clf, criterion, dataset, batch_size: int, k: int, steps: int = 100, lr: float = 0.01, betas=(0.9, 0.999),
                 eps: float = 1e-8, size_coef: float = 0.005, ent_coef: float = 1.0, symmetric: bool = True, target: str = "model",
                 capacity: Optional[tuple] = None, ragged: bool = False, bins: int = 64, max_graphs: Optional[int] = None,
                 max_edges: Optional[int] = None, graphs: Optional[tuple] = None):
        from .baselines import GNNExplainer, MaskState
        _clf_refusals("ReplayedGNNExplainer", clf, criterion, dataset)
        self.explainer = GNNExplainer(clf, criterion, steps, lr, betas, eps, size_coef, ent_coef, symmetric, target)
        if getattr(dataset, "edge_label_all", None) is None:
            raise ValueError("ReplayedGNNExplainer needs a dataset with edge labels (edge_label_all)")
        _check_log_sizes(k, bins)
        self.model, self.criterion, self.dataset, self.steps = clf, criterion, dataset, self.explainer.steps
        if graphs is not None and len(graphs) != 3:
            raise ValueError("graphs is the triple (begin, step, end) of torch.cuda.CUDAGraph objects")
        self._setup(clf, (dataset,), batch_size, capacity, None if graphs is None else graphs[0], ragged)
        later = graphs[1:] if graphs is not None else (torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph())
        self.graphs = self._graphs = dict(zip(self._PHASES, (self.graph,) + tuple(later)))
        self.mask = MaskState(self.capacity[1], dataset.x_all.device)
        self._ctx = self.log = self.batch = self.edge_att = self.mask_logits = self.clf_logits = self.losses = None
        sizes = (int(k), int(bins), max_graphs, max_edges)
        _capture_evaluator(self, lambda: self._make_log(sizes))

    def _make_log(self, sizes):
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        with torch.no_grad():
            logits = _clf_forward(self.model, self.criterion, b)[0]
        self.log, = _new_logs(self, 1, logits, *sizes)

    # -- the three bodies ------------------------------------------------------------------------------------------------------------
    def _begin(self):
        clear_cache()
        b = self.dataset.collate_padded(self.graph_ids, self.capacity, ragged=self.ragged)
        self._ctx = self.explainer.begin(b, self.mask)

    def _step(self):
        self.explainer.step(self._ctx, self.mask)

    def _finish(self, ctx, mask):
        """Objective of the final mask, the scored mask, the append; returns what a batch publishes."""
        ex = self.explainer
        with torch.no_grad():
            pred, size, ent = ex.objective(ctx, mask).unbind(0)
            reg = ex.size_coef * size + ex.ent_coef * ent
            losses = torch.stack([pred + reg, pred, reg])
            att = ex.edge_att(ctx, mask)
            self.log.append(att, ctx["data"], ctx["logits"], losses)
        return dict(batch=ctx["data"], edge_att=att, mask_logits=mask.m, clf_logits=ctx["logits"], losses=losses)

    def _end(self):
        self._publish(False, **self._finish(self._ctx, self.mask))

    def run_once(self):
        """begin, ``steps`` times step, end, eagerly on the current stream."""
        self._begin()
        for _ in range(self.steps):
            self._step()
        self._end()

    def _warm_up_and_capture(self, setup=None, before_capture=None):
        """``_Replayed``'s protocol for a chain of bodies: three eager runs of begin, step, end on a side stream, the one host read that
        tells whether the warm-up batch fit, then one capture per phase, in order -- each phase is captured on what the capture of the
        one before it left behind."""
        from .baselines import _frozen
        bodies = dict(begin=self._begin, step=self._step, end=self._end)
        with _frozen(self.model):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                if setup is not None:
                    setup()
                for _ in range(3):
                    for name in self._PHASES:
                        bodies[name]()
            torch.cuda.current_stream().wait_stream(side)
            if int(self.batch.valid[3]) != 0:
                raise ValueError(f"{type(self).__name__}: graphs 0..{self.batch_size - 1} do not fit the capacity {self.capacity}")
            if before_capture is not None:
                before_capture()
            for name in self._PHASES:
                with torch.cuda.graph(self._graphs[name]):
                    bodies[name]()

    def step(self, graph_ids, epoch: int = 0) -> None:
        """Explain one batch: the ids are copied in, then begin, ``steps`` times step and end are replayed.  Nothing is read back."""
        self._load_ids(graph_ids)
        self._graphs["begin"].replay()
        step = self._graphs["step"]
        for _ in range(self.steps):
            step.replay()
        self._graphs["end"].replay()

    def _forward(self, b, epoch=0):
        """The eager tail: the same three phases on the collated batch ``b`` with a mask state of its size."""
        from .baselines import MaskState, _frozen
        mask = MaskState(int(b.edge_index.shape[1]), b.edge_index.device)
        with _frozen(self.model):
            ctx = self.explainer.begin(b, mask)
            for _ in range(self.steps):
                self.explainer.step(ctx, mask)
            return self._finish(ctx, mask)

    def run(self, graph_ids, epoch: int = 0) -> dict:
        """One explanation epoch over ``graph_ids`` (any number, in visiting order): the log is reset, every full batch is replayed
        (ragged: every row of ``batches``), a tail of fewer than ``batch_size`` graphs runs eagerly, and ``log.compute()`` -- two host
        reads -- gives the scores.  The eager tail is logged but NOT published: afterwards ``batch``, ``edge_att`` and ``mask_logits`` are
        those of the last REPLAYED batch, which is not the last batch of the epoch when there was a tail."""
        return _run_epoch(self, graph_ids, 0)
