"""Post-hoc explainers of a trained backbone, for GSAT's attention to be compared against: gradient saliency and a batched GNNExplainer.

Both run the project's hot path -- the mask-weighted message passing, forward and backward with respect to ``edge_atten`` -- and give a
per-edge score vector that every meter, log and fidelity function of the package takes where it takes GSAT's attention.  The
GNNExplainer objective, its derivative through the sigmoid and the Adam step on the mask logits are ONE launch of
csrc/mask_explainer.hip per optimisation step (plus one single-thread launch that advances the step counter); the objective of a
batch is the sum of its graphs' objectives, so all graphs of a batch are explained at once and a graph's mask does not depend on what
else is in the batch.  There is no CPU fallback.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Optional

import torch

from ._lib import GsatHipError, call, ptr, stream
from .graph_index import get_index
from .gsat import symmetrise_edge_att
from .padding import padded

_TARGETS = ("model", "label")


# ---- what both explainers share -------------------------------------------------------------------------------------------------------------
def _refuse(clf, criterion=None):
    """The refusals of both explainers, said before any launch."""
    if hasattr(clf, "forward_pass") or hasattr(clf, "dual_forward_pass"):
        raise ValueError("the post-hoc explainers take a bare backbone (get_model), not a GSAT / DualGSAT object: pass its clf")
    if any(getattr(m, "sync_group", None) for m in clf.modules()):
        raise ValueError("the post-hoc explainers cannot take sync_group BatchNorm (its statistics are reduced over ranks on the host's schedule)")
    if criterion is not None and getattr(criterion, "multi_label", False):
        raise ValueError("the post-hoc explainers explain one class per graph: a multi-label criterion is not covered")


def _check_target(target):
    if target not in _TARGETS:
        raise ValueError(f"target must be one of {_TARGETS}")
    return target


@contextmanager
def _frozen(clf):
    """Eval mode and frozen parameters inside the block; every module's training flag and every parameter's ``requires_grad`` are put
    back on exit.  Nothing else of the model is touched: eval-mode BatchNorm writes no buffer, eval-mode dropout draws nothing, and the
    explainers take gradients with ``torch.autograd.grad`` with respect to the mask alone, so no ``.grad`` appears."""
    modes = [(m, m.training) for m in clf.modules()]
    flags = [(p, p.requires_grad) for p in clf.parameters()]
    clf.eval()
    for p, _ in flags:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for m, t in modes:
            m.training = t
        for p, f in flags:
            p.requires_grad_(f)


def _segments(data):
    """(index, graph segments) of a collated or padded batch, without a host read when the batch knows its graph count."""
    if not data.edge_index.is_cuda:
        raise GsatHipError("dp_gsat_amd.baselines needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    N = int(data.x.shape[0])
    index = get_index(data.edge_index, N)
    num_graphs = getattr(data, "num_graphs", None)
    return index, index.graphs(data.batch, None if num_graphs is None else int(num_graphs))


def _valid(data):
    valid = getattr(data, "valid", None)
    if valid is not None and (valid.dtype != torch.int32 or valid.numel() < 4 or not valid.is_cuda):
        raise ValueError("data.valid must be an int32 ROCm tensor (N_real, E_real, B, overflow)")
    return None if valid is None else valid.contiguous()


def _forward(clf, data, edge_atten):
    """The backbone's logits on ``data`` with ``edge_atten`` (None: unmasked); a padded batch runs inside ``padded()``."""
    valid = getattr(data, "valid", None)
    if valid is None:
        return clf(data.x, data.edge_index, data.batch, edge_attr=data.edge_attr, edge_atten=edge_atten)
    with padded(valid, (int(data.x.shape[0]), int(data.edge_index.shape[1]))):
        return clf(data.x, data.edge_index, data.batch, edge_attr=data.edge_attr, edge_atten=edge_atten)


def _real_rows(data, t):
    """The rows of the real graphs (and graph slots) of a per-graph tensor: all but the padding graph of a padded batch."""
    return t if getattr(data, "valid", None) is None else t[: int(data.num_graphs) - 1]


def _predicted(logits):
    """The class the classifier predicts, per row: ``z > 0`` of a single-logit head, else the argmax with the lowest index on ties."""
    if logits.shape[1] == 1:
        return (logits > 0).to(torch.float32)
    C = int(logits.shape[1])
    cols = torch.arange(C, device=logits.device).expand_as(logits)
    best = logits == logits.max(dim=1, keepdim=True).values
    return torch.where(best, cols, torch.full_like(cols, C)).min(dim=1).values.clamp_(max=C - 1).to(torch.float32)


def _targets(data, logits, target):
    """The target of every graph as the criterion takes it: [G, 1] 0/1 floats for a single-logit head, [G] class ids else."""
    if target == "model":
        return _predicted(logits.detach())
    if getattr(data, "y", None) is None:
        raise ValueError("target='label' needs data.y")
    y = data.y.detach().to(torch.float32)
    return y.reshape(-1, 1) if logits.shape[1] == 1 else y.reshape(-1)


# ---- per-graph normalisation ---------------------------------------------------------------------------------------------------------------
def normalise_per_graph(att, data, power: float = 1.0, eps: float = 1e-6) -> torch.Tensor:
    """``(att ** power - min_g) / (max_g - min_g + eps)`` over the edges of every graph of ``data`` (an edge belongs to the graph of its
    source), in ``att``'s shape ([E] or [E, 1]).  ``power=10, eps=1e-6`` is the reference's ``visualize_a_graph(norm=True)``
    (src/utils/utils.py:105-107); ``power=1`` is plain min-max.  Graphs with one edge and constant graphs give 0.  On a ``PaddedBatch``
    only the real graphs are normalised and the padding entries are 0.  One launch, nothing read back."""
    if not isinstance(att, torch.Tensor) or not att.is_cuda:
        raise GsatHipError("dp_gsat_amd.baselines needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    if not float(power) > 0.0 or float(eps) < 0.0:
        raise ValueError("normalise_per_graph needs power > 0 and eps >= 0")
    index, seg = _segments(data)
    a = att.detach().reshape(-1).to(torch.float32).contiguous()
    if int(a.shape[0]) != index.E:
        raise ValueError(f"attention has {int(a.shape[0])} entries for {index.E} edges")
    out = torch.empty_like(a)
    eptr, eorder = seg.edge_segments[:2]
    call("gsat_segment_minmax_norm", ptr(a) if index.E else None, ptr(eptr), ptr(eorder) if index.E else None, index.E, seg.G, float(power),
         float(eps), ptr(_valid(data)), ptr(out) if index.E else None, stream())
    return out.view(att.shape)


# ---- gradient saliency ---------------------------------------------------------------------------------------------------------------------
def edge_saliency(clf, data, target: str = "model", absolute: bool = True) -> torch.Tensor:
    """float32[E]: ``d z_target / d edge_atten`` at ``edge_atten = 1`` of every edge, from ONE eval-mode forward and backward of the
    backbone ``clf`` on the collated or padded batch ``data``.  ``target``: "model" -- the class the classifier predicts, ``z > 0`` or
    the argmax with the lowest index on ties -- or "label" (``data.y``).  The target column of a single-logit head is the logit, signed
    by the class: ``+z`` for class 1, ``-z`` for class 0.  ``absolute``: the magnitude.  Graphs do not interact, so the gradient of the
    sum over the graphs is every graph's own; padding entries are 0.

    The classifier runs in eval mode with its parameters frozen; training and ``requires_grad`` flags are put back afterwards and no
    ``.grad``, buffer, optimizer state or seed stream is touched."""
    _refuse(clf)
    _check_target(target)
    index, _ = _segments(data)
    with _frozen(clf):
        att = torch.ones((index.E, 1), dtype=torch.float32, device=data.edge_index.device, requires_grad=True)
        logits = _forward(clf, data, att)
        z = _real_rows(data, logits)
        t = _real_rows(data, _targets(data, logits, target))
        if logits.shape[1] == 1:
            score = (z * (2.0 * t - 1.0)).sum()
        else:
            score = z.gather(1, t.long().clamp(0, int(z.shape[1]) - 1).view(-1, 1)).sum()
        grad, = torch.autograd.grad(score, att)
    grad = grad.reshape(-1)
    return grad.abs() if absolute else grad


# ---- GNNExplainer --------------------------------------------------------------------------------------------------------------------------
class MaskState:
    """The device state of one mask optimisation over ``E`` edge slots: mask logits ``m``, Adam moments ``mu`` / ``nu``, ``a =
    sigmoid(m)``, ``inv_eg`` (1 / edge count of every edge's graph) and ``state`` float32[4] = (steps taken, the two bias corrections of
    the next step, 0).  Allocated once; ``gsat_mask_init`` writes all of it, so it needs no zeroing."""

    def __init__(self, E: int, device):
        new = lambda n: torch.empty(max(int(n), 1), dtype=torch.float32, device=device)[: int(n)]
        self.E = int(E)
        self.m, self.mu, self.nu, self.a, self.inv_eg = (new(E) for _ in range(5))
        self.state = torch.empty(4, dtype=torch.float32, device=device)


class Explanation:
    """What ``GNNExplainer.explain`` returns: ``edge_att`` [E, 1] (the mask, symmetrised when asked for), ``mask_logits`` [E], ``logits``
    (the classifier's on the unmasked batch), ``targets`` (the class explained, as the criterion takes it), ``objective`` float32[3] =
    (pred, size, entropy) of the returned (raw) mask and ``history`` [steps, 3]: the same triple of the mask every step started from, or
    None.  The batch's objective is ``pred + size_coef * size + ent_coef * entropy``."""
    __slots__ = ("edge_att", "mask_logits", "logits", "targets", "objective", "history")

    def __init__(self, edge_att, mask_logits, logits, targets, objective, history):
        self.edge_att, self.mask_logits, self.logits, self.targets = edge_att, mask_logits, logits, targets
        self.objective, self.history = objective, history


class GNNExplainer:
    """``GNNExplainer(clf, criterion, steps=100, lr=0.01, betas=(0.9, 0.999), eps=1e-8, size_coef=0.005, ent_coef=1.0, symmetric=True,
    target="model")``: PyG's GNNExplainer for edge masks (``edge_reduction='sum'`` for the size term, a mean for the entropy) on the
    backbone ``clf``, all graphs of a batch at once.  Per batch the objective is

        L = sum_g crit_g(z_g, t_g) + sum_e [ size_coef * a_e + ent_coef * H(a_e) / E_g(e) ],   a = sigmoid(m)

    and a step is the masked forward, ``criterion`` (the project's mean over the graphs; the kernel multiplies its gradient by the graph
    count, read on the device), one ``torch.autograd.grad`` with respect to ``a`` and ``gsat_mask_step``: the regularisers' derivative,
    the chain through the sigmoid, torch's Adam (no weight decay, no amsgrad) and the next ``a`` in one launch.

    ``target``: "model" -- the class the classifier predicts on the unmasked graph (``z > 0``, or the argmax with the lowest index on
    ties), computed once under ``no_grad`` -- or "label" (``data.y``).  ``symmetric``: the returned mask is averaged with the reverse
    edge when the batch is undirected (``symmetrise_edge_att``, GSAT's own convention); the optimisation itself runs on the raw mask.

    The classifier runs in eval mode with frozen parameters for the duration; training and ``requires_grad`` flags are put back and no
    ``.grad``, buffer, optimizer state or seed stream is touched.  Refused with ValueError before any launch: a multi-label criterion,
    ``GSAT`` / ``DualGSAT`` objects (pass the backbone), ``sync_group`` BatchNorm, ``steps < 1``, a non-positive ``lr``, negative
    coefficients."""

    def __init__(self, clf, criterion, steps: int = 100, lr: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8, size_coef: float = 0.005,
                 ent_coef: float = 1.0, symmetric: bool = True, target: str = "model"):
        _refuse(clf, criterion)
        if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
            raise ValueError("steps must be an int >= 1")
        if not float(lr) > 0.0:
            raise ValueError("lr must be positive")
        if float(size_coef) < 0.0 or float(ent_coef) < 0.0:
            raise ValueError("size_coef and ent_coef must not be negative")
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or float(eps) < 0.0:
            raise ValueError("betas must lie in [0, 1) and eps must not be negative")
        self.clf, self.criterion, self.steps, self.lr, self.betas, self.eps = clf, criterion, int(steps), float(lr), (b1, b2), float(eps)
        self.size_coef, self.ent_coef, self.symmetric, self.target = float(size_coef), float(ent_coef), bool(symmetric), _check_target(target)

    # -- the three phases; ReplayedGNNExplainer captures each into a graph of its own ------------------------------------------------
    def begin(self, data, mask: MaskState, init=None, init_value: float = 0.0) -> dict:
        """The unmasked forward, the targets and ``gsat_mask_init``.  ``init`` float32[E] (or None: ``init_value`` everywhere) are the
        first mask logits.  Returns the context the other phases take.  Runs under ``_frozen``."""
        index, seg = _segments(data)
        E = index.E
        if mask.E != E:
            raise ValueError(f"the mask state has {mask.E} entries for {E} edge slots")
        if init is not None:
            init = init.detach().reshape(-1).to(torch.float32).contiguous()
            if int(init.shape[0]) != E or not init.is_cuda:
                raise ValueError(f"init must be a ROCm tensor with one logit per edge slot ({E})")
        valid = _valid(data)
        with torch.no_grad():
            logits = _forward(self.clf, data, None)
            targets = _targets(data, logits, self.target)
        eptr, eorder = seg.edge_segments[:2]
        some = lambda t: ptr(t) if t.numel() else None
        call("gsat_mask_init", ptr(init) if init is not None and E else None, float(init_value), some(index.src32), some(seg.node_seg32),
             ptr(eptr), index.N, seg.G, E, self.betas[0], self.betas[1], some(mask.m), some(mask.mu), some(mask.nu), some(mask.a),
             some(mask.inv_eg), ptr(mask.state), stream())
        if valid is None:
            g_valid, count = None, None
        else:           # filled slots of a ragged batch; a fixed-count batch keeps B in valid[2] when it overflows
            g_valid = valid[2:3] if getattr(data, "ragged", False) else valid[2:3] * (1 - valid[3:4])
            count = g_valid.to(torch.float32)
        return dict(data=data, index=index, seg=seg, valid=valid, logits=logits, targets=targets, g_valid=g_valid, count=count,
                    eptr=eptr, eorder=eorder, objective=torch.empty(3, dtype=torch.float32, device=logits.device),
                    terms=torch.empty((seg.G, 2), dtype=torch.float32, device=logits.device))

    def _objective(self, ctx, mask, loss, out):
        """out[3] <- (sum_g crit_g, sum_e a_e, sum_g mean H) of the mask the forward behind ``loss`` ran with."""
        E, G = mask.E, ctx["seg"].G
        call("gsat_mask_objective", ptr(mask.a) if E else None, ptr(ctx["eptr"]), ptr(ctx["eorder"]) if E else None, E, G,
             ptr(ctx["valid"]), ptr(ctx["terms"]), stream())
        graphs = float(_real_rows(ctx["data"], ctx["logits"]).shape[0]) if ctx["count"] is None else ctx["count"].reshape(())
        out[0] = loss.detach() * graphs
        out[1:] = ctx["terms"].sum(dim=0)

    def _masked_loss(self, ctx, att):
        data = ctx["data"]
        logits = _forward(self.clf, data, att)
        z, t = _real_rows(data, logits), _real_rows(data, ctx["targets"])
        return self.criterion(z, t) if ctx["g_valid"] is None else self.criterion(z, t, g_valid=ctx["g_valid"])

    def step(self, ctx, mask: MaskState, history_row=None) -> None:
        """One optimisation step: masked forward, criterion, backward to ``a``, ``gsat_mask_step``.  ``history_row`` float32[3]: also
        record (pred, size, entropy) of this step's forward there (four more launches)."""
        E = mask.E
        att = mask.a.view(E, 1).detach().requires_grad_(True)
        loss = self._masked_loss(ctx, att)
        grad, = torch.autograd.grad(loss, att)
        grad = grad.reshape(-1).to(torch.float32).contiguous()
        if history_row is not None:
            with torch.no_grad():
                self._objective(ctx, mask, loss, history_row)
        some = lambda t: ptr(t) if t.numel() else None
        call("gsat_mask_step", some(mask.m), some(mask.mu), some(mask.nu), some(mask.a), some(grad), some(mask.inv_eg), E,
             int(_real_rows(ctx["data"], ctx["logits"]).shape[0]), ptr(ctx["valid"]), ptr(mask.state), self.lr, self.betas[0],
             self.betas[1], self.eps, self.size_coef, self.ent_coef, stream())

    def objective(self, ctx, mask: MaskState) -> torch.Tensor:
        """float32[3] = (pred, size, entropy) of the mask as it stands, from one more masked forward under ``no_grad``: the batch's
        objective is ``pred + size_coef * size + ent_coef * entropy``."""
        with torch.no_grad():
            self._objective(ctx, mask, self._masked_loss(ctx, mask.a.view(mask.E, 1)), ctx["objective"])
        return ctx["objective"]

    def edge_att(self, ctx, mask: MaskState) -> torch.Tensor:
        """[E, 1]: the mask as the meters take it -- a copy of ``a``, symmetrised when ``symmetric`` and the batch is undirected."""
        a = mask.a.view(mask.E, 1)
        with torch.no_grad():
            if self.symmetric and mask.E:
                out = symmetrise_edge_att(a, ctx["data"].edge_index, int(ctx["data"].x.shape[0]))
                return out.clone() if out is a else out
            return a.clone()

    def explain(self, data, init=None, history: bool = False) -> Explanation:
        """Explain every graph of the collated or padded batch ``data`` in ``steps`` optimisation steps from the mask logits ``init``
        ([E], default 0).  ``history``: keep (pred, size, entropy) of every step's forward, [steps, 3] on the device.  A padded batch
        runs inside ``padded()`` and the criterion reads its graph count on the device; its padding entries keep their first logits and
        an overflowing batch updates nothing.  Nothing is read back."""
        index, _ = _segments(data)
        mask = MaskState(index.E, data.edge_index.device)
        hist = torch.empty((self.steps, 3), dtype=torch.float32, device=data.edge_index.device) if history else None
        with _frozen(self.clf):
            ctx = self.begin(data, mask, init)
            for i in range(self.steps):
                self.step(ctx, mask, None if hist is None else hist[i])
            objective = self.objective(ctx, mask)
            att = self.edge_att(ctx, mask)
        return Explanation(att, mask.m, ctx["logits"], ctx["targets"], objective, hist)
