"""Explanation subgraphs on the device: edge / node subgraph extraction with relabelling, top-k explanation subgraphs, fidelity.

The reference cuts the attended subgraph out on the host, graph by graph, after copying everything back
(example/trainer.py:140-170: ``subgraph(node_subset.cpu(), data.edge_index.cpu(), edge_attr=batch_att)``).  Here a 0/1 mask over the
edges (or the nodes) of a whole collated batch becomes a new collated batch in 4-6 kernel launches plus one row gather per
attribute (csrc/subgraph.hip); kept nodes and edges stay in their original order, so the result is unique.

Why a compacted graph and not a hard 0/1 ``edge_atten``: for GIN / GINE (a masked sum) the two are the same thing, for
``PNAConvSimple`` they are not -- a message scaled by 0 still enters ``mean``, ``min``, ``max``, ``std`` and the in-degree.  Fidelity of
a PNA model therefore needs the graph WITHOUT the edges (:func:`explanation_fidelity`).

:func:`edge_subgraph_padded` / :func:`node_subgraph_padded` extract into a batch of a fixed capacity (a ``PaddedBatch``: the kept part
first, the slack as the padding graph, the counts in ``valid`` on the device): no size is needed from the host, so the extraction
replays inside a captured graph (``ReplayedFidelity``).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._lib import GsatHipError, call, ptr, stream
from .collate import PaddedBatch, _take_padded
from .explain import topk_edge_mask
from .graph_index import call_size, get_index, sync_free
from .synth import Batch

_NO_CPU = "dp_gsat_amd.subgraph needs ROCm (cuda) tensors: the HIP path has no CPU fallback"


def subgraph_block_items() -> int:
    """Items (nodes or edges) one workgroup of the extraction kernels owns."""
    return int(_lib.load().gsat_subgraph_block_items())


class SubgraphBatch(Batch):
    """The extracted batch: ``x, edge_index, batch, edge_attr, edge_label, node_label`` of the kept nodes / edges, ``y`` and
    ``num_graphs`` unchanged (a graph that lost every node is an empty segment), plus ``node_id int64[N']`` / ``edge_id int64[E']``
    (old ids, ascending), ``edge_mask bool[E]`` over the ORIGINAL edges, ``node_ptr int32[G+1]`` and ``counts int64[4]`` =
    (N', E', overflow, bad id) on the device."""

    def check(self) -> "SubgraphBatch":
        """One host read of ``counts``: raises ValueError when the ``sizes`` the extraction was given were not the true sizes
        (nothing was written beyond them) or an edge had a node id outside [0, N)."""
        n, e, over, bad = self.counts.tolist()
        if bad:
            raise ValueError("edge_index contains node ids outside [0, num_nodes)")
        if over:
            raise ValueError(f"subgraph sizes were declared as {tuple(self.sizes)} but the extraction keeps ({n}, {e})")
        return self

    def prime(self) -> "SubgraphBatch":
        """Register ``batch`` with ``num_graphs`` at the batch index of ``edge_index``: a model forward on this batch then returns
        ``num_graphs`` rows also when the last graphs are empty, and never reads ``batch.max()`` back.  Done by the extraction
        itself, except during stream capture and for an empty result."""
        if self.num_nodes > 0 and self.num_edges > 0:
            get_index(self.edge_index, self.num_nodes).graphs(self.batch, self.num_graphs)
        return self


def _need_cuda(*tensors):
    for t in tensors:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise GsatHipError(_NO_CPU)


def _keep_u8(keep, n: int, what: str) -> torch.Tensor:
    """0/1-or-nonzero uint8[n] view of a mask (bool and uint8 masks cost nothing)."""
    keep = keep.reshape(-1)
    if keep.shape[0] != n:
        raise ValueError(f"{what} has {keep.shape[0]} entries for {n}")
    if keep.dtype == torch.uint8:
        return keep.contiguous()
    return keep.contiguous().view(torch.uint8) if keep.dtype == torch.bool else (keep != 0).to(torch.uint8)


def gather_rows(table: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """``table[index]`` along dim 0 for a tensor of any dtype and trailing shape (gsat_gather_rows); ``index`` int64, trusted."""
    _need_cuda(table, index)
    if index.dtype != torch.int64 or index.dim() != 1:
        raise ValueError("index must be an int64 vector")
    table = table.contiguous()
    n = int(index.shape[0])
    out = torch.empty((n,) + tuple(table.shape[1:]), dtype=table.dtype, device=table.device)
    row_bytes = table.element_size()
    for s in table.shape[1:]:
        row_bytes *= int(s)
    if n and row_bytes:
        call("gsat_gather_rows", ptr(table), ptr(index.contiguous()), n, row_bytes, ptr(out), stream())
    return out


def _extract(data, keep: torch.Tensor, mode: int, drop_isolated: bool, sizes: Optional[Sequence[int]]) -> SubgraphBatch:
    x, edge_index, batch = data.x, data.edge_index, data.batch
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
    N, E, dev = int(x.shape[0]), int(edge_index.shape[1]), edge_index.device
    if batch.dtype != torch.int64 or batch.dim() != 1 or int(batch.shape[0]) != N:
        raise ValueError("batch must be an int64 vector with one entry per node")
    if keep.numel() != (E if mode == 0 else N):
        raise ValueError(f"{'edge_keep' if mode == 0 else 'node_keep'} has {keep.numel()} entries for {E if mode == 0 else N}")
    _need_cuda(x, edge_index, batch, keep)
    keep = _keep_u8(keep, E if mode == 0 else N, "edge_keep" if mode == 0 else "node_keep")
    capturing = torch.cuda.is_current_stream_capturing()
    if sizes is None and (sync_free() or capturing):
        raise ValueError("edge_subgraph / node_subgraph read the sizes of the result back once; in sync-free mode or during "
                         "stream capture pass sizes=(num_nodes, num_edges) of the result instead")
    if sizes is not None:
        sizes = (int(sizes[0]), int(sizes[1]))
        if not (0 <= sizes[0] <= N and 0 <= sizes[1] <= E):
            raise ValueError(f"sizes {sizes} outside (0..{N}, 0..{E})")
    seg = get_index(edge_index, N).graphs(batch, getattr(data, "num_graphs", None))
    G = seg.G
    ei = edge_index.contiguous()
    ws_bytes = max(call_size("gsat_subgraph_workspace_bytes", N, E), 256)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    edge_mask = torch.empty(E, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    new_ptr = torch.empty(G + 1, dtype=torch.int32, device=dev)

    def run(phases, n_out, e_out, out):
        call("gsat_subgraph_index", ptr(ei) if E else None, E, N, ptr(seg.batch) if N else None, ptr(seg.node_ptr), G,
             ptr(keep) if keep.numel() else None, mode, int(bool(drop_isolated)), phases, n_out, e_out, 1,
             *(ptr(t) if t is not None and t.numel() else None for t in out), ptr(new_ptr), ptr(edge_mask) if E else None,
             ptr(counts), ptr(ws), ws_bytes, stream())

    if sizes is None:
        run(1, -1, -1, (None, None, None, None))
        n_out, e_out, _, bad = counts.tolist()               # the one host read
        if bad:
            raise ValueError("edge_index contains node ids outside [0, num_nodes)")
    else:
        n_out, e_out = sizes
    node_id = torch.empty(n_out, dtype=torch.int64, device=dev)
    edge_id = torch.empty(e_out, dtype=torch.int64, device=dev)
    new_ei = torch.empty(2, e_out, dtype=torch.int64, device=dev)
    new_batch = torch.empty(n_out, dtype=torch.int64, device=dev)
    run(2 if sizes is None else 3, n_out, e_out, (node_id, edge_id, new_ei, new_batch))

    sub = SubgraphBatch(x=gather_rows(x, node_id), edge_index=new_ei, batch=new_batch, y=getattr(data, "y", None), num_graphs=G,
                        node_id=node_id, edge_id=edge_id, edge_mask=edge_mask.view(torch.bool), node_ptr=new_ptr, counts=counts,
                        sizes=(n_out, e_out))
    for name, index in (("edge_attr", edge_id), ("edge_label", edge_id), ("node_label", node_id)):
        t = getattr(data, name, None)
        if isinstance(t, torch.Tensor):
            _need_cuda(t)
            if int(t.shape[0]) != (E if index is edge_id else N):
                raise ValueError(f"{name} has {t.shape[0]} rows")
            t = gather_rows(t, index)
        setattr(sub, name, t)
    if not capturing:
        sub.prime()
    return sub


def edge_subgraph(data, edge_keep: torch.Tensor, drop_isolated: bool = True, sizes: Optional[Tuple[int, int]] = None) -> SubgraphBatch:
    """The batch restricted to the edges with ``edge_keep`` (bool / nonzero, [E]).  ``drop_isolated``: keep only the endpoints of the
    kept edges (relabelled); otherwise every node stays and only ``edge_index`` and the edge attributes shrink.
    ``data``: anything with ``x``, ``edge_index``, ``batch`` and optionally ``edge_attr``, ``edge_label``, ``node_label``, ``y``,
    ``num_graphs`` (a synth.Batch, a PyG batch).  One host read (the result's sizes) per call; ``sizes=(N', E')`` skips it -- the call
    is then capturable (bool / uint8 masks), nothing is written beyond the declared sizes and a wrong declaration raises at the
    result's ``.check()``."""
    if not isinstance(edge_keep, torch.Tensor):
        raise ValueError("edge_keep must be a tensor")
    return _extract(data, edge_keep, 0, drop_isolated, sizes)


def node_subgraph(data, node_keep: torch.Tensor, sizes: Optional[Tuple[int, int]] = None) -> SubgraphBatch:
    """PyG ``subgraph(node_keep, edge_index, relabel_nodes=True)`` on a whole collated batch (example/trainer.py:168): the kept nodes,
    relabelled in order, and the edges with both endpoints kept.  ``node_keep``: a bool mask [N]; an int64 id list is turned into
    one."""
    if not isinstance(node_keep, torch.Tensor):
        raise ValueError("node_keep must be a tensor")
    if node_keep.dtype == torch.int64:
        _need_cuda(data.x, node_keep)
        mask = torch.zeros(int(data.x.shape[0]), dtype=torch.uint8, device=node_keep.device)
        mask[node_keep.reshape(-1)] = 1
        node_keep = mask
    return _extract(data, node_keep, 1, False, sizes)


class PaddedSubgraphBatch(PaddedBatch):
    """The extracted batch of :func:`edge_subgraph_padded` / :func:`node_subgraph_padded`: a ``PaddedBatch`` of the declared ``capacity``
    -- kept nodes and edges first, the slack as the padding graph ``num_graphs - 1`` -- with ``valid`` (int32[4] on the device: N', E',
    graphs, overflow), ``node_id int64[N_cap]`` / ``edge_id int64[E_cap]`` (old ids, ascending, -1 for padding), ``edge_mask bool[E]`` over
    the ORIGINAL edge slots and ``y`` unchanged."""

    def check(self) -> "PaddedSubgraphBatch":
        """One host read of ``valid``: raises ValueError when the extraction overflowed (the batch is then all padding)."""
        if int(self.valid[3]):
            raise ValueError(_overflow_text(self.capacity))
        return self


def _overflow_text(capacity) -> str:
    return (f"the extraction does not fit the capacity (N_cap, E_cap) = {tuple(capacity)} (two padding nodes must remain), its input "
            "had overflowed, or edge_index contains node ids outside [0, num_nodes)")


def _extract_padded(data, keep: torch.Tensor, mode: int, drop_isolated: bool, capacity) -> PaddedSubgraphBatch:
    x, edge_index, batch = data.x, data.edge_index, data.batch
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
    N, E, dev = int(x.shape[0]), int(edge_index.shape[1]), edge_index.device
    if batch.dtype != torch.int64 or batch.dim() != 1 or int(batch.shape[0]) != N:
        raise ValueError("batch must be an int64 vector with one entry per node")
    what = "edge_keep" if mode == 0 else "node_keep"
    if keep.numel() != (E if mode == 0 else N):
        raise ValueError(f"{what} has {keep.numel()} entries for {E if mode == 0 else N}")
    N_cap, E_cap = int(capacity[0]), int(capacity[1])
    if N_cap < 2 or E_cap < 0:
        raise ValueError("a padded extraction needs a capacity of at least two nodes (the padding nodes)")
    _need_cuda(x, edge_index, batch, keep)
    keep = _keep_u8(keep, E if mode == 0 else N, what)
    valid_in = getattr(data, "valid", None)
    if valid_in is not None:
        if valid_in.dtype != torch.int32 or valid_in.numel() < 4 or not valid_in.is_cuda:
            raise ValueError("data.valid must be an int32 ROCm tensor (N_real, E_real, B, overflow)")
        valid_in = valid_in.contiguous()
        num_graphs = int(data.num_graphs)                    # the input's own padding graph stays the padding graph
        real_graphs = num_graphs - 1
    else:
        real_graphs = getattr(data, "num_graphs", None)
        if real_graphs is None:
            if sync_free() or torch.cuda.is_current_stream_capturing():
                raise ValueError("a padded extraction of a batch without num_graphs would read batch.max() back")
            real_graphs = int(batch.max().item()) + 1 if N else 0
        real_graphs = int(real_graphs)
        num_graphs = real_graphs + 1
    ei, batch = edge_index.contiguous(), batch.contiguous()
    # every real node kept at the input's own shape: rows and graph ids are the input's, padding rows included
    shares_nodes = mode == 0 and not drop_isolated and valid_in is not None and N_cap == N
    ws_bytes = max(call_size("gsat_subgraph_workspace_bytes", N, E), 256)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    edge_mask = torch.empty(E, dtype=torch.uint8, device=dev)
    valid = torch.empty(4, dtype=torch.int32, device=dev)
    node_id = torch.empty(N_cap, dtype=torch.int64, device=dev)
    edge_id = torch.empty(E_cap, dtype=torch.int64, device=dev)
    new_ei = torch.empty(2, E_cap, dtype=torch.int64, device=dev)
    new_batch = None if shares_nodes else torch.empty(N_cap, dtype=torch.int64, device=dev)
    some = lambda t: ptr(t) if t is not None and t.numel() else None
    call("gsat_subgraph_padded", some(ei), E, N, None if shares_nodes or not N else ptr(batch), real_graphs, some(keep), mode,
         int(bool(drop_isolated)), ptr(valid_in) if valid_in is not None else None, num_graphs - 1, N_cap, E_cap, ptr(node_id),
         some(edge_id), some(new_ei), some(new_batch), some(edge_mask), ptr(valid), ptr(ws), ws_bytes, stream())
    if not (sync_free() or torch.cuda.is_current_stream_capturing()) and int(valid[3]):          # the one host read
        raise ValueError(_overflow_text((N_cap, E_cap)))
    sub = PaddedSubgraphBatch(x=x if shares_nodes else _take_padded(x, node_id), edge_index=new_ei,
                              batch=batch if shares_nodes else new_batch, y=getattr(data, "y", None), num_graphs=num_graphs, valid=valid,
                              capacity=(N_cap, E_cap), node_id=node_id, edge_id=edge_id, edge_mask=edge_mask.view(torch.bool))
    for name, index in (("edge_attr", edge_id), ("edge_label", edge_id), ("edge_att", edge_id), ("node_label", node_id)):
        t = getattr(data, name, None)
        if isinstance(t, torch.Tensor):
            _need_cuda(t)
            if int(t.shape[0]) != (E if index is edge_id else N):
                raise ValueError(f"{name} has {t.shape[0]} rows")
            t = t if (index is node_id and shares_nodes) else _take_padded(t, index)
        if t is not None or name != "edge_att":
            setattr(sub, name, t)
    for name in ("ragged", "r"):
        if hasattr(data, name):
            setattr(sub, name, getattr(data, name))
    return sub


def edge_subgraph_padded(data, edge_keep: torch.Tensor, capacity: Tuple[int, int], drop_isolated: bool = False) -> PaddedSubgraphBatch:
    """:func:`edge_subgraph` into a batch of the fixed shape ``capacity = (N_cap, E_cap)`` (gsat_subgraph_padded): the kept nodes and
    edges first, bit for bit what ``edge_subgraph`` returns, the slack as the padding graph of ``collate_padded``, the counts in
    ``valid`` on the device.  No size is needed from the host and none is read: the call is capturable, and its result goes wherever a
    ``PaddedBatch`` goes (``padded(sub.valid, sub.capacity)``).

    ``data``: a ``Batch`` of ``G`` graphs -- the result has ``G + 1``, graph ``G`` being the padding graph -- or a ``PaddedBatch``, whose
    ``valid`` is honoured: its padding rows and slots are never kept and ``edge_keep`` is not even read there, its own padding graph
    stays the padding graph, ``ragged`` and ``r`` are carried over.  ``x``, ``edge_attr``, ``edge_label``, ``node_label`` and an
    optional ``edge_att`` are gathered with zero rows in the padding; with ``drop_isolated=False`` on a ``PaddedBatch`` of ``N_cap`` rows
    ``x``, ``batch`` and ``node_label`` are the input's own tensors (nothing decides on the host, so also when the extraction overflows:
    see below).

    An extraction that does not fit (``N' + 2 > N_cap`` or ``E' > E_cap``), whose input had overflowed or that met a bad node id is all
    padding with ``valid == (0, 0, 0, 1)``: a ValueError after one host read of ``valid`` -- in sync-free mode or under capture
    nothing is read and ``.check()`` reports it.  The one exception to "all padding": where ``x`` and ``batch`` are the input's own
    tensors they stay what the input holds, real rows and graph ids included; ``valid``, ``edge_index``, ``node_id``, ``edge_id`` and the
    gathered edge attributes are the all-padding ones, and everything that counts by ``valid`` (``padded()``, the logs) sees no row."""
    if not isinstance(edge_keep, torch.Tensor):
        raise ValueError("edge_keep must be a tensor")
    return _extract_padded(data, edge_keep, 0, drop_isolated, capacity)


def node_subgraph_padded(data, node_keep: torch.Tensor, capacity: Tuple[int, int]) -> PaddedSubgraphBatch:
    """:func:`node_subgraph` into a batch of the fixed shape ``capacity``; see :func:`edge_subgraph_padded`.  ``node_keep``: a mask
    [N] (an id list would need its length on the host)."""
    if not isinstance(node_keep, torch.Tensor):
        raise ValueError("node_keep must be a tensor")
    if node_keep.dtype == torch.int64:
        raise ValueError("node_subgraph_padded takes a mask, not an id list")
    return _extract_padded(data, node_keep, 1, False, capacity)


def explanation_subgraph(att, data, k: Optional[int] = None, ratio: Optional[float] = None, complement: bool = False,
                         drop_isolated: bool = True, path: str = "auto", connected: bool = False) -> SubgraphBatch:
    """Every graph's ``k`` (or ``ceil(ratio * E_g)``) highest-attention edges as a batch of their own (``complement``: everything
    BUT those edges); ties as in :mod:`dp_gsat_amd.explain` (lower edge id first).  The kept edges' attention rides along as
    ``edge_att = att[edge_id]``.  ``connected=True``: the mask is replaced by its largest connected component in every graph before the
    extraction (:func:`~dp_gsat_amd.explain.largest_component_mask`: most kept edges, ties to the component with the smaller smallest
    node id) -- the explanation as ONE motif."""
    if (k is None) == (ratio is None):
        raise ValueError("give exactly one of k and ratio")
    a = ops.edge_tensor(att)
    if not isinstance(a, torch.Tensor) or a.numel() != int(data.edge_index.shape[1]):
        raise ValueError(f"attention must have one entry for each of the {int(data.edge_index.shape[1])} edges")
    _need_cuda(a, data.edge_index, data.batch, data.x)
    mask = topk_edge_mask(a, data.edge_index, data.batch, k=k, ratio=ratio, num_graphs=getattr(data, "num_graphs", None), path=path)
    if complement:
        mask = ~mask
    if connected:
        from .explain import largest_component_mask
        mask = largest_component_mask(data.edge_index, data.batch, mask, num_graphs=getattr(data, "num_graphs", None))
    sub = edge_subgraph(data, mask, drop_isolated=drop_isolated)
    sub.edge_att = gather_rows(a.detach(), sub.edge_id)
    return sub


def explanation_fidelity(clf, data, att, k: Optional[int] = None, ratio: Optional[float] = None, drop_isolated: bool = False) -> dict:
    """Fidelity of the top-k explanation for the backbone ``clf``: three forwards WITHOUT ``edge_atten`` (eval mode, no grad) -- the
    full batch, the explanation alone, the batch with the explanation removed -- on compacted graphs, which is what makes the
    numbers right for PNA.  Returns device tensors: ``logits_full / logits_keep / logits_drop [G, C]`` and the scalars
    ``fidelity_plus = mean_g(p_full - p_drop)``, ``fidelity_minus = mean_g(p_full - p_keep)`` with ``p`` the probability of the class
    the full model predicts (one logit: sigmoid and its sign; otherwise softmax and argmax).  The results stay on the device; the
    two extractions read their sizes back once each."""
    was_training = clf.training
    clf.eval()
    try:
        with torch.no_grad():
            keep = explanation_subgraph(att, data, k=k, ratio=ratio, complement=False, drop_isolated=drop_isolated)
            drop = explanation_subgraph(att, data, k=k, ratio=ratio, complement=True, drop_isolated=drop_isolated)
            for sub in (keep, drop):
                if sub.num_nodes == 0:
                    raise ValueError("an extraction kept no node at all: use drop_isolated=False")
            for sub in (keep, drop):           # also for an extraction without edges: the forwards below must return num_graphs rows
                get_index(sub.edge_index, sub.num_nodes).graphs(sub.batch, sub.num_graphs)
            full, lk, ld = (clf(d.x, d.edge_index, d.batch, getattr(d, "edge_attr", None)) for d in (data, keep, drop))
            if full.dim() == 2 and full.shape[1] > 1:
                cls = full.argmax(dim=1, keepdim=True)
                p_full, p_keep, p_drop = (torch.softmax(z, dim=1).gather(1, cls).view(-1) for z in (full, lk, ld))
            else:
                sign = torch.where(full >= 0, 1.0, -1.0)
                p_full, p_keep, p_drop = (torch.sigmoid(sign * z).view(-1) for z in (full, lk, ld))
    finally:
        clf.train(was_training)
    return {"logits_full": full, "logits_keep": lk, "logits_drop": ld,
            "fidelity_plus": (p_full - p_drop).mean(), "fidelity_minus": (p_full - p_keep).mean()}


# ---- fidelity curves: every sparsity level of a batch in one stacked batch ------------------------------------------------------------------
def fidelity_stack_block_items() -> int:
    """Edge slots one workgroup of the stack kernels owns."""
    return int(_lib.load().gsat_fidelity_stack_block_items())


class StackedExplanationBatch(Batch):
    """The result of :func:`explanation_stack`: a plain batch of ``variants * graphs_per_variant`` graphs -- ``x``, ``edge_index``,
    ``batch``, ``edge_attr``, ``num_graphs`` -- plus ``valid`` (int32[variants, 4] on the device: N_real, kept edges, graphs, overflow of
    every variant), ``levels`` (the ``ks`` or ``ratios``) and ``by_ratio``, ``variants`` (``2 * len(levels) + 1``), ``segment_offsets``
    (host ints: variant ``v`` owns the edge slots ``[segment_offsets[v], segment_offsets[v + 1])``), ``node_capacity`` (variant ``v`` owns
    the node rows ``[v * node_capacity, (v + 1) * node_capacity)``), ``graphs_per_variant`` (the padding graph last), ``edge_id``
    (int64[E_stack]: the input's edge slot, -1 for padding) and ``edge_level`` (uint8[E]: :func:`explanation_levels` of the input).
    ``rankings`` is 1; of :func:`explanation_stack_multi` it is ``R``, with ``variants = 1 + 2 R S`` and ``edge_level`` uint8[R, E].
    Of :func:`explanation_stack_nodes` the variants are node-induced: ``valid[v, 0]`` is the variant's own node count, and in place of
    ``edge_level`` the batch carries ``node_id`` (int64[variants * node_capacity]: the input's row, -1 for padding), ``node_level``
    (uint8[N]) and the gathered ``node_label``."""

    def check(self) -> "StackedExplanationBatch":
        """One host read of ``valid``: raises ValueError when a variant overflowed (it is then all padding)."""
        if int(self.valid[:, 3].any()):
            raise ValueError(_overflow_text((self.node_capacity, "its segment")))
        return self


def explanation_stack(data, att, ks=None, ratios=None, batch_size: Optional[int] = None, *, max_seg_edges: Optional[int] = None,
                      edge_level: Optional[torch.Tensor] = None) -> StackedExplanationBatch:
    """Every sparsity level of the explanation ``att`` of ``data`` as ONE batch (gsat_fidelity_stack): with ``S`` levels (``ks`` or
    ``ratios``, as in :func:`~dp_gsat_amd.explain.explanation_levels`) the ``V = 2 S + 1`` variants "the batch itself", "level s alone"
    (``v = 1 + s``) and "the batch without level s" (``v = 1 + S + s``) side by side, so that ONE backbone forward scores a whole fidelity
    curve.  In eval mode the backbone works row by row -- running statistics, no dropout, per-node aggregation, per-graph pools -- so
    the logits of a graph in the stack are those of the graph on its own up to GEMM rounding.

    ``data``: a ``Batch`` of ``G`` graphs (then ``graphs_per_variant = G + 1``, ``node_capacity = N + 2``, ``E_cap = E``) or a
    ``PaddedBatch`` (its own ``num_graphs``, node rows and edge slots).  Every variant keeps every node (``drop_isolated=False``) and
    holds, inside its node rows, graph ids and edge segment, bit for bit what ``edge_subgraph_padded(data, mask_v, (node_capacity,
    cap_v))`` holds, with ``cap_v = E_cap`` for the full and the drop variants and ``keep_capacity(E_cap, batch_size, k_s | ratio_s)`` for
    the keep variants (``batch_size`` defaults to the number of real graph slots).  ``x`` is the input's ``x`` (with two zero rows behind
    an unpadded batch) ``V`` times, ``edge_attr`` is gathered through ``edge_id`` with zero rows in the padding.

    ``max_seg_edges``: the bound that keeps the ranking on the fused path (needed in sync-free mode and under capture); ``edge_level``:
    levels computed before, in place of ``att``.  Five launches (the levels, four for the stack) besides the ranking, the row gathers
    and the stack's batch index, whatever ``S`` is, and nothing read back: capturable.  A
    variant that does not fit, an overflowed input or a bad node id is all padding with ``valid == (0, 0, 0, 1)``: a ValueError after one
    host read of ``valid`` -- in sync-free mode or under capture nothing is read and ``.check()`` reports it."""
    return _explanation_stack(data, [att], ks, ratios, batch_size, max_seg_edges, None if edge_level is None else [edge_level], False)


def explanation_stack_multi(data, atts, ks=None, ratios=None, batch_size: Optional[int] = None, *, max_seg_edges: Optional[int] = None,
                            edge_levels=None) -> StackedExplanationBatch:
    """:func:`explanation_stack` for ``R`` explanations ``atts`` of the same edges around ONE copy of the batch itself
    (gsat_fidelity_stack_multi): ``V = 1 + 2 R S`` variants -- ``v = 0`` the batch, ``v = 1 + r S + s`` "ranking r, level s alone", ``v = 1
    + R S + r S + s`` "the batch without it" -- so that ONE backbone forward scores ``R`` fidelity curves, and a ``FidelityCurveLog(...,
    rankings=R)`` takes its logits as they are.  Every variant of ranking ``r`` holds, bit for bit, what ``explanation_stack(data,
    atts[r], ...)`` holds for it, moved to its new node rows and graph ids; the segment capacities are those of ``explanation_stack``,
    ranking after ranking.  ``atts``: a sequence of ``R`` attentions; ``edge_levels``: in their place, levels computed before -- a
    sequence of ``R`` uint8[E] tensors or one uint8[R, E].  The result has ``rankings = R``, ``variants`` and ``edge_level`` uint8[R, E].
    Still four launches for the stack whatever ``R`` and ``S`` are, nothing read back: capturable with ``max_seg_edges``.  Refused like
    ``explanation_stack``, and when ``R * S`` is above 16."""
    if edge_levels is None:
        if atts is None or isinstance(atts, torch.Tensor) or len(atts) < 1:
            raise ValueError("atts must be a sequence of one or more attentions (one tensor: explanation_stack)")
        atts = list(atts)
    else:
        edge_levels = list(edge_levels) if not isinstance(edge_levels, torch.Tensor) else (
            list(edge_levels) if edge_levels.dim() == 2 else [edge_levels])
        if len(edge_levels) < 1:
            raise ValueError("edge_levels must hold one or more level rows")
        atts = [None] * len(edge_levels)
    return _explanation_stack(data, atts, ks, ratios, batch_size, max_seg_edges, edge_levels, True)


def _explanation_stack(data, atts, ks, ratios, batch_size, max_seg_edges, edge_levels, multi) -> StackedExplanationBatch:
    """The body of :func:`explanation_stack` (``multi`` False: one ranking through gsat_fidelity_stack, ``edge_level`` uint8[E]) and
    :func:`explanation_stack_multi` (gsat_fidelity_stack_multi, ``edge_level`` uint8[R, E])."""
    from .explain import check_levels, check_rankings, explanation_levels
    from .replay import keep_capacity
    ks, ratios = check_levels(ks, ratios)
    levels = ks if ks is not None else ratios
    S, R = len(levels), len(atts)
    if multi:
        check_rankings(R, S)
    V = 2 * R * S + 1
    x, edge_index, batch = data.x, data.edge_index, data.batch
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
    N, E, dev = int(x.shape[0]), int(edge_index.shape[1]), edge_index.device
    if batch.dtype != torch.int64 or batch.dim() != 1 or int(batch.shape[0]) != N:
        raise ValueError("batch must be an int64 vector with one entry per node")
    _need_cuda(x, edge_index, batch, *(edge_levels or ()))
    capturing = torch.cuda.is_current_stream_capturing()
    valid_in = getattr(data, "valid", None)
    if valid_in is not None:
        if valid_in.dtype != torch.int32 or valid_in.numel() < 4 or not valid_in.is_cuda:
            raise ValueError("data.valid must be an int32 ROCm tensor (N_real, E_real, B, overflow)")
        valid_in = valid_in.contiguous()
        Gp = int(data.num_graphs)
        real, N_cap = Gp - 1, N
        if N_cap < 2:
            raise ValueError("a padded batch has at least two node rows (the padding nodes)")
    else:
        real = getattr(data, "num_graphs", None)
        if real is None:
            if sync_free() or capturing:
                raise ValueError("a stack of a batch without num_graphs would read batch.max() back")
            real = int(batch.max().item()) + 1 if N else 0
        real = int(real)
        Gp, N_cap = real + 1, N + 2
    B = real if batch_size is None else int(batch_size)
    ei, batch = edge_index.contiguous(), batch.contiguous()
    rows = []
    for r in range(R):
        if edge_levels is None:
            a = ops.edge_tensor(atts[r])
            if not isinstance(a, torch.Tensor) or a.numel() != E:
                raise ValueError(f"attention must have one entry for each of the {E} edges")
            rows.append(explanation_levels(a, ei, batch, ks=ks, ratios=ratios, num_graphs=Gp if valid_in is not None else real,
                                           max_seg_edges=max_seg_edges, ranked_graphs=real if max_seg_edges is not None else None))
        else:
            lv = edge_levels[r]
            if not isinstance(lv, torch.Tensor) or lv.dtype != torch.uint8 or lv.numel() != E:
                raise ValueError(f"edge_level must be a uint8 tensor with one entry for each of the {E} edges")
            rows.append(lv.reshape(-1).contiguous())
    edge_level = torch.stack(rows) if multi else rows[0]
    keep_caps = [keep_capacity(E, B, **({"k": l} if ks is not None else {"ratio": l})) for l in levels]
    caps = [E] + keep_caps * R + [E] * (R * S)
    offsets = [0]
    for c in caps:
        offsets.append(offsets[-1] + int(c))
    E_stack = offsets[-1]
    ws_bytes = max(call_size("gsat_fidelity_stack_multi_workspace_bytes", E, R, S) if multi
                   else call_size("gsat_fidelity_stack_workspace_bytes", E, S), 256)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    new_ei = torch.empty(2, E_stack, dtype=torch.int64, device=dev)
    edge_id = torch.empty(E_stack, dtype=torch.int64, device=dev)
    new_batch = torch.empty(V * N_cap, dtype=torch.int64, device=dev)
    valid = torch.empty(V, 4, dtype=torch.int32, device=dev)
    some = lambda t: ptr(t) if t is not None and t.numel() else None
    head = (some(ei), E, N, some(batch), real, ptr(valid_in) if valid_in is not None else None, some(edge_level))
    tail = (Gp, N_cap, (ctypes.c_int64 * (V + 1))(*offsets), some(new_ei), some(edge_id), ptr(new_batch), ptr(valid), ptr(ws), ws_bytes,
            stream())
    if multi:
        call("gsat_fidelity_stack_multi", *head, R, S, *tail)
    else:
        call("gsat_fidelity_stack", *head, S, *tail)
    if not (sync_free() or capturing) and int(valid[:, 3].any()):                                   # the one host read
        raise ValueError(_overflow_text((N_cap, tuple(caps))))
    if N_cap != N:
        x = torch.cat([x, x.new_zeros((N_cap - N,) + tuple(x.shape[1:]))])
    edge_attr = getattr(data, "edge_attr", None)
    if isinstance(edge_attr, torch.Tensor):
        _need_cuda(edge_attr)
        if int(edge_attr.shape[0]) != E:
            raise ValueError(f"edge_attr has {edge_attr.shape[0]} rows")
        edge_attr = _take_padded(edge_attr, edge_id)
    stack = StackedExplanationBatch(x=x.repeat((V,) + (1,) * (x.dim() - 1)), edge_index=new_ei, batch=new_batch, edge_attr=edge_attr,
                                    y=getattr(data, "y", None), num_graphs=V * Gp, valid=valid, levels=tuple(levels),
                                    by_ratio=ratios is not None, variants=V, segment_offsets=tuple(offsets), node_capacity=N_cap,
                                    graphs_per_variant=Gp, edge_id=edge_id, edge_level=edge_level, rankings=R)
    # a backbone forward on the stack then returns num_graphs rows and never reads batch.max() back
    get_index(new_ei, V * N_cap).graphs(new_batch, V * Gp)
    return stack


def _stack_curve(clf, make_stack) -> dict:
    """Eval mode, no grad: ``stack = make_stack()``, ONE ``clf`` forward WITHOUT ``edge_atten`` on it, and the scores of
    :func:`explanation_fidelity_curve` as fp64 device tensors, plus ``stack``."""
    was_training = clf.training
    clf.eval()
    try:
        with torch.no_grad():
            stack = make_stack()
            S, V, Gp = len(stack.levels), stack.variants, stack.graphs_per_variant
            logits = clf(stack.x, stack.edge_index, stack.batch, stack.edge_attr).view(V, Gp, -1)
            z = logits.double()
            real = (torch.arange(Gp, device=z.device) < stack.valid[0, 2]).double()          # the padding graph and empty slots count 0
            n = real.sum()
            if z.shape[2] > 1:
                cls = z.argmax(dim=2)
                p = torch.softmax(z, dim=2).gather(2, cls[0].expand(V, Gp).unsqueeze(2)).squeeze(2)
            else:
                cls = (z[:, :, 0] >= 0).long()
                p = torch.sigmoid(torch.where(cls[0] != 0, 1.0, -1.0) * z[:, :, 0])
            mean = lambda t: (t * real).sum(dim=-1) / n
            flips = mean((cls != cls[0]).double())
            kept = stack.valid[:, 1].double()
    finally:
        clf.train(was_training)
    return {"levels": stack.levels, "fidelity_plus": mean(p[0] - p[1 + S:]), "fidelity_minus": mean(p[0] - p[1:1 + S]), "p_full": mean(p[0]),
            "p_keep": mean(p[1:1 + S]), "p_drop": mean(p[1 + S:]), "flip_plus": flips[1 + S:], "flip_minus": flips[1:1 + S],
            "kept_fraction": kept[1:1 + S] / kept[0], "n": n, "logits": logits, "stack": stack}


def explanation_fidelity_curve(clf, data, att, ks=None, ratios=None) -> dict:
    """The fidelity curve of the explanation ``att`` for the backbone ``clf`` over the levels ``ks`` or ``ratios``: eval mode, no grad,
    :func:`explanation_stack`, ONE ``clf`` forward WITHOUT ``edge_atten`` on the stack.  Returns what ``FidelityCurveLog.compute()``
    returns, as fp64 device tensors -- ``fidelity_plus`` / ``fidelity_minus`` / ``p_keep`` / ``p_drop`` / ``flip_plus`` / ``flip_minus`` /
    ``kept_fraction`` of shape [S], ``p_full`` and ``n`` 0-dim -- with ``levels`` and the stacked ``logits [V, graphs_per_variant, C]``."""
    res = _stack_curve(clf, lambda: explanation_stack(data, att, ks=ks, ratios=ratios))
    del res["stack"]
    return res


def explanation_fidelity_curves(clf, data, atts, ks=None, ratios=None, *, batch_size: Optional[int] = None,
                                max_seg_edges: Optional[int] = None) -> dict:
    """:func:`explanation_fidelity_curve` for ``R`` explanations ``atts`` of the same edges at once: eval mode, no grad,
    :func:`explanation_stack_multi`, ONE ``clf`` forward WITHOUT ``edge_atten`` on the ``1 + 2 R S`` variants.  The same dict with a
    leading ranking axis -- ``fidelity_plus`` / ``fidelity_minus`` / ``p_keep`` / ``p_drop`` / ``flip_plus`` / ``flip_minus`` /
    ``kept_fraction`` of shape [R, S], ``p_full`` and ``n`` 0-dim, ``levels``, the stacked ``logits [V, graphs_per_variant, C]`` -- plus,
    for ``R == 2``, ``jaccard`` and ``overlap`` [S]: :func:`~dp_gsat_amd.explain.level_overlap` of the two rankings' levels, as
    ``both / (a + b - both)`` and ``both / min(a, b)`` (0 where the denominator is 0)."""
    from .explain import level_overlap
    was_training = clf.training
    clf.eval()
    try:
        with torch.no_grad():
            stack = explanation_stack_multi(data, atts, ks=ks, ratios=ratios, batch_size=batch_size, max_seg_edges=max_seg_edges)
            R, S, V, Gp = stack.rankings, len(stack.levels), stack.variants, stack.graphs_per_variant
            logits = clf(stack.x, stack.edge_index, stack.batch, stack.edge_attr).view(V, Gp, -1)
            z = logits.double()
            real = (torch.arange(Gp, device=z.device) < stack.valid[0, 2]).double()          # the padding graph and empty slots count 0
            n = real.sum()
            if z.shape[2] > 1:
                cls = z.argmax(dim=2)
                p = torch.softmax(z, dim=2).gather(2, cls[0].expand(V, Gp).unsqueeze(2)).squeeze(2)
            else:
                cls = (z[:, :, 0] >= 0).long()
                p = torch.sigmoid(torch.where(cls[0] != 0, 1.0, -1.0) * z[:, :, 0])
            mean = lambda t: (t * real).sum(dim=-1) / n
            flips = mean((cls != cls[0]).double())
            kept = stack.valid[:, 1].double()
            keep, drop = slice(1, 1 + R * S), slice(1 + R * S, V)
            out = {"levels": stack.levels, "fidelity_plus": mean(p[0] - p[drop]).view(R, S), "fidelity_minus": mean(p[0] - p[keep]).view(R, S),
                   "p_full": mean(p[0]), "p_keep": mean(p[keep]).view(R, S), "p_drop": mean(p[drop]).view(R, S),
                   "flip_plus": flips[drop].view(R, S), "flip_minus": flips[keep].view(R, S), "kept_fraction": (kept[keep] / kept[0]).view(R, S),
                   "n": n, "logits": logits}
            if R == 2:
                c = level_overlap(stack.edge_level[0], stack.edge_level[1], S, valid=getattr(data, "valid", None)).double()
                union, least = c[:, 1] + c[:, 2] - c[:, 0], torch.minimum(c[:, 1], c[:, 2])
                out["jaccard"] = torch.where(union > 0, c[:, 0] / union.clamp(min=1.0), torch.zeros_like(union))
                out["overlap"] = torch.where(least > 0, c[:, 0] / least.clamp(min=1.0), torch.zeros_like(least))
    finally:
        clf.train(was_training)
    return out


# ---- node explanations: top-k node subgraphs, the node-induced stack, its fidelity curve -------------------------------------------------------
def _node_scores(node_att, N: int) -> torch.Tensor:
    a = node_att.node_att if isinstance(node_att, ops.LiftedAttention) else node_att
    if not isinstance(a, torch.Tensor) or a.numel() != N:
        raise ValueError(f"node attention must have one entry for each of the {N} nodes")
    return a


def explanation_node_subgraph(node_att, data, k: Optional[int] = None, ratio: Optional[float] = None, complement: bool = False) -> SubgraphBatch:
    """Every graph's ``k`` (or ``ceil(ratio * N_g)``) highest-attention NODES and the edges among them as a batch of their own
    (``complement``: everything BUT those nodes): :func:`node_subgraph` on :func:`~dp_gsat_amd.explain.topk_node_mask`; ties as in
    :mod:`dp_gsat_amd.explain` (lower node id first).  The kept nodes' attention rides along as ``node_att = node_att[node_id]``."""
    from .explain import topk_node_mask
    if (k is None) == (ratio is None):
        raise ValueError("give exactly one of k and ratio")
    a = _node_scores(node_att, int(data.x.shape[0]))
    _need_cuda(a, data.edge_index, data.batch, data.x)
    mask = topk_node_mask(a, data.batch, k=k, ratio=ratio, num_graphs=getattr(data, "num_graphs", None))
    if complement:
        mask = ~mask
    sub = node_subgraph(data, mask)
    sub.node_att = gather_rows(a.detach().contiguous(), sub.node_id)
    return sub


def explanation_stack_nodes(data, node_att, ks=None, ratios=None, batch_size: Optional[int] = None, *, max_seg_nodes: Optional[int] = None,
                            node_level: Optional[torch.Tensor] = None) -> StackedExplanationBatch:
    """:func:`explanation_stack` for a NODE explanation (gsat_fidelity_stack_nodes): with ``S`` levels the ``V = 2 S + 1`` node-induced
    variants "the batch itself", "the nodes of level s alone" (``v = 1 + s``) and "the batch without them" (``v = 1 + S + s``) side by
    side, so that ONE backbone forward scores a whole node-fidelity curve.  A variant deletes rows -- which is what changes sum / mean
    pools and PNA degrees --, relabels its endpoints and keeps an edge only when both ends survive; it holds, inside its node rows, graph
    ids and edge segment, bit for bit what ``node_subgraph_padded(data, mask_v, (node_capacity, E))`` holds.

    ``data``: a ``Batch`` of ``G`` graphs (``graphs_per_variant = G + 1``, ``node_capacity = N + 2``) or a ``PaddedBatch`` (its own
    ``num_graphs`` and node rows), the node capacity of ``explanation_stack``.  Every variant's edge segment is ``E``: the levels bound
    the kept NODES of a graph, and a node-induced subgraph has no bound below ``E`` that they imply (a top-1 node with self loops keeps
    them all), so ``batch_size`` changes nothing here and is accepted for symmetry only.  ``x`` and ``node_label`` are gathered by
    ``node_id`` and ``edge_attr`` by ``edge_id``, with zero rows in the padding; the result also carries ``node_id`` (int64[V *
    node_capacity], the input's row, -1 for padding) and ``node_level`` (uint8[N]: :func:`~dp_gsat_amd.explain.node_levels` of the input).

    ``max_seg_nodes``: the bound that keeps the ranking on the fused path (needed in sync-free mode and under capture); ``node_level``:
    levels computed before, in place of ``node_att``.  Five launches for the stack whatever ``S`` is, nothing read back: capturable.
    Overflow is per variant; an overflowed input or a bad node id spoils all: a ValueError after one host read of ``valid[:, 3]`` -- in
    sync-free mode or under capture nothing is read and ``.check()`` reports it."""
    from .explain import check_levels, node_levels
    ks, ratios = check_levels(ks, ratios)
    levels = ks if ks is not None else ratios
    S = len(levels)
    V = 2 * S + 1
    x, edge_index, batch = data.x, data.edge_index, data.batch
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
    N, E, dev = int(x.shape[0]), int(edge_index.shape[1]), edge_index.device
    if batch.dtype != torch.int64 or batch.dim() != 1 or int(batch.shape[0]) != N:
        raise ValueError("batch must be an int64 vector with one entry per node")
    _need_cuda(x, edge_index, batch, node_level)
    capturing = torch.cuda.is_current_stream_capturing()
    valid_in = getattr(data, "valid", None)
    if valid_in is not None:
        if valid_in.dtype != torch.int32 or valid_in.numel() < 4 or not valid_in.is_cuda:
            raise ValueError("data.valid must be an int32 ROCm tensor (N_real, E_real, B, overflow)")
        valid_in = valid_in.contiguous()
        Gp = int(data.num_graphs)
        real, N_cap = Gp - 1, N
        if N_cap < 2:
            raise ValueError("a padded batch has at least two node rows (the padding nodes)")
    else:
        real = getattr(data, "num_graphs", None)
        if real is None:
            if sync_free() or capturing:
                raise ValueError("a stack of a batch without num_graphs would read batch.max() back")
            real = int(batch.max().item()) + 1 if N else 0
        real = int(real)
        Gp, N_cap = real + 1, N + 2
    ei, batch = edge_index.contiguous(), batch.contiguous()
    if node_level is None:
        a = _node_scores(node_att, N)
        node_level = node_levels(a, batch, ks=ks, ratios=ratios, num_graphs=Gp if valid_in is not None else real,
                                 max_seg_nodes=max_seg_nodes, ranked_graphs=real if max_seg_nodes is not None else None)
    else:
        if node_level.dtype != torch.uint8 or node_level.numel() != N:
            raise ValueError(f"node_level must be a uint8 tensor with one entry for each of the {N} nodes")
        node_level = node_level.reshape(-1).contiguous()
    offsets = [v * E for v in range(V + 1)]
    E_stack = offsets[-1]
    ws_bytes = max(call_size("gsat_fidelity_stack_nodes_workspace_bytes", N, E, S), 256)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    new_ei = torch.empty(2, E_stack, dtype=torch.int64, device=dev)
    edge_id = torch.empty(E_stack, dtype=torch.int64, device=dev)
    node_id = torch.empty(V * N_cap, dtype=torch.int64, device=dev)
    new_batch = torch.empty(V * N_cap, dtype=torch.int64, device=dev)
    valid = torch.empty(V, 4, dtype=torch.int32, device=dev)
    some = lambda t: ptr(t) if t is not None and t.numel() else None
    call("gsat_fidelity_stack_nodes", some(ei), E, N, some(batch), real, ptr(valid_in) if valid_in is not None else None, some(node_level), S,
         Gp, N_cap, (ctypes.c_int64 * (V + 1))(*offsets), some(new_ei), some(edge_id), ptr(node_id), ptr(new_batch), ptr(valid), ptr(ws),
         ws_bytes, stream())
    if not (sync_free() or capturing) and int(valid[:, 3].any()):                                   # the one host read
        raise ValueError(_overflow_text((N_cap, (E,) * V)))
    gathered = {}
    for name, index, rows in (("edge_attr", edge_id, E), ("node_label", node_id, N)):
        t = getattr(data, name, None)
        if isinstance(t, torch.Tensor):
            _need_cuda(t)
            if int(t.shape[0]) != rows:
                raise ValueError(f"{name} has {t.shape[0]} rows")
            t = _take_padded(t, index)
        gathered[name] = t
    stack = StackedExplanationBatch(x=_take_padded(x, node_id), edge_index=new_ei, batch=new_batch, y=getattr(data, "y", None),
                                    num_graphs=V * Gp, valid=valid, levels=tuple(levels), by_ratio=ratios is not None, variants=V,
                                    segment_offsets=tuple(offsets), node_capacity=N_cap, graphs_per_variant=Gp, edge_id=edge_id,
                                    node_id=node_id, node_level=node_level, rankings=1, **gathered)
    # a backbone forward on the stack then returns num_graphs rows and never reads batch.max() back
    get_index(new_ei, V * N_cap).graphs(new_batch, V * Gp)
    return stack


def explanation_node_fidelity_curve(clf, data, node_att, ks=None, ratios=None) -> dict:
    """:func:`explanation_fidelity_curve` for a NODE explanation: eval mode, no grad, :func:`explanation_stack_nodes`, ONE ``clf`` forward
    WITHOUT ``edge_atten`` on the stack.  The same keys as fp64 device tensors -- ``kept_fraction`` stays the fraction of EDGES a keep
    variant holds -- plus ``kept_node_fraction`` [S] (``valid[1:1 + S, 0] / valid[0, 0]``)."""
    res = _stack_curve(clf, lambda: explanation_stack_nodes(data, node_att, ks=ks, ratios=ratios))
    valid = res.pop("stack").valid
    kept = valid[:, 0].double()
    res["kept_node_fraction"] = kept[1:len(res["levels"]) + 1] / kept[0]
    return res
