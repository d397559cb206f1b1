"""Explanation metrics on the device: per-graph edge ranking, precision@k, attention ROC-AUC, delta-KL.

The reference scores the edge attention against ground-truth edge labels after every batch on the host
(src/run_gsat.py:656-668): ``att.data.cpu()``, a Python loop over graphs with two boolean masks over all E edges, a host
``argsort`` and an ``.item()`` per graph (get_precision_at_k, :783-791), sklearn's ``roc_auc_score`` (:763) and get_delta_kl
(:793-800).  Here the same numbers come from HIP kernels (csrc/explain.hip) on the attention where it already lives; nothing is
copied to the host until :meth:`ExplanationMeter.compute`.

Tie rule (the contract of every ranking here): higher attention first, equal attention -> LOWER EDGE ID first, -0.0 == +0.0.  The
reference's ``np.argsort(-att)[:k]`` is an unstable sort, i.e. ambiguous under ties -- and ties are the rule in edge-attention mode,
where the symmetrised mask gives an edge and its reverse the same value.  NaN attention is unsupported.

Node-attention models score nodes: ``rank_nodes`` / ``topk_node_mask`` / ``node_levels`` / ``node_precision_at_k`` run the same kernels on
the node segments of the batch (``node_ptr``, the identity order, the batch vector), with the same rule: lower NODE id first on ties.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib, ops
from ._lib import GsatHipError, call, ptr, stream
from .graph_index import call_size, get_index, sync_free

_PATHS = {"auto": 0, "fused": 1, "general": 2}


class EdgeRanking(NamedTuple):
    """order int32[E]: edge ids graph by graph, best first (``order[edge_ptr[g] + r]`` = rank-r edge of graph g); rank int32[E]:
    position of edge e inside its graph; edge_ptr int32[G+1]."""
    order: torch.Tensor
    rank: torch.Tensor
    edge_ptr: torch.Tensor


def _att(att) -> torch.Tensor:
    att = ops.edge_tensor(att)
    if not isinstance(att, torch.Tensor) or not att.is_cuda:
        raise GsatHipError("dp_gsat_amd.explain needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    if att.dim() > 2 or (att.dim() == 2 and att.shape[1] != 1):
        raise ValueError("attention must have shape [E] or [E, 1]")
    return att.detach().reshape(-1).to(torch.float32).contiguous()


def _labels(exp_labels, E: int) -> torch.Tensor:
    if not isinstance(exp_labels, torch.Tensor) or not exp_labels.is_cuda:
        raise GsatHipError("dp_gsat_amd.explain needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    lab = exp_labels.reshape(-1)
    if lab.shape[0] != E:
        raise ValueError(f"exp_labels has {lab.shape[0]} entries for {E} edges")
    if lab.dtype == torch.uint8:                 # the kernels read "nonzero = labelled" themselves
        return lab.contiguous()
    return lab.contiguous().view(torch.uint8) if lab.dtype == torch.bool else (lab != 0).to(torch.uint8)


def _segments(edge_index, batch, num_graphs):
    if not edge_index.is_cuda or not batch.is_cuda:
        raise GsatHipError("dp_gsat_amd.explain needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    return get_index(edge_index, int(batch.shape[0])).graphs(batch, num_graphs)


def _rank(att, edge_index, batch, num_graphs, path, k=0, label=None, want=("order", "rank"), max_seg_edges=None, ranked_graphs=None):
    """One gsat_rank_edges call; returns (dict of the wanted outputs, GraphSegments).  ``max_seg_edges``: the caller's bound on the
    largest graph, in place of the one the batch index may have to read back -- the fused path is then taken whatever the mode, and a
    bound above ``rank_edges_lds_cap()`` is a ValueError.  ``ranked_graphs`` (with ``max_seg_edges`` only): only the first so many graphs
    are ranked; the entries of the other graphs' edges are not written."""
    if path not in _PATHS:
        raise ValueError(f"path must be one of {sorted(_PATHS)}")
    if ranked_graphs is not None and max_seg_edges is None:
        # the radix path sorts every edge slot and would rank the unranked graphs' edges inside the last ranked graph
        raise ValueError("ranked_graphs is defined on the fused ranking only: give max_seg_edges (a bound on the edges of one graph) with it")
    if max_seg_edges is not None and _PATHS[path] == 2:
        raise ValueError("max_seg_edges declares a bound for the fused ranking: it does not go with path='general'")
    a = _att(att)
    seg = _segments(edge_index, batch, num_graphs)
    E = seg.index.E
    if a.shape[0] != E:
        raise ValueError(f"attention has {a.shape[0]} entries for {E} edges")
    eptr, eorder = seg.edge_segments[:2]
    lab = _labels(label, E) if label is not None else None
    # -1: the largest graph is unknown and not to be read back now -> general path
    out = _rank_segments(a, eptr, eorder, seg.G, seg.max_edges_per_graph, path, k, lab, want, max_seg_edges, "max_seg_edges", ranked_graphs)
    return out, seg


def _rank_segments(a, eptr, eorder, G, max_seg, path, k, lab, want, bound, bound_name, ranked_graphs):
    """The gsat_rank_edges call on generic segments -- the edges of a batch grouped by graph, or its nodes: ``a`` fp32[E] the scores,
    ``eptr`` int32[G + 1] / ``eorder`` int32[E] the items grouped by graph, ``max_seg`` the largest segment (-1: unknown), ``bound`` the
    caller's declared bound (named ``bound_name`` in messages) or None.  Returns the dict of the wanted outputs."""
    E, dev = int(a.shape[0]), a.device
    out = {}
    if "order" in want:
        out["order"] = torch.empty(E, dtype=torch.int32, device=dev)
    if "rank" in want:
        out["rank"] = torch.empty(E, dtype=torch.int32, device=dev)
    if "topk" in want:
        out["topk"] = torch.empty(E, dtype=torch.uint8, device=dev)
    if "hits" in want:
        out["hits"] = torch.empty(G, dtype=torch.int32, device=dev)
    code = _PATHS[path]
    if bound is not None:
        max_seg = int(bound)
        if not 0 <= max_seg <= rank_edges_lds_cap():
            raise ValueError(f"{bound_name} = {max_seg} is outside [0, rank_edges_lds_cap() = {rank_edges_lds_cap()}]: the fused "
                             "ranking cannot take it, and a declared bound never changes the path silently")
        code = 1
    if ranked_graphs is not None:
        if not 0 <= int(ranked_graphs) <= G:
            raise ValueError(f"ranked_graphs = {ranked_graphs} outside [0, {G}]")
        G = int(ranked_graphs)
    fused = code == 1 or (code == 0 and 0 <= max_seg <= rank_edges_lds_cap())
    ws, ws_bytes = None, 0
    if not fused:
        ws_bytes = call_size("gsat_rank_edges_workspace_bytes", E)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    call("gsat_rank_edges", ptr(a) if E else None, ptr(eptr), ptr(eorder) if E else None, ptr(lab) if lab is not None and E else None,
         E, G, int(k), int(max_seg), code, *(ptr(out[n]) if n in out and out[n].numel() else None for n in ("order", "rank", "topk")),
         ptr(out["hits"]) if "hits" in out and G and lab is not None and E else None, ptr(ws), ws_bytes, stream())
    if "hits" in out and (E == 0 or lab is None):
        out["hits"].zero_()
    return out


def rank_edges_lds_cap() -> int:
    """Largest graph (in edges) the fused ranking kernel sorts; larger graphs take the general (radix sort) path."""
    return int(_lib.load().gsat_rank_edges_lds_cap())


def rank_edges(att, edge_index, batch, num_graphs: Optional[int] = None, path: str = "auto") -> EdgeRanking:
    """Every graph's edges in descending attention order (ties: lower edge id first).  ``path``: "auto" (fused kernel when the
    largest graph fits it), "fused" (raises GsatHipError when it does not) or "general"."""
    out, seg = _rank(att, edge_index, batch, num_graphs, path)
    return EdgeRanking(out["order"], out["rank"], seg.edge_segments[0])


def topk_edge_mask(att, edge_index, batch, k: Optional[int] = None, ratio: Optional[float] = None, num_graphs: Optional[int] = None,
                   path: str = "auto", *, max_seg_edges: Optional[int] = None, ranked_graphs: Optional[int] = None) -> torch.Tensor:
    """bool[E]: the ``k`` best edges of every graph, or its ``ceil(ratio * E_g)`` best.

    ``max_seg_edges`` (keyword only): a bound on the edges of one graph that the caller knows, e.g. from its dataset.  The ranking then
    runs the fused one-launch path also in sync-free mode and inside a stream capture, where the batch's own largest graph is unknown;
    a bound above ``rank_edges_lds_cap()`` raises ValueError.  ``ranked_graphs`` (keyword only): rank the first so many graphs only --
    for a padded batch its ``num_graphs - 1``, so that the padding graph is not ranked at all; only the fused path can leave graphs out, so
    it needs ``max_seg_edges`` (ValueError without it, or with ``path="general"``).  The mask's entries at the edges of the
    other graphs are then NOT written (arbitrary bytes): ``edge_subgraph_padded`` never reads them."""
    if (k is None) == (ratio is None):
        raise ValueError("give exactly one of k and ratio")
    bound = dict(max_seg_edges=max_seg_edges, ranked_graphs=ranked_graphs)
    if k is not None:
        out, _ = _rank(att, edge_index, batch, num_graphs, path, k=k, want=("topk",), **bound)
        return out["topk"].bool()
    out, seg = _rank(att, edge_index, batch, num_graphs, path, want=("rank",), **bound)
    eptr, _, eg, _ = seg.edge_segments
    keep = torch.ceil((eptr[1:] - eptr[:-1]).double() * float(ratio)).to(torch.int32)
    return out["rank"] < keep[eg]


MAX_LEVELS = 16


def check_levels(ks=None, ratios=None):
    """The sparsity levels of a fidelity curve as ``(ks, ratios)``, one of them a list and the other None.  ValueError unless exactly one
    is given, with 1 to ``MAX_LEVELS`` strictly increasing entries: positive ints, or floats in (0, 1]."""
    if (ks is None) == (ratios is None):
        raise ValueError("give exactly one of ks and ratios")
    levels = list(ks if ks is not None else ratios)
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f"a fidelity curve takes 1 to {MAX_LEVELS} levels, got {len(levels)}")
    if ks is not None:
        if any(isinstance(k, bool) or int(k) != k or int(k) < 1 for k in levels):
            raise ValueError("ks must be positive ints")
        levels = [int(k) for k in levels]
    else:
        if any(not 0.0 < float(r) <= 1.0 for r in levels):
            raise ValueError("ratios must lie in (0, 1]")
        levels = [float(r) for r in levels]
    if any(b <= a for a, b in zip(levels, levels[1:])):
        raise ValueError("the levels must be strictly increasing")
    return (levels, None) if ks is not None else (None, levels)


def check_rankings(rankings, levels: int) -> int:
    """The number of rankings a multi-ranking stack or log takes with ``levels`` levels each: ValueError unless it is a positive int and
    ``rankings * levels`` is at most ``MAX_LEVELS`` (the stack lays ``1 + 2 * rankings * levels`` variants out)."""
    if isinstance(rankings, bool) or int(rankings) != rankings or int(rankings) < 1:
        raise ValueError("rankings must be a positive int")
    if int(rankings) * int(levels) > MAX_LEVELS:
        raise ValueError(f"rankings * levels must be at most {MAX_LEVELS}, got {int(rankings)} * {int(levels)}")
    return int(rankings)


def level_overlap(level_a, level_b, S: int, valid=None, out=None) -> torch.Tensor:
    """Agreement of two rankings of the same edges (gsat_level_overlap): ADDS into ``out`` int64[S, 3] on the device -- a fresh zeroed
    block when ``out`` is None -- per level ``s`` the counts ``#(a <= s & b <= s)``, ``#(a <= s)``, ``#(b <= s)`` over the edges that
    are in some level at all, and returns it.  ``level_a`` / ``level_b``: uint8[E] from :func:`explanation_levels` with the same ``S``
    levels; ``valid``: the int32[4] word of a padded batch -- entries at or beyond ``valid[1]`` are never loaded.  Integer and exact,
    one launch (two with the zeroing), nothing read back: capturable.  Jaccard = ``c0 / (c1 + c2 - c0)``, overlap coefficient = ``c0 /
    min(c1, c2)``."""
    if isinstance(S, bool) or int(S) != S or not 1 <= int(S) <= MAX_LEVELS:
        raise ValueError(f"level_overlap takes 1 to {MAX_LEVELS} levels")
    S = int(S)
    for t in (level_a, level_b):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise GsatHipError("dp_gsat_amd.explain needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
        if t.dtype != torch.uint8:
            raise ValueError("levels must be uint8 tensors (explanation_levels)")
    a, b = level_a.reshape(-1).contiguous(), level_b.reshape(-1).contiguous()
    E = int(a.shape[0])
    if int(b.shape[0]) != E:
        raise ValueError(f"the two level vectors must have the same length, got {E} and {int(b.shape[0])}")
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype != torch.int32 or valid.numel() < 4 or not valid.is_cuda:
            raise ValueError("valid must be an int32 ROCm tensor (N_real, E_real, B, overflow)")
        valid = valid.contiguous()
    if out is None:
        out = torch.empty((S, 3), dtype=torch.int64, device=a.device)
        call("gsat_level_overlap_reset", ptr(out), S, stream())
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (S, 3) or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int64 ROCm tensor of shape [{S}, 3]")
    call("gsat_level_overlap", ptr(a) if E else None, ptr(b) if E else None, E, S, ptr(valid) if valid is not None else None, ptr(out),
         stream())
    return out


def level_overlap_reset(out: torch.Tensor) -> None:
    """Zero an accumulator of :func:`level_overlap` by a kernel (no memset node, so a captured graph may hold it)."""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or out.dim() != 2 or int(out.shape[1]) != 3 or not out.is_cuda:
        raise ValueError("out must be an int64 ROCm tensor of shape [S, 3]")
    call("gsat_level_overlap_reset", ptr(out), int(out.shape[0]), stream())


# ---- connectivity: components of the kept edges per graph and level (csrc/components.hip) -----------------------------------------------------
class LevelComponents(NamedTuple):
    """out int64[S, 8]: the accumulator; per_graph int32[G, S, 5]: (components, kept, big_edges, touched, big_nodes) per looked-at graph
    and level, -1 rows for a skipped graph, 0 rows for a graph that was not looked at (or None); node_comp int32[N] / edge_big bool[E]
    of the LAST level (or None): the smallest node id of the node's component, -1 for an untouched node or a graph that was not looked
    at; whether the edge lies in its graph's largest component by kept edges."""
    out: torch.Tensor
    per_graph: Optional[torch.Tensor]
    node_comp: Optional[torch.Tensor]
    edge_big: Optional[torch.Tensor]


def components_lds_cap() -> int:
    """Largest graph (in NODES) gsat_level_components takes; there is no path for larger graphs."""
    return int(_lib.load().gsat_level_components_lds_cap())


def components_wave_nodes() -> int:
    """Largest graph (in nodes) one wavefront of gsat_level_components takes; a larger one is the whole workgroup's."""
    return int(_lib.load().gsat_level_components_wave_nodes())


def _check_valid(valid):
    if valid is None:
        return None
    if not isinstance(valid, torch.Tensor) or valid.dtype != torch.int32 or valid.numel() < 4 or not valid.is_cuda:
        raise ValueError("valid must be an int32 ROCm tensor (N_real, E_real, B, overflow)")
    return valid.contiguous()


def level_components(edge_index, batch, level, S: int, *, num_graphs: Optional[int] = None, max_seg_nodes: Optional[int] = None,
                     ranked_graphs: Optional[int] = None, valid=None, out=None, per_graph: bool = False, labels: bool = False):
    """Connected components of every graph's kept edges at every level of a fidelity curve (gsat_level_components): ADDS into ``out``
    int64[S, 8] on the device -- a fresh block zeroed by the reset kernel when ``out`` is None -- per level ``s`` and counted graph
    ``(1, components, kept, big_edges, touched, big_nodes, components == 1, 0)``; ``out[0, 7]`` counts the skipped graphs.  ``level``:
    uint8[E] from :func:`explanation_levels` with the same ``S`` levels; level ``s`` keeps the edges with ``level <= s``.  Direction is
    ignored, a self-loop joins nothing, the touched nodes of a level are the endpoints of its kept edges.

    Returns ``out``, or with ``per_graph`` / ``labels`` a :class:`LevelComponents` that also holds ``per_graph`` int32[G, S, 5] and the
    last level's ``node_comp`` int32[N] and ``edge_big`` bool[E] (ties between equally large components go to the smaller label).

    ``max_seg_nodes`` (keyword only): a bound on the NODES of one graph that the caller knows, e.g. from its dataset; above
    :func:`components_lds_cap` it is a ValueError, and a graph that exceeds a wrong bound is skipped whole (-1 rows, ``out[0, 7]``),
    never cut.  Without it the batch index's largest node count is read back once (cached) -- a ValueError in sync-free mode and under
    capture.  ``ranked_graphs``: look at the first so many graphs only -- for a padded batch its ``num_graphs - 1``, so that the padding
    graph is never touched.  ``valid``: the int32[4] word of a padded batch -- only graphs below ``valid[2]`` count, edges at or beyond
    ``valid[1]`` are never loaded, nothing is added when ``valid[3]`` is set.  One launch (two with the zeroing; the outputs asked for
    are filled first), integer and exact, nothing read back: capturable with ``max_seg_nodes``."""
    if isinstance(S, bool) or int(S) != S or not 1 <= int(S) <= MAX_LEVELS:
        raise ValueError(f"level_components takes 1 to {MAX_LEVELS} levels")
    S = int(S)
    if not isinstance(level, torch.Tensor) or level.dtype != torch.uint8:
        raise ValueError("level must be a uint8 tensor (explanation_levels)")
    if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
    E = int(edge_index.shape[1])
    if level.numel() != E:
        raise ValueError(f"level has {level.numel()} entries for {E} edges")
    if max_seg_nodes is not None:
        if isinstance(max_seg_nodes, bool) or int(max_seg_nodes) != max_seg_nodes or not 0 <= int(max_seg_nodes) <= components_lds_cap():
            raise ValueError(f"max_seg_nodes = {max_seg_nodes} is outside [0, components_lds_cap() = {components_lds_cap()}]: the "
                             "components kernel cannot take it, and a declared bound never changes behaviour silently")
        max_seg_nodes = int(max_seg_nodes)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (S, 8)
                            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int64 ROCm tensor of shape [{S}, 8]")
    for t in (edge_index, batch, level) + ((out,) if out is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise GsatHipError("dp_gsat_amd.explain needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    valid = _check_valid(valid)
    if max_seg_nodes is None and (sync_free() or torch.cuda.is_current_stream_capturing()):
        raise ValueError("level_components without max_seg_nodes would read the batch's largest node count back: give the bound in "
                         "sync-free mode and under capture")
    seg = _segments(edge_index, batch, num_graphs)
    G, N, dev = seg.G, seg.index.N, edge_index.device
    if max_seg_nodes is None:
        max_seg_nodes = seg.max_nodes_per_graph
        if max_seg_nodes > components_lds_cap():
            raise ValueError(f"the batch's largest graph has {max_seg_nodes} nodes, above components_lds_cap() = {components_lds_cap()}")
    if ranked_graphs is not None:
        if isinstance(ranked_graphs, bool) or not 0 <= int(ranked_graphs) <= G:
            raise ValueError(f"ranked_graphs = {ranked_graphs} outside [0, {G}]")
        G = int(ranked_graphs)
    eptr, eorder = seg.edge_segments[:2]
    lv = level.reshape(-1).contiguous()
    fresh = out is None
    if fresh:
        out = torch.empty((S, 8), dtype=torch.int64, device=dev)
        call("gsat_level_components_reset", ptr(out), S, stream())
    pg = torch.zeros((G, S, 5), dtype=torch.int32, device=dev) if per_graph else None
    node_comp = torch.full((N,), -1, dtype=torch.int32, device=dev) if labels else None
    edge_big = torch.zeros(E, dtype=torch.uint8, device=dev) if labels else None
    some = lambda t: ptr(t) if t is not None and t.numel() else None
    call("gsat_level_components", some(seg.index.edge_index), E, N, ptr(seg.node_ptr), ptr(eptr), some(eorder), G, some(lv), S,
         max_seg_nodes, ptr(valid) if valid is not None else None, some(pg), ptr(out), some(node_comp), some(edge_big), stream())
    if not (per_graph or labels):
        return out
    return LevelComponents(out, pg, node_comp, edge_big.bool() if labels else None)


def level_components_reset(out: torch.Tensor) -> None:
    """Zero an accumulator of :func:`level_components` by a kernel (no memset node, so a captured graph may hold it)."""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or out.dim() != 2 or int(out.shape[1]) != 8 or not out.is_cuda \
            or not out.is_contiguous():
        raise ValueError("out must be a contiguous int64 ROCm tensor of shape [S, 8]")
    call("gsat_level_components_reset", ptr(out), int(out.shape[0]), stream())


def _mask_level(edge_mask, E: int) -> torch.Tensor:
    """uint8[E] levels of a one-level curve whose level 0 keeps the edges of ``edge_mask``: 0 where it is set, 1 elsewhere."""
    if not isinstance(edge_mask, torch.Tensor) or edge_mask.dtype not in (torch.bool, torch.uint8) or edge_mask.numel() != E:
        raise ValueError(f"edge_mask must be a bool or uint8 tensor with one entry for each of the {E} edges")
    if not edge_mask.is_cuda:
        raise GsatHipError("dp_gsat_amd.explain needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    return (edge_mask.reshape(-1) == 0).to(torch.uint8)


def largest_component_mask(edge_index, batch, edge_mask, *, num_graphs: Optional[int] = None, max_seg_nodes: Optional[int] = None,
                           ranked_graphs: Optional[int] = None, valid=None) -> torch.Tensor:
    """bool[E]: the edges of ``edge_mask`` that lie in their graph's largest connected component by kept edges (ties: the component with
    the smaller smallest node id) -- :func:`level_components` with one level.  False at the edges of graphs that are not looked at or
    are skipped.  The keywords are those of :func:`level_components`."""
    lv = _mask_level(edge_mask, int(edge_index.shape[1]))
    return level_components(edge_index, batch, lv, 1, num_graphs=num_graphs, max_seg_nodes=max_seg_nodes, ranked_graphs=ranked_graphs,
                            valid=valid, labels=True).edge_big


def component_labels(edge_index, batch, edge_mask, *, num_graphs: Optional[int] = None, max_seg_nodes: Optional[int] = None,
                     ranked_graphs: Optional[int] = None, valid=None) -> torch.Tensor:
    """int32[N]: for every node the smallest node id (batch-global) of its connected component under the edges of ``edge_mask``, -1 for
    a node no kept edge touches (and for graphs that are not looked at or are skipped).  The keywords are those of
    :func:`level_components`."""
    lv = _mask_level(edge_mask, int(edge_index.shape[1]))
    return level_components(edge_index, batch, lv, 1, num_graphs=num_graphs, max_seg_nodes=max_seg_nodes, ranked_graphs=ranked_graphs,
                            valid=valid, labels=True).node_comp


CONNECTIVITY_KEYS = ("components", "largest_edge_share", "largest_node_share", "connected_fraction")


def connectivity_scores(counts) -> dict:
    """The host side of a :func:`level_components` accumulator read back as nested lists ``[S][8]``: lists over the levels --
    ``components`` (mean per graph), ``largest_edge_share`` (sum of big_edges / sum of kept), ``largest_node_share`` (sum of big_nodes /
    sum of touched), ``connected_fraction`` (graphs with exactly one component / graphs) -- 0.0 where a denominator is 0, and ``n``,
    the graphs counted."""
    ratio = lambda a, b: a / b if b else 0.0
    return {"components": [ratio(c[1], c[0]) for c in counts], "largest_edge_share": [ratio(c[3], c[2]) for c in counts],
            "largest_node_share": [ratio(c[5], c[4]) for c in counts], "connected_fraction": [ratio(c[6], c[0]) for c in counts],
            "n": int(counts[0][0])}


def explanation_connectivity(data, att, ks=None, ratios=None) -> dict:
    """How connected the explanation ``att`` of the batch ``data`` is at the sparsity levels ``ks`` or ``ratios``: one ranking,
    :func:`explanation_levels`, one :func:`level_components` launch and ONE host read of its 8 S counts (besides the batch index's
    cached read of its largest graph, which the eager ranking makes anyway).  Returns :func:`connectivity_scores` -- ``components``,
    ``largest_edge_share``, ``largest_node_share``, ``connected_fraction`` as lists over the levels, ``n`` -- and ``levels``.  ``data``: a
    ``Batch``, or a ``PaddedBatch`` (its padding graph and empty slots count nothing).  For the baseline of the ground truth itself, pass
    ``edge_label`` as ``att`` (its labelled edges rank first), or the label mask to :func:`level_components` as a one-level curve."""
    ks, ratios = check_levels(ks, ratios)
    S = len(ks if ks is not None else ratios)
    G = getattr(data, "num_graphs", None)
    valid = getattr(data, "valid", None)
    seg = _segments(data.edge_index, data.batch, G)
    seg.largest_graph()                                    # both maxima in one read: the ranking's bound and the components'
    level = explanation_levels(att, data.edge_index, data.batch, ks=ks, ratios=ratios, num_graphs=G)
    out = level_components(data.edge_index, data.batch, level, S, num_graphs=G, valid=valid,
                           ranked_graphs=seg.G - 1 if valid is not None else None)
    res = connectivity_scores(out.tolist())               # the one host read
    res["levels"] = list(ks if ks is not None else ratios)
    return res


def explanation_levels(att, edge_index, batch, ks=None, ratios=None, num_graphs: Optional[int] = None, *,
                       max_seg_edges: Optional[int] = None, ranked_graphs: Optional[int] = None) -> torch.Tensor:
    """uint8[E]: for every edge the smallest level ``s`` whose top-``ks[s]`` (or top-``ceil(ratios[s] * E_g)``) of its graph holds it,
    ``len(levels)`` when none does -- all levels of a fidelity curve from ONE ranking, since their kept sets are nested:
    ``explanation_levels(...) <= s`` is bit for bit ``topk_edge_mask(..., k=ks[s] | ratio=ratios[s])``.  ``ks`` / ``ratios``: exactly
    one, 1 to 16 strictly increasing entries.  ``max_seg_edges`` / ``ranked_graphs`` as in :func:`topk_edge_mask`; an edge of a graph that
    is not ranked gets ``len(levels)``.  Two launches (the ranking and gsat_fidelity_levels), capturable with ``max_seg_edges``."""
    ks, ratios = check_levels(ks, ratios)
    S = len(ks if ks is not None else ratios)
    out, seg = _rank(att, edge_index, batch, num_graphs, "auto", want=("rank",), max_seg_edges=max_seg_edges, ranked_graphs=ranked_graphs)
    eptr, _, _, eg32 = seg.edge_segments
    E = seg.index.E
    level = torch.empty(E, dtype=torch.uint8, device=out["rank"].device)
    host_ks = (ctypes.c_int64 * S)(*ks) if ks is not None else None
    host_ratios = (ctypes.c_double * S)(*ratios) if ratios is not None else None
    call("gsat_fidelity_levels", ptr(out["rank"]) if E else None, ptr(eptr), ptr(eg32) if E else None, E,
         seg.G if ranked_graphs is None else int(ranked_graphs), host_ks, host_ratios, S, ptr(level) if E else None, stream())
    return level


def precision_at_k(att, exp_labels, k: int, batch, edge_index, num_graphs: Optional[int] = None, path: str = "auto") -> torch.Tensor:
    """float32[G] on the device: labelled edges among each graph's ``k`` best, divided by ``k`` -- also for a graph with fewer
    than ``k`` edges (src/run_gsat.py:790).  Argument order of the reference's get_precision_at_k."""
    if int(k) <= 0:
        raise ValueError("k must be positive")
    out, _ = _rank(att, edge_index, batch, num_graphs, path, k=k, label=exp_labels, want=("hits",))
    # int / k correctly rounded to fp32: a float32 tensor divided by a Python scalar is a multiplication by the rounded reciprocal
    # on the device (15 / 100 -> 0.14999999), so the quotient is formed in fp64 and rounded once
    return (out["hits"].to(torch.float64) / float(k)).to(torch.float32)


# ---- the same ranking over NODES: node-attention models score atoms, superpixels, words ---------------------------------------------------------
class NodeRanking(NamedTuple):
    """order int32[N]: node ids graph by graph, best first (``order[node_ptr[g] + r]`` = rank-r node of graph g); rank int32[N]:
    position of node i inside its graph; node_ptr int32[G+1]."""
    order: torch.Tensor
    rank: torch.Tensor
    node_ptr: torch.Tensor


def _node_att(att) -> torch.Tensor:
    """fp32[N] of a node attention given as [N], [N, 1] or a ``LiftedAttention`` (its ``node_att``, not the lifted product)."""
    if isinstance(att, ops.LiftedAttention):
        att = att.node_att
    if not isinstance(att, torch.Tensor) or not att.is_cuda:
        raise GsatHipError("dp_gsat_amd.explain needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    if att.dim() > 2 or (att.dim() == 2 and att.shape[1] != 1):
        raise ValueError("node attention must have shape [N] or [N, 1]")
    return att.detach().reshape(-1).to(torch.float32).contiguous()


def _node_segments(batch, num_graphs):
    """(node_ptr int32[G + 1], node_graph int32[N], G) of a ``batch`` vector: the segments a batch index has registered for this very
    tensor (every model forward registers its batch, so a captured body finds them), else one gsat_segment_ptr32 launch."""
    from .graph_index import _CACHE
    if not isinstance(batch, torch.Tensor) or not batch.is_cuda:
        raise GsatHipError("dp_gsat_amd.explain needs ROCm (cuda) tensors: the HIP path has no CPU fallback")
    if batch.dtype != torch.int64 or batch.dim() != 1:
        raise ValueError("batch must be an int64 vector")
    from .graph_index import tensor_version
    version = tensor_version(batch)
    key = (batch.data_ptr(), version, int(batch.shape[0]))
    for ix in (_CACHE.values() if version is not None else ()):
        seg = ix._graphs.get(key)
        if seg is not None and (num_graphs is None or seg.G == int(num_graphs)):
            return seg.node_ptr, seg.node_seg32, seg.G
    n = int(batch.shape[0])
    if num_graphs is None:
        if sync_free() or torch.cuda.is_current_stream_capturing():
            raise ValueError("a node ranking of a batch without num_graphs would read batch.max() back")
        num_graphs = int(batch.max().item()) + 1 if n else 0
    G, b = int(num_graphs), batch.contiguous()
    node_ptr = torch.empty(G + 1, dtype=torch.int32, device=b.device)
    node_graph = torch.empty(max(n, 1), dtype=torch.int32, device=b.device)[:n]
    flags = torch.zeros(1, dtype=torch.int32, device=b.device)
    call("gsat_segment_ptr32", ptr(b), n, G, ptr(node_ptr), ptr(node_graph), ptr(flags), stream())
    return node_ptr, node_graph, G


def _rank_n(node_att, batch, num_graphs, path, k=0, label=None, want=("order", "rank"), max_seg_nodes=None, ranked_graphs=None):
    """:func:`_rank` on the node segments of the batch: ``node_ptr`` as the pointer array, the identity as the order (the nodes of a
    collated batch are grouped by graph).  Returns (dict of the wanted outputs, node_ptr, node_graph int32[N], G)."""
    if path not in _PATHS:
        raise ValueError(f"path must be one of {sorted(_PATHS)}")
    if ranked_graphs is not None and max_seg_nodes is None:
        raise ValueError("ranked_graphs is defined on the fused ranking only: give max_seg_nodes (a bound on the nodes of one graph) with it")
    if max_seg_nodes is not None and _PATHS[path] == 2:
        raise ValueError("max_seg_nodes declares a bound for the fused ranking: it does not go with path='general'")
    a = _node_att(node_att)
    N = int(a.shape[0])
    if int(batch.shape[0]) != N:
        raise ValueError(f"node attention has {N} entries for {int(batch.shape[0])} nodes")
    node_ptr, node_graph, G = _node_segments(batch, num_graphs)
    max_seg = -1                                           # unknown and not to be read back now -> general path
    if max_seg_nodes is None and not (sync_free() or torch.cuda.is_current_stream_capturing()):
        max_seg = int((node_ptr[1:] - node_ptr[:-1]).max().item()) if G > 0 else 0
    order = torch.arange(N, dtype=torch.int32, device=a.device)
    lab = _labels(label, N) if label is not None else None
    out = _rank_segments(a, node_ptr, order, G, max_seg, path, k, lab, want, max_seg_nodes, "max_seg_nodes", ranked_graphs)
    return out, node_ptr, node_graph, G


def rank_nodes(node_att, batch, num_graphs: Optional[int] = None, path: str = "auto") -> NodeRanking:
    """Every graph's nodes in descending attention order -- the total order of :func:`rank_edges`: higher score first, equal score ->
    lower node id first, -0.0 == +0.0.  ``node_att``: [N], [N, 1] or a ``LiftedAttention`` (its ``node_att``); ``path`` as in
    :func:`rank_edges`, the largest graph counted in nodes."""
    out, node_ptr, _, _ = _rank_n(node_att, batch, num_graphs, path)
    return NodeRanking(out["order"], out["rank"], node_ptr)


def topk_node_mask(node_att, batch, k: Optional[int] = None, ratio: Optional[float] = None, num_graphs: Optional[int] = None,
                   path: str = "auto", *, max_seg_nodes: Optional[int] = None, ranked_graphs: Optional[int] = None) -> torch.Tensor:
    """bool[N]: the ``k`` best nodes of every graph, or its ``ceil(ratio * N_g)`` best.  ``max_seg_nodes`` / ``ranked_graphs`` (keyword
    only) mean for nodes what ``max_seg_edges`` / ``ranked_graphs`` mean in :func:`topk_edge_mask`: a declared bound on the nodes of one
    graph forces the fused one-launch ranking, also in sync-free mode and under capture (ValueError above ``rank_edges_lds_cap()``), and
    with ``ranked_graphs`` the rows of the other graphs -- the padding graph of a padded batch -- are NOT written."""
    if (k is None) == (ratio is None):
        raise ValueError("give exactly one of k and ratio")
    bound = dict(max_seg_nodes=max_seg_nodes, ranked_graphs=ranked_graphs)
    if k is not None:
        out = _rank_n(node_att, batch, num_graphs, path, k=k, want=("topk",), **bound)[0]
        return out["topk"].bool()
    out, node_ptr, node_graph, _ = _rank_n(node_att, batch, num_graphs, path, want=("rank",), **bound)
    keep = torch.ceil((node_ptr[1:] - node_ptr[:-1]).double() * float(ratio)).to(torch.int32)
    return out["rank"] < keep[node_graph.long()]


def node_levels(node_att, batch, ks=None, ratios=None, num_graphs: Optional[int] = None, *, max_seg_nodes: Optional[int] = None,
                ranked_graphs: Optional[int] = None) -> torch.Tensor:
    """uint8[N]: :func:`explanation_levels` over nodes -- for every node the smallest level ``s`` whose top-``ks[s]`` (or
    top-``ceil(ratios[s] * N_g)``) of its graph holds it, ``len(levels)`` when none does, from ONE ranking: ``node_levels(...) <= s`` is
    bit for bit ``topk_node_mask(..., k=ks[s] | ratio=ratios[s])``.  A node of a graph that is not ranked gets ``len(levels)``.  Two
    launches besides the identity order (the ranking and gsat_fidelity_levels), capturable with ``max_seg_nodes``."""
    ks, ratios = check_levels(ks, ratios)
    S = len(ks if ks is not None else ratios)
    out, node_ptr, node_graph, G = _rank_n(node_att, batch, num_graphs, "auto", want=("rank",), max_seg_nodes=max_seg_nodes,
                                           ranked_graphs=ranked_graphs)
    N = int(out["rank"].shape[0])
    level = torch.empty(N, dtype=torch.uint8, device=out["rank"].device)
    host_ks = (ctypes.c_int64 * S)(*ks) if ks is not None else None
    host_ratios = (ctypes.c_double * S)(*ratios) if ratios is not None else None
    call("gsat_fidelity_levels", ptr(out["rank"]) if N else None, ptr(node_ptr), ptr(node_graph) if N else None, N,
         G if ranked_graphs is None else int(ranked_graphs), host_ks, host_ratios, S, ptr(level) if N else None, stream())
    return level


def node_precision_at_k(node_att, node_label, k: int, batch, num_graphs: Optional[int] = None) -> torch.Tensor:
    """float32[G] on the device: labelled nodes among each graph's ``k`` best, divided by ``k`` -- also for a graph with fewer than ``k``
    nodes; the quotient is formed in fp64 and rounded once, like :func:`precision_at_k`."""
    if int(k) <= 0:
        raise ValueError("k must be positive")
    out = _rank_n(node_att, batch, num_graphs, "auto", k=k, label=node_label, want=("hits",))[0]
    return (out["hits"].to(torch.float64) / float(k)).to(torch.float32)


def attention_auroc_counts(att, exp_labels) -> torch.Tensor:
    """int64[3] on the device: (U2, P, Nn) with P / Nn the numbers of labelled / unlabelled edges and
    U2 = sum over labelled edges of (2 * unlabelled edges with lower attention + unlabelled edges with equal attention);
    ROC-AUC = U2 / (2 P Nn).  Integer arithmetic: bitwise repeatable."""
    a = _att(att)
    E = a.shape[0]
    lab = _labels(exp_labels, E)
    out = torch.empty(3, dtype=torch.int64, device=a.device)
    ws_bytes = call_size("gsat_auroc_workspace_bytes", E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
    call("gsat_auroc", ptr(a) if E else None, ptr(lab) if E else None, E, ptr(out), ptr(ws), ws_bytes, stream())
    return out


def attention_auroc(att, exp_labels) -> torch.Tensor:
    """Exact tie-aware ROC-AUC of the attention against binary edge labels: a 0-dim float64 device tensor; 0.0 when only one
    class is present (src/run_gsat.py:761-763).  It scores any vector against labels of the same length: for a node-attention model,
    ``attention_auroc(node_att, node_label)`` with the [N] or [N, 1] node attention (of a ``LiftedAttention`` its ``.node_att`` -- the
    object itself stands for the lifted [E, 1] product)."""
    c = attention_auroc_counts(att, exp_labels)
    den = 2 * c[1] * c[2]
    return torch.where(den > 0, c[0].double() / den.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=c.device))


def delta_kl_stats(att, exp_labels, eps: float = 1e-6) -> torch.Tensor:
    """float32[3] on the device: (delta_kl, mean attention of labelled edges, mean attention of unlabelled edges); the mean of an
    empty class is 0."""
    a = _att(att)
    E = a.shape[0]
    lab = _labels(exp_labels, E)
    out = torch.empty(3, dtype=torch.float32, device=a.device)
    ws_bytes = call_size("gsat_delta_kl_workspace_bytes", E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
    call("gsat_delta_kl", ptr(a) if E else None, ptr(lab) if E else None, E, float(eps), ptr(out), ptr(ws), ws_bytes, stream())
    return out


def delta_kl(att, exp_labels, eps: float = 1e-6) -> torch.Tensor:
    """The reference's get_delta_kl (src/run_gsat.py:793-800) as a 0-dim float32 device tensor."""
    return delta_kl_stats(att, exp_labels, eps)[0]


class ExplanationMeter:
    """Device twin of the accumulation in dual_run_one_epoch (src/run_gsat.py:646-678).  ``update`` launches kernels and keeps device
    copies, never syncing (given ``data.num_graphs``); ``compute`` scores everything seen -- one global ROC-AUC, the mean of the per-graph precisions, the mean of
    the per-batch delta_kl, the mean attention of labelled / unlabelled edges -- with ONE host read at the very end."""

    def __init__(self, k: int):
        if int(k) <= 0:
            raise ValueError("k must be positive")
        self.k = int(k)
        self.reset()

    def reset(self):
        self._att, self._lab, self._prec, self._dkl = [], [], [], []

    def update(self, att, data) -> None:
        """``data``: a collated batch with ``edge_index``, ``batch``, ``edge_label`` and ``num_graphs``.  Without ``num_graphs`` the graph
        count is read back from ``batch.max()`` once per batch -- the only sync ``update`` can cause."""
        a = _att(att)
        lab = _labels(data.edge_label, a.shape[0])
        self._prec.append(precision_at_k(a, lab, self.k, data.batch, data.edge_index, getattr(data, "num_graphs", None)))
        self._dkl.append(delta_kl(a, lab))
        self._att.append(a.clone())
        self._lab.append(lab.clone())            # like the attention: the caller may refill its (static) buffers between batches

    def compute(self) -> dict:
        if not self._att:
            raise ValueError("ExplanationMeter.compute() before any update()")
        a, lab = torch.cat(self._att), torch.cat(self._lab)
        means = delta_kl_stats(a, lab)[1:].double()
        vals = torch.cat([attention_auroc(a, lab).view(1), torch.cat(self._prec).double().mean().view(1),
                          torch.stack(self._dkl).double().mean().view(1), means]).tolist()          # the one host read
        return {"att_auroc": vals[0], f"precision@{self.k}": vals[1], "delta_kl": vals[2],
                "avg_signal_att_weights": vals[3], "avg_bkg_att_weights": vals[4]}
