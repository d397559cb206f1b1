"""degree, is_undirected, sort_edge_index (torch_geometric.utils 2.0.3, documented behaviour); the rest: placeholders."""
import torch

from _placeholder import make as _make


def _num_nodes(index, num_nodes):
    if num_nodes is not None:
        return int(num_nodes)
    return int(index.max()) + 1 if index.numel() > 0 else 0


def degree(index, num_nodes=None, dtype=None):
    """How often every id occurs in ``index`` (unweighted)."""
    n = _num_nodes(index, num_nodes)
    out = torch.zeros(n, dtype=dtype, device=index.device)
    return out.scatter_add_(0, index, torch.ones(index.size(0), dtype=out.dtype, device=index.device))


def sort_edge_index(edge_index, edge_attr=None, num_nodes=None):
    """Row-major sort of the edges; 2.0.3 always returns the pair (edge_index, edge_attr or None)."""
    n = _num_nodes(edge_index, num_nodes)
    perm = (edge_index[0] * n + edge_index[1]).argsort()
    return edge_index[:, perm], (None if edge_attr is None else edge_attr[perm])


def is_undirected(edge_index, edge_attr=None, num_nodes=None):
    """True iff the multiset of edges equals the multiset of reversed edges (and their attributes agree)."""
    pairs = list(zip(edge_index[0].tolist(), edge_index[1].tolist()))
    if edge_attr is None:
        return sorted(pairs) == sorted((b, a) for a, b in pairs)
    attr = [tuple(torch.as_tensor(v).reshape(-1).tolist()) for v in edge_attr]
    return sorted(zip(pairs, attr)) == sorted(((b, a), v) for (a, b), v in zip(pairs, attr))


to_networkx = _make("to_networkx")
subgraph = _make("subgraph")
dense_to_sparse = _make("dense_to_sparse")
from _placeholder import module_getattr as __getattr__  # noqa: E402,F401  (any other name: an inert placeholder)
