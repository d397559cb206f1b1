"""Restatement for the ragged dual/primal tests: the THREE-budget batching rule in numpy, one Python step per graph (the thing
PackedDataset.budget_batches(..., dual=) must not do), and the case the host and the GPU tests share."""
import numpy as np
import torch

from tests import dual_oracle as do
from tests import padded_oracle as po

# do.labelled_graphs(**po.STEP_GRAPHS), 16 slots
PAIR_SLOTS = 16
PAIR_CAPACITY = (320, 620, 1000)                 # (N_cap, E_cap, E_dual_cap)
PAIR_SIZES = [7, 9, 10, 5, 9, 7, 1]              # range(48): the last batch is a single graph
PAIR_CLOSED_BY = ["E", "D", "E", "N", "E", "N"]  # the budget the next graph would have broken: each of the three binds


def pair_sizes(graphs):
    """(node counts, edge counts, dual edge counts) per graph."""
    n, e = po.sizes(graphs)
    return n, e, np.array([d.shape[1] for d in do.dual_edges(graphs)], np.int64)


def budget_batches(node_counts, edge_counts, dual_edge_counts, perm, capacity, max_graphs):
    """(lists of graph ids, the reason every batch but the last was closed): in ``perm``'s order a graph opens a new batch when adding it
    would break nodes + 2 <= N_cap ("N"), edges <= E_cap ("E"), dual_edges <= E_dual_cap ("D") or count <= max_graphs ("S"); the first
    that applies, in this order, is the reason."""
    out, why, cur, n, e, d = [], [], [], 0, 0, 0
    for g in perm:
        gn, ge, gd = int(node_counts[g]), int(edge_counts[g]), int(dual_edge_counts[g])
        if gn + 2 > capacity[0] or ge > capacity[1] or gd > capacity[2]:
            raise ValueError(f"graph {g} fits no batch")
        reason = ("N" if n + gn + 2 > capacity[0] else "E" if e + ge > capacity[1] else "D" if d + gd > capacity[2] else
                  "S" if len(cur) + 1 > max_graphs else None)
        if cur and reason:
            out.append(cur)
            why.append(reason)
            cur, n, e, d = [], 0, 0, 0
        cur.append(int(g))
        n, e, d = n + gn, e + ge, d + gd
    return (out + [cur] if cur else out), why


def host_dual_dataset(graphs, ds):
    """The dual of ``ds`` (a PackedDataset of ``graphs`` on the CPU) built on the host from do.dual_edges: the sizes are all that the
    budget rule reads, so the dual features are left empty."""
    import dp_gsat_amd as G
    de = do.dual_edges(graphs)
    counts = torch.tensor([d.shape[1] for d in de], dtype=torch.int64)
    local = torch.from_numpy(np.concatenate([d.reshape(2, -1) for d in de], axis=1).astype(np.int64))
    return G.PackedDataset(torch.zeros(int(ds.edge_ptr_all[-1]), 1), local, ds.edge_ptr_all,
                           torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]), ds.y_all)
