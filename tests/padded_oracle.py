"""numpy restatement of fixed-capacity collation (PackedDataset.collate_padded / capacity_for) and the graph lists the padded-batch tests
cut from tests/golden/mutag128.npz."""
import os
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTAG128 = os.path.join(ROOT, "tests", "golden", "mutag128.npz")


def mutag_graphs(count, single_node=(), self_loop=()):
    """The first ``count`` graphs of mutag128.npz as a data list (x = one-hot(14) node labels, local edge ids, y [1, 1]).  Graphs listed
    in ``single_node`` are cut down to their first node (no edges); graphs in ``self_loop`` get one extra edge (0 -> 0), which keeps
    their edge set symmetric and makes their edge count odd."""
    z = np.load(MUTAG128)
    ei, batch, lab, y = z["edge_index"].astype(np.int64), z["batch"].astype(np.int64), z["node_label"].astype(np.int64), z["y"]
    start = np.concatenate([[0], np.cumsum(np.bincount(batch))])
    eg = batch[ei[0]]
    out = []
    for g in range(count):
        n = int(start[g + 1] - start[g])
        e = ei[:, eg == g] - start[g]
        labels = lab[start[g]:start[g + 1]]
        if g in single_node:
            n, e, labels = 1, e[:, :0], labels[:1]
        if g in self_loop:
            e = np.concatenate([e, np.zeros((2, 1), np.int64)], axis=1)
        x = torch.zeros(n, 14)
        x[torch.arange(n), torch.from_numpy(labels)] = 1.0
        out.append(NS(x=x, edge_index=torch.from_numpy(np.ascontiguousarray(e)), y=torch.tensor([[float(y[g])]]), edge_attr=None,
                      edge_label=None))
    return out


def sizes(graphs):
    return (np.array([g.x.shape[0] for g in graphs], np.int64), np.array([g.edge_index.shape[1] for g in graphs], np.int64))


def capacity_for(node_counts, edge_counts, batch_size):
    k = min(int(batch_size), len(node_counts))
    return int(np.sort(node_counts)[::-1][:k].sum()) + 2, int(np.sort(edge_counts)[::-1][:k].sum())


def totals(graphs, ids):
    n, e = sizes(graphs)
    return int(n[list(ids)].sum()), int(e[list(ids)].sum())


def collate_padded(graphs, ids, capacity):
    """dict of int64 arrays: batch [N_cap], node_src_row [N_cap], edge_index [2, E_cap], edge_src_slot [E_cap], valid [4]; rows / slots of
    the dataset are numbered as PackedDataset.from_data_list packs them (graphs concatenated in list order)."""
    n_all, e_all = sizes(graphs)
    node_ptr = np.concatenate([[0], np.cumsum(n_all)])
    edge_ptr = np.concatenate([[0], np.cumsum(e_all)])
    N_cap, E_cap = capacity
    B = len(ids)
    N, E = totals(graphs, ids)
    overflow = N + 2 > N_cap or E > E_cap
    batch = np.full(N_cap, B, np.int64)
    node_src = np.full(N_cap, -1, np.int64)
    ei = np.zeros((2, E_cap), np.int64)
    edge_src = np.full(E_cap, -1, np.int64)
    if overflow:
        N = E = 0
    else:
        no = eo = 0
        for k, g in enumerate(ids):
            n, e = int(n_all[g]), int(e_all[g])
            batch[no:no + n] = k
            node_src[no:no + n] = node_ptr[g] + np.arange(n)
            ei[:, eo:eo + e] = graphs[g].edge_index.numpy() + no
            edge_src[eo:eo + e] = edge_ptr[g] + np.arange(e)
            no, eo = no + n, eo + e
    n_pad, e_pad = N_cap - N, E_cap - E
    for j in range(e_pad):
        q = j // 2
        a, b = N + q % n_pad, N + (q + 1) % n_pad
        if j == e_pad - 1 and e_pad % 2 == 1:
            ei[:, E + j] = (a, a)
        else:
            ei[:, E + j] = (a, b) if j % 2 == 0 else (b, a)
    return dict(batch=batch, node_src_row=node_src, edge_index=ei, edge_src_slot=edge_src,
                valid=np.array([N, E, B, int(overflow)], np.int64))


def check_invariants(layout, capacity):
    """What makes the padding inert: a symmetric padding edge multiset among the padding nodes only, at least two padding nodes, and a
    padding in-degree of at most ceil(e_pad / n_pad) + 1."""
    N_cap, E_cap = capacity
    N, E = int(layout["valid"][0]), int(layout["valid"][1])
    n_pad, e_pad = N_cap - N, E_cap - E
    assert n_pad >= 2
    ei = layout["edge_index"]
    real, pad = ei[:, :E], ei[:, E:]
    assert real.size == 0 or (real.min() >= 0 and real.max() < N)
    assert pad.size == 0 or (pad.min() >= N and pad.max() < N_cap)
    fwd = sorted(map(tuple, pad.T.tolist()))
    bwd = sorted(map(tuple, pad[::-1].T.tolist()))
    assert fwd == bwd, "padding edge set is not symmetric"
    if e_pad:
        indeg = np.bincount(pad[1] - N, minlength=n_pad)
        assert indeg.max() <= -(-e_pad // n_pad) + 1
    assert (layout["batch"][N:] == layout["valid"][2]).all() and (layout["node_src_row"][N:] == -1).all()
    assert (layout["edge_src_slot"][E:] == -1).all()
    assert (np.diff(layout["batch"]) >= 0).all()


# ---- the cases of the GPU tests, fixed here so that the host tests can vet them ---------------------------------------------------------
LAYOUT_GRAPHS = dict(count=12, single_node=(11,))
LAYOUT_IDS = [7, 11, 2, 9, 0]                  # not sorted; graph 11 is the one-node graph without edges


def layout_cases():
    """name -> capacity for LAYOUT_IDS: e_pad = 0 with n_pad = 2; odd e_pad; 40 padding edges on 2 padding nodes; 30 padding nodes, 7 edges."""
    N, E = totals(mutag_graphs(**LAYOUT_GRAPHS), LAYOUT_IDS)
    return {"tight": (N + 2, E), "odd_self_loop": (N + 5, E + 9), "duplicated": (N + 2, E + 40), "wide": (N + 30, E + 7)}


STEP_GRAPHS = dict(count=48, self_loop=(5,))   # graph 5 (8 nodes, the smallest) gets an odd edge count
STEP_BATCH = 16
STEP_IDS = [list(range(16, 32)),                                                    # even e_pad
            [47, 3, 5, 40, 12, 9, 30, 31, 32, 18, 24, 13, 8, 20, 37, 38],          # holds graph 5: odd E_real, odd e_pad
            [27, 40, 0, 26, 7, 17, 6, 47, 43, 11, 34, 13, 1, 2, 4, 42]]            # the large graphs
