"""CPU oracle of dp_gsat_amd.explain (numpy / scipy): the ranking contract, the reference's precision@k loop, midrank AUROC, delta-KL."""
import numpy as np
import torch
from scipy.stats import rankdata

from dp_gsat_amd.synth import Batch


def canon(att):
    """fp32 attention with -0.0 folded into +0.0 (the contract's only canonicalisation)."""
    return np.asarray(att, dtype=np.float32).reshape(-1) + np.float32(0.0)


def rank_oracle(att, edge_index, batch, G, k, labels=None):
    """order, rank, topk, hits, edge_ptr: per graph (edges keyed on batch[edge_index[0]], ascending edge id) the stable
    ``np.argsort(-a, kind="stable")`` -- higher attention first, ties by lower edge id."""
    a = canon(att)
    ei, b = np.asarray(edge_index), np.asarray(batch)
    E = ei.shape[1]
    eg = b[ei[0]] if E else np.zeros(0, dtype=np.int64)
    grouped = np.argsort(eg, kind="stable")
    counts = np.bincount(eg, minlength=G) if E else np.zeros(G, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    order = np.empty(E, dtype=np.int32)
    rank = np.empty(E, dtype=np.int32)
    hits = np.zeros(G, dtype=np.int32)
    lab = (np.asarray(labels).reshape(-1) != 0) if labels is not None else None
    for g in range(G):
        ids = grouped[ptr[g]:ptr[g + 1]]
        o = ids[np.argsort(-a[ids], kind="stable")]
        order[ptr[g]:ptr[g + 1]] = o
        rank[o] = np.arange(len(o), dtype=np.int32)
        if lab is not None:
            hits[g] = int(lab[o[:k]].sum())
    return order, rank, (rank < k).astype(np.uint8), hits, ptr


def precision_at_k_reference_loop(att, exp_labels, k, batch, edge_index):
    """The host loop of get_precision_at_k (src/run_gsat.py:783-791) restated on numpy arrays with the stable sort: for every graph,
    the edges with BOTH endpoints in it, their k highest-attention entries, labelled ones counted and divided by k (also when the
    graph has fewer than k edges).  fp32 like the device result (both are int / k)."""
    a, lab = canon(att), np.asarray(exp_labels).reshape(-1) != 0
    b, ei = np.asarray(batch), np.asarray(edge_index)
    G = int(b.max()) + 1
    out = np.empty(G, dtype=np.float32)
    for g in range(G):
        in_g = b == g
        mine = in_g[ei[0]] & in_g[ei[1]]
        best = np.argsort(-a[mine], kind="stable")[:k]
        out[g] = np.float32(lab[mine][best].sum()) / np.float32(k)
    return out


def topk_ratio_oracle(att, edge_index, batch, G, ratio):
    """bool[E]: rank < ceil(ratio * E_g), the ceiling of the fp64 product (what the module documents)."""
    _, rank, _, _, ptr = rank_oracle(att, edge_index, batch, G, 0)
    keep = np.ceil(np.diff(ptr).astype(np.float64) * float(ratio)).astype(np.int64)
    ei, b = np.asarray(edge_index), np.asarray(batch)
    return rank < keep[b[ei[0]]] if ei.shape[1] else np.zeros(0, dtype=bool)


def auroc_counts_oracle(att, labels):
    """(U2, P, Nn) as Python ints from scipy midranks: 2 * midrank is an integer, U2 = sum over positives of 2 * midrank - P (P + 1)."""
    a = canon(att)
    pos = np.asarray(labels).reshape(-1) != 0
    P, Nn = int(pos.sum()), int((~pos).sum())
    if a.size == 0:
        return 0, 0, 0
    r2 = np.rint(2.0 * rankdata(a.astype(np.float64), method="average")).astype(np.int64)
    return int(r2[pos].sum()) - P * (P + 1), P, Nn


def auroc_oracle(att, labels):
    U2, P, Nn = auroc_counts_oracle(att, labels)
    return U2 / (2 * P * Nn) if P * Nn else 0.0


def delta_kl_oracle(att, labels, eps=1e-6):
    """(delta_kl, mean labelled attention, mean unlabelled attention) in fp64 (src/run_gsat.py:793-800, 773-774)."""
    a = np.asarray(att, dtype=np.float32).reshape(-1).astype(np.float64)
    pos = np.asarray(labels).reshape(-1) != 0
    p = np.clip(pos.astype(np.float64), eps, 1 - eps)
    r_uv = np.clip(a, eps, 1 - eps)
    r = np.clip(r_uv.mean(), eps, 1 - eps)
    kl = (p * np.log(r_uv / r) + (1 - p) * np.log((1 - r_uv) / (1 - r))).sum()
    return np.array([kl, a[pos].mean() if pos.any() else 0.0, a[~pos].mean() if (~pos).any() else 0.0])


def custom_batch(edge_counts, nodes_per_graph=6, seed=0):
    """Hand-built collated batch: graph g has ``nodes_per_graph`` nodes and exactly ``edge_counts[g]`` random directed edges inside
    it (0 allowed); edge ids of the graphs are interleaved so that ``edge_order`` is a real permutation."""
    rng = np.random.RandomState(seed)
    G = len(edge_counts)
    src, dst = [], []
    for g, n in enumerate(edge_counts):
        src.append(rng.randint(0, nodes_per_graph, size=n) + g * nodes_per_graph)
        dst.append(rng.randint(0, nodes_per_graph, size=n) + g * nodes_per_graph)
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64) if G else np.zeros((2, 0), dtype=np.int64)
    ei = ei[:, rng.permutation(ei.shape[1])]
    return Batch(x=torch.zeros(G * nodes_per_graph, 1), edge_index=torch.from_numpy(np.ascontiguousarray(ei)),
                 batch=torch.from_numpy(np.repeat(np.arange(G, dtype=np.int64), nodes_per_graph)), edge_attr=None,
                 y=torch.zeros(G, 1), num_graphs=G)
