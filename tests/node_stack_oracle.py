"""CPU oracle of the node explanations (dp_gsat_amd.rank_nodes / topk_node_mask / node_levels / node_precision_at_k and
gsat_fidelity_stack_nodes; dp_gsat_amd.explanation_stack_nodes), numpy.  The ranking is a stable sort on (-att, id) with -0.0 counted as
+0.0; the stack is built variant by variant through tests.padded_subgraph_oracle.subgraph_padded_oracle(mode="node")."""
import numpy as np

from tests import padded_subgraph_oracle as pso


def node_ptr_of(batch, G):
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(batch, dtype=np.int64), minlength=G)[:G])]).astype(np.int64)


def rank_nodes_oracle(att, batch, G):
    """(order int64[N], rank int64[N], node_ptr int64[G + 1]) of the first G graphs of a sorted ``batch`` vector: inside every graph
    higher score first, equal score -> lower node id first, -0.0 == +0.0.  Nodes of graphs >= G get order / rank -1."""
    att = np.asarray(att, dtype=np.float32).reshape(-1) + np.float32(0.0)            # -0.0 + 0.0 = +0.0
    batch = np.asarray(batch, dtype=np.int64)
    ptr = node_ptr_of(batch, G)
    order = np.full(len(att), -1, np.int64)
    rank = np.full(len(att), -1, np.int64)
    for g in range(G):
        lo, hi = ptr[g], ptr[g + 1]
        o = lo + np.argsort(-att[lo:hi].astype(np.float64), kind="stable")
        order[lo:hi] = o
        rank[o] = np.arange(hi - lo)
    return order, rank, ptr


def kept_counts(counts, k=None, ratio=None):
    """Nodes a level keeps of graphs with ``counts`` nodes: min(k, N_g), or ceil(N_g * ratio) in fp64."""
    counts = np.asarray(counts, dtype=np.int64)
    if k is not None:
        return np.minimum(counts, int(k))
    return np.ceil(counts.astype(np.float64) * np.float64(ratio)).astype(np.int64)


def topk_node_mask_oracle(att, batch, G, k=None, ratio=None):
    """bool[N]; False for the nodes of graphs >= G."""
    _, rank, ptr = rank_nodes_oracle(att, batch, G)
    batch = np.asarray(batch, dtype=np.int64)
    keep = kept_counts(np.diff(ptr), k, ratio)
    ranked = batch < G
    return ranked & (rank < keep[np.minimum(batch, max(G - 1, 0))]) if G else np.zeros(len(batch), bool)


def node_levels_oracle(att, batch, G, ks=None, ratios=None):
    """uint8[N]: the smallest level that keeps the node, S when none does (also for the nodes of graphs >= G)."""
    levels = ks if ks is not None else ratios
    masks = [topk_node_mask_oracle(att, batch, G, **({"k": l} if ks is not None else {"ratio": l})) for l in levels]
    kept = np.stack(masks).astype(np.int64)
    assert (np.diff(kept, axis=0) >= 0).all(), "the kept sets of increasing levels must be nested"
    return (len(levels) - kept.sum(axis=0)).astype(np.uint8)


def node_precision_oracle(att, label, k, batch, G):
    """float32[G]: labelled nodes among the min(k, N_g) best of every graph, over k, the quotient formed in fp64."""
    order, _, ptr = rank_nodes_oracle(att, batch, G)
    label = np.asarray(label).reshape(-1) != 0
    hits = np.array([label[order[ptr[g]:ptr[g] + min(k, ptr[g + 1] - ptr[g])]].sum() for g in range(G)], dtype=np.float64)
    return (hits / float(k)).astype(np.float32)


def variant_masks(level, S):
    """The V = 2 S + 1 keep masks over the node rows: everything, level <= s, level > s (levels above S count as S)."""
    lv = np.minimum(np.asarray(level, dtype=np.int64), S)
    return [np.ones(len(lv), bool)] + [lv <= s for s in range(S)] + [lv > s for s in range(S)]


def node_stack_oracle(edge_index, N, batch, G, level, S, caps, N_cap, valid_in=None, Gp=None):
    """``edge_index`` [2, E], ``batch`` [N], ``level`` uint8[N] of the input at its full shape; ``valid_in`` of a padded input or None;
    ``caps`` the V edge-segment lengths; ``Gp`` the graphs per variant (default ``G + 1``).  Variant v is
    ``subgraph_padded_oracle(mode="node", keep = its mask, capacity (N_cap, caps[v]), pad_graph Gp - 1)`` with the node ids of its
    edge_index moved by v * N_cap and its batch by v * Gp.  Returns int64 ``edge_index`` [2, E_stack], ``edge_id`` [E_stack], ``node_id`` /
    ``batch`` [V * N_cap], ``valid`` [V, 4] and the host list ``offsets``."""
    V = 2 * S + 1
    Gp = G + 1 if Gp is None else Gp
    offsets = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    out_ei = np.zeros((2, offsets[-1]), np.int64)
    out_id = np.zeros(offsets[-1], np.int64)
    node_id = np.zeros(V * N_cap, np.int64)
    out_batch = np.zeros(V * N_cap, np.int64)
    valid = np.zeros((V, 4), np.int64)
    for v, mask in enumerate(variant_masks(level, S)):
        o = pso.subgraph_padded_oracle(edge_index, N, batch, G, mask, "node", False, (N_cap, caps[v]), valid_in, pad_graph=Gp - 1)
        lo, hi = offsets[v], offsets[v + 1]
        out_ei[:, lo:hi] = o["edge_index"] + v * N_cap
        out_id[lo:hi] = o["edge_id"]
        node_id[v * N_cap:(v + 1) * N_cap] = o["node_id"]
        out_batch[v * N_cap:(v + 1) * N_cap] = o["batch"] + v * Gp
        valid[v] = o["valid"]
    return dict(edge_index=out_ei, edge_id=out_id, node_id=node_id, batch=out_batch, valid=valid, offsets=[int(o) for o in offsets])
