"""The inputs the multi-ranking stack and the level-overlap tests share, numpy only: batches with an exact edge count whose graphs sit
where the kernels can go wrong, and levels restated from a per-graph ranking."""
import numpy as np

EDGE_COUNTS = (0, 1, 1023, 1024, 1025, 2049)       # around gsat_fidelity_stack_block_items() = 1024 edge slots per workgroup
KS = (3, 40, 200, 260, 300)                         # the smallest k is above the tiny graph's 2 edges


def graph_edge_counts(E):
    """1 to 7 graphs with E edges in all: a graph of 2 edges (below the smallest k), a graph without edges, and five that share the rest
    -- with E above 1024 one of them straddles the workgroup boundary at edge slot 1024 (and at 2048 for E = 2049)."""
    if E < 8:
        return [E]
    rest = E - 2
    parts = [int(rest * f) for f in (0.3, 0.25, 0.2, 0.15)]
    return [2, 0] + parts + [rest - sum(parts)]


def make_graphs(E, seed=0):
    """edge_index int64[2, E] (grouped by graph, random endpoints inside the graph), batch int64[N], the per-graph edge counts."""
    rng = np.random.RandomState(1000 + 7 * E + seed)
    counts = graph_edge_counts(E)
    src, dst, batch, off = [], [], [], 0
    for g, e in enumerate(counts):
        n = max(2, e // 3 + 2)
        src.append(off + rng.randint(0, n, size=e))
        dst.append(off + rng.randint(0, n, size=e))
        batch += [g] * n
        off += n
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64).reshape(2, -1)
    assert ei.shape[1] == E
    return ei, np.asarray(batch, dtype=np.int64), counts


def random_ranks(counts, seed=0):
    """int64[E]: every graph's edges in a random order -- the position of each edge inside its graph."""
    rng = np.random.RandomState(50 + seed)
    return np.concatenate([rng.permutation(e) for e in counts] + [np.zeros(0, np.int64)]).astype(np.int64)


def reversed_ranks(rank, counts):
    """The reverse ranking: the best edge of a graph becomes its worst."""
    eg = np.repeat(np.asarray(counts, dtype=np.int64), counts)
    return eg - 1 - rank


def levels_of(rank, counts, ks=None, ratios=None):
    """uint8[E]: the smallest level whose top-k (top-ceil(ratio E_g)) of the edge's graph holds the edge, S when none does."""
    levels = ks if ks is not None else ratios
    S = len(levels)
    eg = np.repeat(np.asarray(counts, dtype=np.int64), counts)
    out = np.full(len(rank), S, dtype=np.uint8)
    for s in range(S - 1, -1, -1):
        kc = np.minimum(levels[s], eg) if ks is not None else np.ceil(eg.astype(np.float64) * levels[s]).astype(np.int64)
        out[rank < kc] = s
    return out


def ranking_levels(E, R, ks, seed=0):
    """uint8[R, E] and the graphs: ranking 0 random, ranking 1 its reverse (disjoint keep sets at small levels), ranking 2 equal to
    ranking 0 (identical variants)."""
    ei, batch, counts = make_graphs(E, seed)
    r0 = random_ranks(counts, seed)
    ranks = [r0, reversed_ranks(r0, counts), r0][:R]
    return np.stack([levels_of(r, counts, ks=list(ks)) for r in ranks]).reshape(R, E), ei, batch, counts
