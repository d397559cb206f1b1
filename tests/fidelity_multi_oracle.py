"""CPU oracle of the multi-ranking stack and the level overlap (gsat_fidelity_stack_multi / gsat_level_overlap;
dp_gsat_amd.explanation_stack_multi / level_overlap), numpy: tests/fidelity_stack_oracle.py called per ranking and re-indexed."""
import numpy as np

from tests import fidelity_stack_oracle as fso


def variant_index(R, S, r, s, keep):
    """v = 1 + r S + s keeps level[r] <= s, v = 1 + R S + r S + s drops those edges; v = 0 is the batch itself."""
    return 1 + (0 if keep else R * S) + r * S + s


def segment_capacities(E_cap, batch_size, R, ks=None, ratios=None):
    """[E_cap], the keep capacities of the levels ranking after ranking, [E_cap] * R S."""
    one = fso.segment_capacities(E_cap, batch_size, ks=ks, ratios=ratios)
    S = (len(one) - 1) // 2
    return [E_cap] + one[1:1 + S] * R + [E_cap] * (R * S)


def stack_oracle(edge_index, N, batch, G, levels, S, caps, N_cap, valid_in=None, Gp=None):
    """``levels`` uint8[R, E]; ``caps`` the 1 + 2 R S segment capacities.  Every ranking goes through the single-ranking oracle with its
    own segments; its variants are moved to their place: node ids by (v - u) N_cap, graph ids by (v - u) Gp, u the single index."""
    levels = np.asarray(levels)
    R = levels.shape[0]
    V = 1 + 2 * R * S
    assert len(caps) == V
    Gp = G + 1 if Gp is None else Gp
    offsets = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    out_ei = np.zeros((2, offsets[-1]), np.int64)
    out_id = np.full(offsets[-1], -1, np.int64)
    out_batch = np.zeros(V * N_cap, np.int64)
    valid = np.zeros((V, 4), np.int64)
    for r in range(R):
        keep_v = [variant_index(R, S, r, s, True) for s in range(S)]
        drop_v = [variant_index(R, S, r, s, False) for s in range(S)]
        place = [0] + keep_v + drop_v                                  # single variant u -> multi variant v
        one = fso.stack_oracle(edge_index, N, batch, G, levels[r], S, [caps[v] for v in place], N_cap, valid_in, Gp)
        for u, v in enumerate(place):
            if v == 0 and r > 0:
                continue                                               # the full variant is shared: ranking 0 wrote it
            lo, hi = one["offsets"][u], one["offsets"][u + 1]
            out_ei[:, offsets[v]:offsets[v + 1]] = one["edge_index"][:, lo:hi] + (v - u) * N_cap
            out_id[offsets[v]:offsets[v + 1]] = one["edge_id"][lo:hi]
            out_batch[v * N_cap:(v + 1) * N_cap] = one["batch"][u * N_cap:(u + 1) * N_cap] + (v - u) * Gp
            valid[v] = one["valid"][u]
    return dict(edge_index=out_ei, edge_id=out_id, batch=out_batch, valid=valid, offsets=[int(o) for o in offsets])


def overlap_counts(a, b, S, count=None):
    """int64[S, 3]: per level s, #(a <= s & b <= s), #(a <= s), #(b <= s) over the first ``count`` entries; an entry at level S or
    above is in no level."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    n = len(a) if count is None else min(max(int(count), 0), len(a))
    a, b = a[:n], b[:n]
    return np.array([[int(((a <= s) & (b <= s)).sum()), int((a <= s).sum()), int((b <= s).sum())] for s in range(S)], dtype=np.int64).reshape(S, 3)


def overlap_counts_by_sets(a, b, S, count=None):
    """The same from the definition: the kept sets of level s as Python sets of edge ids, and their intersection."""
    n = len(a) if count is None else min(max(int(count), 0), len(a))
    rows = []
    for s in range(S):
        A = {e for e in range(n) if int(a[e]) < S and int(a[e]) <= s}
        B = {e for e in range(n) if int(b[e]) < S and int(b[e]) <= s}
        rows.append([len(A & B), len(A), len(B)])
    return np.array(rows, dtype=np.int64).reshape(S, 3)
