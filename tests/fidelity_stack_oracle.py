"""CPU oracle of the fidelity-curve levels and the stacked batch (gsat_fidelity_levels / gsat_fidelity_stack;
dp_gsat_amd.explanation_levels / explanation_stack), numpy.  The stack is built variant by variant from the definition -- a mask, the kept
edges in order, the padding rule restated -- and NOT through tests.padded_subgraph_oracle: test_fidelity_stack_host.py holds the two
against each other."""
import numpy as np

from tests import explain_oracle as xo


def levels_oracle(att, edge_index, batch, G, ks=None, ratios=None):
    """uint8[E]: the smallest level that keeps the edge, S when none does.  The kept sets are nested, so that is S minus the number of
    levels that keep it; every level's mask comes from the ranking oracles of tests.explain_oracle."""
    levels = ks if ks is not None else ratios
    ei, b = np.asarray(edge_index), np.asarray(batch)
    masks = [xo.rank_oracle(att, ei, b, G, l)[2].astype(bool) if ks is not None else xo.topk_ratio_oracle(att, ei, b, G, l) for l in levels]
    kept = np.stack(masks).astype(np.int64)
    assert (np.diff(kept, axis=0) >= 0).all(), "the kept sets of increasing levels must be nested"
    return (len(levels) - kept.sum(axis=0)).astype(np.uint8)


def keep_capacity(E_cap, batch_size, k=None, ratio=None):
    """dp_gsat_amd.replay.keep_capacity, restated."""
    return k * batch_size if k is not None else min(E_cap, int(np.ceil(ratio * E_cap)) + batch_size)


def segment_capacities(E_cap, batch_size, ks=None, ratios=None):
    """[E_cap] for the full variant, the keep capacities of the levels, [E_cap] * S for the drop variants."""
    levels = ks if ks is not None else ratios
    keep = [keep_capacity(E_cap, batch_size, **({"k": l} if ks is not None else {"ratio": l})) for l in levels]
    return [E_cap] + keep + [E_cap] * len(levels)


def padding_edges(N, n_pad, e_pad):
    """int64[2, e_pad]: pair q joins the padding nodes N + q % n_pad and N + (q + 1) % n_pad, forward in the even slot and back in the odd
    one; an odd count ends in a self loop (padding_edge of csrc/common.h)."""
    j = np.arange(e_pad, dtype=np.int64)
    q = j >> 1
    a, b = N + q % n_pad, N + (q + 1) % n_pad
    fwd = (j & 1) == 0
    loop = (j == e_pad - 1) & bool(e_pad & 1)
    return np.stack([np.where(fwd, a, b), np.where(loop, a, np.where(fwd, b, a))])


def variant_masks(level, S):
    """The V = 2 S + 1 masks over the counted edges: everything, level <= s, level > s."""
    lv = np.minimum(np.asarray(level, dtype=np.int64), S)
    return [np.ones(len(lv), bool)] + [lv <= s for s in range(S)] + [lv > s for s in range(S)]


def stack_oracle(edge_index, N, batch, G, level, S, caps, N_cap, valid_in=None, Gp=None):
    """``edge_index`` [2, E], ``batch`` [N], ``level`` [E] of the input at its full shape; ``valid_in`` (N_real, E_real, graphs, overflow)
    of a padded input or None; ``caps`` the V segment capacities; ``Gp`` the graphs per variant (default ``G + 1``).  Entries of ``level``
    at or beyond the counted edges are never looked at.  Returns int64 ``edge_index`` [2, E_stack], ``edge_id`` [E_stack], ``batch``
    [V * N_cap], ``valid`` [V, 4] and the host list ``offsets``."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    E, V = ei.shape[1], 2 * S + 1
    batch = np.asarray(batch, dtype=np.int64)
    Gp = G + 1 if Gp is None else Gp
    Nv, Ev, g, spoiled = N, E, G, False
    if valid_in is not None:
        spoiled = int(valid_in[3]) != 0
        Nv = 0 if spoiled else min(max(int(valid_in[0]), 0), N)
        Ev = 0 if spoiled else min(max(int(valid_in[1]), 0), E)
        g = int(valid_in[2])
    real = ei[:, :Ev]
    bad = ((real < 0) | (real >= Nv)).any(axis=0)
    share = valid_in is not None and N_cap == N
    offsets = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    out_ei = np.zeros((2, offsets[-1]), np.int64)
    out_id = np.full(offsets[-1], -1, np.int64)
    out_batch = np.zeros(V * N_cap, np.int64)
    valid = np.zeros((V, 4), np.int64)
    rows = np.arange(N_cap)
    for v, mask in enumerate(variant_masks(np.asarray(level).reshape(-1)[:Ev], S)):
        ids = np.nonzero(mask & ~bad)[0]
        over = Nv + 2 > N_cap or len(ids) > caps[v] or spoiled or bool(bad.any())
        n_out, e_out = (0, 0) if over else (Nv, len(ids))
        valid[v] = [0, 0, 0, 1] if over else [n_out, e_out, g, 0]
        lo = offsets[v]
        out_ei[:, lo:lo + e_out] = real[:, ids[:e_out]] + v * N_cap
        out_id[lo:lo + e_out] = ids[:e_out]
        out_ei[:, lo + e_out:lo + caps[v]] = padding_edges(n_out, N_cap - n_out, caps[v] - e_out) + v * N_cap
        own = (rows < N) & (share | (rows < n_out))
        out_batch[v * N_cap:(v + 1) * N_cap] = v * Gp + np.where(own, batch[np.minimum(rows, max(N - 1, 0))] if N else 0, Gp - 1)
    return dict(edge_index=out_ei, edge_id=out_id, batch=out_batch, valid=valid, offsets=[int(o) for o in offsets])
