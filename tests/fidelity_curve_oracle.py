"""CPU oracle of the level-aware fidelity log (gsat_fidelity_curve_append / FidelityCurveLog.compute), fp64 numpy."""
import numpy as np

from tests import fidelity_oracle as fo


def rows(logits, Gp, S, g):
    """(cls int32[g, V], p float64[g, V]) of one stacked batch: ``logits`` fp32 [V * Gp, C], block v = variant v; the first ``g`` graphs
    of every block are logged.  Column v: the class predicted from block v, and block v's probability of the class predicted from block 0."""
    V = 2 * S + 1
    z = np.asarray(logits, dtype=np.float32).reshape(V, Gp, -1)[:, :g]
    cls_full = fo.classes(z[0])
    return (np.stack([fo.classes(z[v]) for v in range(V)], axis=1).astype(np.int32),
            np.stack([fo.prob_of(z[v], cls_full) for v in range(V)], axis=1))


def compute(cls, p, S, kept_edges, real_edges, levels):
    """FidelityCurveLog.compute() over the logged rows; ``kept_edges`` [S] and ``real_edges`` are the integer sums over the batches."""
    n = len(cls)
    keep, drop = slice(1, 1 + S), slice(1 + S, 1 + 2 * S)
    return {"levels": list(levels),
            "fidelity_plus": [float(v) for v in (p[:, :1] - p[:, drop]).mean(axis=0)],
            "fidelity_minus": [float(v) for v in (p[:, :1] - p[:, keep]).mean(axis=0)],
            "p_full": float(p[:, 0].mean()), "p_keep": [float(v) for v in p[:, keep].mean(axis=0)],
            "p_drop": [float(v) for v in p[:, drop].mean(axis=0)],
            "flip_plus": [int(v) / n for v in (cls[:, drop] != cls[:, :1]).sum(axis=0)],
            "flip_minus": [int(v) / n for v in (cls[:, keep] != cls[:, :1]).sum(axis=0)],
            "kept_fraction": [int(k) / int(real_edges) for k in kept_edges], "n": n}


PROB_KEYS = ("fidelity_plus", "fidelity_minus", "p_full", "p_keep", "p_drop")
EXACT_KEYS = ("levels", "flip_plus", "flip_minus", "kept_fraction", "n")

