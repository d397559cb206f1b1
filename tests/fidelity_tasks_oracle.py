"""CPU oracle of the fidelity-curve log with a task axis (gsat_fidelity_curve_append_tasks / FidelityCurveLog(tasks=T).compute), fp64
numpy.  A multi-label head decides every (graph, task) on its own: class z >= 0, probability sigmoid(+-z) -- the one-logit rules of
tests/fidelity_oracle.py -- so task t of a stacked batch is tests/fidelity_curve_oracle.py on column t alone."""
import numpy as np

from tests import fidelity_curve_oracle as fco


def rows(logits, Gp, S, g, T):
    """(cls int32[g, T, V], p float64[g, T, V]) of one stacked batch: ``logits`` fp32 [V * Gp, T], block v = variant v; the first ``g``
    graphs of every block are logged.  Entry [i, t, v]: the class of graph i, task t predicted from block v, and block v's probability of
    the class predicted from block 0."""
    z = np.asarray(logits, dtype=np.float32).reshape(-1, T)
    per_task = [fco.rows(z[:, t:t + 1], Gp, S, g) for t in range(T)]
    return (np.stack([c for c, _ in per_task], axis=1).astype(np.int32), np.stack([p for _, p in per_task], axis=1))


TASK_KEYS = ("fidelity_plus", "fidelity_minus", "p_keep", "p_drop", "flip_plus", "flip_minus")


def compute(cls, p, S, kept_edges, real_edges, levels):
    """FidelityCurveLog(tasks=T).compute() over the logged rows ``cls`` / ``p`` [n, T, V]: per task the curve of
    tests/fidelity_curve_oracle.py (``*_tasks`` as [S][T], ``p_full_tasks`` as [T]); the plain keys are the fp64 mean over the tasks of
    the per-task means."""
    T = cls.shape[1]
    per = [fco.compute(cls[:, t], p[:, t], S, kept_edges, real_edges, levels) for t in range(T)]
    res = {"levels": list(levels), "kept_fraction": per[0]["kept_fraction"], "n": per[0]["n"],
           "p_full_tasks": [r["p_full"] for r in per], "p_full": float(np.mean([r["p_full"] for r in per]))}
    for key in TASK_KEYS:
        res[key + "_tasks"] = [[per[t][key][s] for t in range(T)] for s in range(S)]
        res[key] = [float(np.mean(np.array(row, dtype=np.float64))) for row in res[key + "_tasks"]]
    return res


PROB_KEYS = fco.PROB_KEYS + tuple(k + "_tasks" for k in fco.PROB_KEYS)
EXACT_KEYS = ("levels", "kept_fraction", "n", "flip_plus_tasks", "flip_minus_tasks")
