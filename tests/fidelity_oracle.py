"""CPU oracle of the fidelity log (gsat_fidelity_append / FidelityLog.compute), fp64 numpy."""
import numpy as np


def classes(z):
    """Predicted class per row of fp32 logits [G, C]: C == 1: z >= 0; else the argmax, lowest index on ties."""
    z = np.asarray(z, dtype=np.float32)
    return (z[:, 0] >= 0).astype(np.int32) if z.shape[1] == 1 else np.argmax(z, axis=1).astype(np.int32)


def prob_of(z, cls):
    """fp64 probability of class ``cls[i]`` under row i: sigmoid(+-z) for one logit, else the softmax with the row maximum subtracted."""
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    if z.shape[1] == 1:
        t = np.where(cls != 0, z[:, 0], -z[:, 0])
        return 1.0 / (1.0 + np.exp(-t))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e[np.arange(len(z)), cls] / e.sum(axis=1)


def rows(full, keep, drop):
    """(cls int32[G, 3], p float64[G, 3]) of one batch, as the append kernel writes them."""
    cls = classes(full)
    return (np.stack([cls, classes(keep), classes(drop)], axis=1).astype(np.int32),
            np.stack([prob_of(full, cls), prob_of(keep, cls), prob_of(drop, cls)], axis=1))


def compute(cls, p):
    """FidelityLog.compute() over the logged rows."""
    n = len(cls)
    return {"fidelity_plus": float((p[:, 0] - p[:, 2]).mean()), "fidelity_minus": float((p[:, 0] - p[:, 1]).mean()),
            "p_full": float(p[:, 0].mean()), "p_keep": float(p[:, 1].mean()), "p_drop": float(p[:, 2].mean()),
            "flip_plus": int((cls[:, 2] != cls[:, 0]).sum()) / n, "flip_minus": int((cls[:, 1] != cls[:, 0]).sum()) / n, "n": n}
