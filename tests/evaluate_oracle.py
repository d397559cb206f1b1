"""CPU oracle of dp_gsat_amd.evaluate (numpy / scipy, nothing from the package): per-task midrank AUROC counts with NaN labels, the ogb
mean rule, both accuracies, the fp64 bin formula of the attention histogram and the suffix-sum PR curve."""
import numpy as np
from scipy.stats import rankdata


def _canon(x):
    """fp32 with -0.0 folded into +0.0 (the contract's only canonicalisation)."""
    return np.asarray(x, dtype=np.float32) + np.float32(0.0)


def _two_d(x, dtype):
    x = np.asarray(x, dtype=dtype)
    return x.reshape(-1, 1) if x.ndim == 1 else x


def task_counts_oracle(scores, labels):
    """int64[T, 3]: per column (U2, P, Nn) over the rows whose label is not NaN; label 0 = negative, anything else = positive.
    2 * midrank is an integer and U2 = sum over positives of 2 * midrank - P (P + 1), as in tests/explain_oracle.py."""
    s, y = _canon(_two_d(scores, np.float32)), _two_d(labels, np.float64)
    assert s.shape == y.shape
    out = np.zeros((s.shape[1], 3), dtype=np.int64)
    for t in range(s.shape[1]):
        have = ~np.isnan(y[:, t])
        a, pos = s[have, t].astype(np.float64), y[have, t] != 0
        P, Nn = int(pos.sum()), int((~pos).sum())
        U2 = 0
        if a.size:
            r2 = np.rint(2.0 * rankdata(a, method="average")).astype(np.int64)
            U2 = int(r2[pos].sum()) - P * (P + 1)
        out[t] = (U2, P, Nn)
    return out


def rocauc_oracle(scores, labels):
    """The ogb Evaluator's rule (_eval_rocauc): the mean of the per-task AUROC over the tasks with a positive and a negative labelled
    row; NaN where ogb raises because no task qualifies."""
    c = task_counts_oracle(scores, labels)
    per = [int(U2) / (2 * int(P) * int(Nn)) for U2, P, Nn in c if P > 0 and Nn > 0]
    return float(np.mean(per)) if per else float("nan")


def preds_oracle(logits, multi_label):
    """get_preds (src/utils/get_model.py:37-44): sigmoid > 0.5 for multi-label and one-column heads, else argmax.  Restated as
    logit > 0, which differs from the fp32 sigmoid only for 0 < logit < 2^-23 (there the sigmoid rounds to 0.5): callers keep their
    logits away from that sliver."""
    z = np.asarray(logits, dtype=np.float32)
    if multi_label or z.shape[1] == 1:
        return (z > 0).astype(np.float32)
    return z.argmax(axis=1).astype(np.float32)


def accuracy_oracle(logits, labels, multi_label):
    """src/run_gsat.py:748 (matches over the rows) / src/pretrain_clf.py:97 (matches over R * T; a NaN label never matches)."""
    p = preds_oracle(logits, multi_label)
    y = np.asarray(labels, dtype=np.float64).reshape(p.shape)
    return float((p == y).sum()) / float(p.size if multi_label else p.shape[0])


def histogram_oracle(att, labels, bins, lo, hi):
    """(counts int64[2, bins], outside int64[2]).  The contract's bin in fp64: t = (float64(a) - lo) * (bins / (hi - lo)),
    bin = min(floor(t), bins - 1); a < lo, a > hi or NaN is not binned and counts in outside[class]."""
    a = np.asarray(att, dtype=np.float32).reshape(-1).astype(np.float64)
    cls = np.zeros(a.size, dtype=np.int64) if labels is None else (np.asarray(labels).reshape(-1) != 0).astype(np.int64)
    lo, hi = np.float64(lo), np.float64(hi)
    inside = (a >= lo) & (a <= hi)                                        # False for NaN
    scale = np.float64(bins) / (hi - lo)
    b = np.minimum(np.floor((a[inside] - lo) * scale).astype(np.int64), bins - 1)
    counts = np.zeros((2, bins), dtype=np.int64)
    np.add.at(counts, (cls[inside], b), 1)
    return counts, np.bincount(cls[~inside], minlength=2).astype(np.int64)


def pr_curve_oracle(counts):
    """Threshold i predicts positive what fell into a bin >= i: suffix sums of the two rows."""
    c = np.asarray(counts, dtype=np.int64)
    fp, tp = (np.cumsum(c[k][::-1])[::-1] for k in (0, 1))
    tn, fn = c[0].sum() - fp, c[1].sum() - tp
    return {"tp": tp, "fp": fp, "tn": tn, "fn": fn, "precision": tp / np.maximum(tp + fp, 1), "recall": tp / np.maximum(tp + fn, 1)}
