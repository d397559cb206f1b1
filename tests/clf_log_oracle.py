"""CPU oracle of the classifier log (csrc/clf_log.hip, dp_gsat_amd.eval_log.ClfLog): numpy, nothing from the package.  Written from the
rules of include/gsat_hip.h: append with its plan and flags, the integer counts, and compute()."""
import numpy as np

from tests import evaluate_oracle as eo

FLAG_OVERFLOW, FLAG_FULL = 1, 2


def mode_of(multi_label, logit_cols):
    return 2 if multi_label else (0 if logit_cols == 1 else 1)


def counts_oracle(logits, y, mode):
    """mode 0 / 1: int64[C * C + 1] -- confusion (row = label, column = prediction), then ``bad``.  mode 2: int64[T, 5] -- (tn, fp, fn,
    tp, unlabelled) per task."""
    z = np.asarray(logits, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32).reshape(z.shape[0], z.shape[1] if mode == 2 else 1)
    if mode == 2:
        out = np.zeros((z.shape[1], 5), dtype=np.int64)
        for t in range(z.shape[1]):
            for zz, yy in zip(z[:, t], y[:, t]):
                if np.isnan(yy):
                    out[t, 4] += 1
                else:
                    out[t, (2 if yy != 0 else 0) + (1 if zz > 0 else 0)] += 1
        return out
    C = 2 if mode == 0 else z.shape[1]
    out = np.zeros(C * C + 1, dtype=np.int64)
    for row, yy in zip(z, y[:, 0]):
        if np.isnan(row).any() or np.isnan(yy) or yy != np.floor(yy) or not 0 <= yy < C:
            out[C * C] += 1
            continue
        pred = int(row[0] > 0) if mode == 0 else int(np.argmax(row))       # numpy's argmax: the first of equal maxima
        out[int(yy) * C + pred] += 1
    return out


class ClfLogOracle:
    SENTINEL = 0x7FC0A5A5     # every word of a fresh array, a NaN with a payload: whatever an append does not write keeps it

    def __init__(self, max_graphs, max_batches, logit_cols, y_cols=1, multi_label=False):
        self.max_graphs, self.max_batches, self.logit_cols, self.y_cols = max_graphs, max_batches, logit_cols, y_cols
        self.multi_label, self.mode = multi_label, mode_of(multi_label, logit_cols)
        fresh = lambda shape: np.full(shape, self.SENTINEL, dtype=np.int32).view(np.float32)
        self.logits = fresh((max_graphs, logit_cols))
        self.y = fresh((max_graphs, y_cols))
        self.loss_sum = np.zeros(1, dtype=np.float64)
        self.state = np.zeros(4, dtype=np.int64)

    def reset(self):
        self.state[:] = 0
        self.loss_sum[:] = 0

    def append(self, logits, y, loss=None, valid=None):
        """``valid``: the int32[4] word (N_real, E_real, B, overflow) of a padded batch, or None: every row."""
        z = np.asarray(logits, dtype=np.float32).reshape(-1, self.logit_cols)
        y = np.asarray(y, dtype=np.float32).reshape(z.shape[0], self.y_cols)
        G_cap = z.shape[0]
        g0, b0 = int(self.state[0]), int(self.state[1])
        if valid is not None and valid[3] != 0:
            self.state[2] |= FLAG_OVERFLOW
            return
        G = int(valid[2]) if valid is not None else G_cap
        if G < 0 or G > G_cap or g0 + G > self.max_graphs or b0 + 1 > self.max_batches:
            self.state[2] |= FLAG_FULL
            return
        self.logits[g0:g0 + G] = z[:G]
        self.y[g0:g0 + G] = y[:G]
        self.loss_sum[0] += np.float64(np.float32(loss)) if loss is not None else np.nan
        self.state[0], self.state[1] = g0 + G, b0 + 1

    def compute(self):
        n, nb, flags, _ = (int(v) for v in self.state)
        if flags & FLAG_OVERFLOW:
            raise ValueError("flag bit 0")
        if flags & FLAG_FULL:
            raise ValueError("flag bit 1")
        if nb == 0:
            raise ValueError("before any append")
        z, y = self.logits[:n], self.y[:n]
        c = counts_oracle(z, y, self.mode)
        res = {"n": n, "loss": float(self.loss_sum[0] / nb)}
        if self.mode == 2:
            T = self.logit_cols
            res.update(task_counts=c[:, :4].copy(), unlabelled=c[:, 4].copy())
            res["clf_acc"] = float(c[:, 0].sum() + c[:, 3].sum()) / (n * T) if n else float("nan")
            tc = eo.task_counts_oracle(z, y)
            res["clf_roc_tasks"] = np.array([int(U2) / (2 * int(P) * int(Nn)) if P > 0 and Nn > 0 else np.nan for U2, P, Nn in tc])
            res["clf_roc"] = eo.rocauc_oracle(z, y)
        else:
            C = 2 if self.mode == 0 else self.logit_cols
            conf = c[:C * C].reshape(C, C)
            res.update(confusion=conf.copy(), bad=int(c[C * C]))
            res["clf_acc"] = float(np.trace(conf)) / n if n else float("nan")
            res["clf_roc"] = (eo.rocauc_oracle(z, y) if n else float("nan")) if self.mode == 0 else 0.0
        return res
