"""numpy restatement of dp_gsat_amd.eval_log: the append layout of EpochLog and the scores of its compute()."""
import numpy as np

from tests import evaluate_oracle as eo
from tests import explain_oracle as xo

FLAG_OVERFLOW, FLAG_FULL = 1, 2


class LogOracle:
    """The arrays of EpochLog as numpy arrays of the same dtype, every one prefilled with a sentinel byte pattern so that a test can
    tell untouched memory; ``state`` = [edges, graphs, batches, flags]."""

    SENTINEL = 0xA5

    def __init__(self, k, max_graphs, max_edges, max_batches, logit_cols, y_cols=1, bins=64):
        self.k, self.bins = k, bins
        self.max_graphs, self.max_edges, self.max_batches = max_graphs, max_edges, max_batches
        fill = lambda shape, dt: np.frombuffer(bytes([self.SENTINEL]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dtype=dt).reshape(shape).copy()
        self.att, self.label = fill((max_edges,), np.float32), fill((max_edges,), np.uint8)
        self.graph_edge_ptr = fill((max_graphs + 1,), np.int32)
        self.logits, self.y = fill((max_graphs, logit_cols), np.float32), fill((max_graphs, y_cols), np.float32)
        self.batch_edge_ptr = fill((max_batches + 1,), np.int64)
        self.loss_sums = np.zeros(3, np.float64)
        self.state = np.zeros(4, np.int64)

    def arrays(self):
        return dict(att=self.att, label=self.label, graph_edge_ptr=self.graph_edge_ptr, logits=self.logits, y=self.y,
                    batch_edge_ptr=self.batch_edge_ptr)

    def append(self, att, labels, edge_index, batch, num_graphs, logits, y, losses=None, real_graphs=None, overflow=False):
        """``num_graphs``: the graphs of the batch arrays (for a padded batch: B + 1); ``real_graphs``: how many of them are logged (a
        padded batch's valid[2]; default all); ``overflow``: the padded batch's valid[3]."""
        if overflow:
            self.state[3] |= FLAG_OVERFLOW
            return
        G = num_graphs if real_graphs is None else real_graphs
        ei, b = np.asarray(edge_index), np.asarray(batch)
        eg = b[ei[0]] if ei.shape[1] else np.zeros(0, np.int64)
        order = np.argsort(eg, kind="stable")                              # graph by graph, ascending edge id inside a graph
        ptr = np.concatenate([[0], np.cumsum(np.bincount(eg, minlength=num_graphs))]).astype(np.int64)
        E = int(ptr[G])
        e0, g0, b0 = (int(v) for v in self.state[:3])
        if e0 + E > self.max_edges or g0 + G > self.max_graphs or b0 + 1 > self.max_batches:
            self.state[3] |= FLAG_FULL
            return
        a = np.asarray(att, np.float32).reshape(-1)
        lab = np.asarray(labels).reshape(-1) != 0
        self.att[e0:e0 + E] = a[order[:E]]
        self.label[e0:e0 + E] = lab[order[:E]]
        self.graph_edge_ptr[g0:g0 + G + 1] = e0 + ptr[:G + 1]
        self.logits[g0:g0 + G] = np.asarray(logits, np.float32).reshape(num_graphs, -1)[:G]
        self.y[g0:g0 + G] = np.asarray(y, np.float32).reshape(num_graphs, -1)[:G]
        self.batch_edge_ptr[b0] = e0
        self.batch_edge_ptr[b0 + 1] = e0 + E
        self.loss_sums += np.asarray(losses, np.float32).astype(np.float64) if losses is not None else np.nan
        self.state[:3] = (e0 + E, g0 + G, b0 + 1)

    # ---- the scores, from the logged prefix alone -------------------------------------------------------------------------------------
    def prefix(self):
        E, G, nb = (int(v) for v in self.state[:3])
        return self.att[:E], self.label[:E], self.graph_edge_ptr[:G + 1], self.batch_edge_ptr[:nb + 1]

    def hits(self):
        """int per logged graph: labelled edges among its k best (higher attention first, ties by lower position in the log)."""
        a, lab, gp, _ = self.prefix()
        a = xo.canon(a)
        out = []
        for g in range(len(gp) - 1):
            s = slice(gp[g], gp[g + 1])
            best = np.argsort(-a[s], kind="stable")[:self.k]
            out.append(int((lab[s][best] != 0).sum()))
        return np.array(out, np.int64)

    def auroc_counts(self):
        a, lab, _, _ = self.prefix()
        return xo.auroc_counts_oracle(a, lab)

    def histogram(self):
        a, lab, _, _ = self.prefix()
        return eo.histogram_oracle(a, lab, self.bins, 0.0, 1.0)

    def delta_kl_per_batch(self):
        a, lab, _, bp = self.prefix()
        return np.array([xo.delta_kl_oracle(a[bp[i]:bp[i + 1]], lab[bp[i]:bp[i + 1]])[0] if bp[i + 1] > bp[i] else 0.0
                         for i in range(len(bp) - 1)])

    def compute(self, multi_label=False):
        """The floats of EpochLog.compute() in fp64 and its integer arrays."""
        a, lab, gp, bp = self.prefix()
        G, nb = len(gp) - 1, len(bp) - 1
        U2, P, Nn = self.auroc_counts()
        counts, outside = self.histogram()
        z, y = self.logits[:G], self.y[:G]
        means = xo.delta_kl_oracle(a, lab)[1:]
        binary = multi_label or z.shape[1] == 1
        res = {"att_auroc": U2 / (2 * P * Nn) if P * Nn else 0.0, f"precision@{self.k}": float(self.hits().mean()) / self.k,
               "delta_kl": float(np.float32(self.delta_kl_per_batch()).astype(np.float64).mean()),
               "avg_signal_att_weights": float(means[0]), "avg_bkg_att_weights": float(means[1]),
               "clf_acc": eo.accuracy_oracle(z, y, multi_label), "clf_roc": eo.rocauc_oracle(z, y) if binary else 0.0,
               "bkg_att_hist": counts[0], "signal_att_hist": counts[1], "att_outside": outside, "pr_curve": eo.pr_curve_oracle(counts)}
        for i, n in enumerate(("loss", "pred", "info")):
            res[n] = float(self.loss_sums[i] / nb)
        return res
