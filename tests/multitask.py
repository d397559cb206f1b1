"""Fixtures of the multi-task tests: three label columns with NaNs for the graphs of tests/padded_oracle.py, the multi-label model
builder, and the per-task ROC-AUC of tests/evaluate_oracle.py."""
import numpy as np
import torch

from tests import evaluate_oracle as eo
from tests import padded_oracle as po

T = 3
UNSCORABLE = 2                 # the task whose labelled rows are all positive
NAN_TASK = 1                   # the task that is unlabelled ...
NAN_GRAPHS = range(7, 17)      # ... throughout these graphs: the second budget batch of range(48) at tests/ragged_oracle.py's capacity
H = 32


def task_labels(graphs):
    """float32[len(graphs), T]: task 0 the graph's own label, task 1 'more nodes than the median graph', task 2 always 1; about 20 % of the
    entries NaN (unlabelled), task NAN_TASK NaN for every graph of NAN_GRAPHS."""
    n = np.array([g.x.shape[0] for g in graphs])
    y = np.stack([np.array([float(g.y.reshape(-1)[0]) for g in graphs]), (n > np.median(n)).astype(np.float64), np.ones(len(graphs))], axis=1)
    y = y.astype(np.float32)
    y[np.random.RandomState(11).rand(*y.shape) < 0.2] = np.nan
    y[[g for g in NAN_GRAPHS if g < len(graphs)], NAN_TASK] = np.nan
    return y


def labelled_graphs(count, **kw):
    """po.mutag_graphs with y [1, T] from task_labels and pseudo-random edge labels (tests/test_gpu_eval_log.py's rule)."""
    graphs = po.mutag_graphs(count, **kw)
    y = task_labels(graphs)
    rng = np.random.RandomState(5)
    for i, g in enumerate(graphs):
        g.y = torch.from_numpy(y[i:i + 1].copy())
        g.edge_label = torch.from_numpy((rng.rand(g.edge_index.shape[1]) < 0.3).astype(np.float32))
    return graphs


def gsat(dev, backbone, edge, graphs, capturable=True, dropout_p=0.3):
    """tests/test_gpu_eval_log.py's model with a T-column multi-label head and ``Criterion(T, True, capturable=capturable)``."""
    import dp_gsat_amd as G
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=dropout_p, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=deg)
    clf = G.get_model(14, 0, T, True, cfg, dev)
    ext = G.ExtractorMLP(H, edge).to(dev)
    params = list(clf.parameters()) + list(ext.parameters())
    opt = torch.optim.Adam(params, lr=1e-2, weight_decay=3e-6, capturable=True, fused=True)
    return G.GSAT(clf, ext, G.Criterion(T, True, capturable=capturable), opt, learn_edge_att=edge, decay_interval=1).train()


def roc_tasks_oracle(logits, y):
    """float64[T]: the per-task ROC-AUC of tests/evaluate_oracle.py's counts, NaN for a task without both classes among its labelled rows."""
    return np.array([int(U2) / (2 * int(P) * int(Nn)) if P > 0 and Nn > 0 else np.nan for U2, P, Nn in eo.task_counts_oracle(logits, y)])
