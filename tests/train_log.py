"""Helpers of the training-pass-log tests: feed tests/eval_log_oracle.py what a replayed training step left behind, and read the kernel
nodes of a dumped hipGraph in launch order."""
import re

import numpy as np
import torch

from tests import eval_log_oracle as lo

K = 5


def cpu(t):
    return t.detach().cpu().numpy()


def new_oracle(ds, logit_cols=1):
    """A LogOracle with the capacities ``_new_logs`` gives a ragged instance: the dataset's totals, one batch per graph."""
    return lo.LogOracle(K, ds.num_graphs, int(ds.edge_local_all.shape[1]), ds.num_graphs, logit_cols)


def feed_padded(oracle, att, pb, logits, losses, real_graphs):
    """Append a replay's capacity-shaped outputs, copied to the host NOW: the next replay overwrites them."""
    oracle.append(cpu(att), cpu(pb.edge_label), cpu(pb.edge_index), cpu(pb.batch), int(pb.num_graphs), cpu(logits), cpu(pb.y), cpu(losses),
                  real_graphs=real_graphs)


def loss_means(triples):
    """fp64 means of fp32 (loss, pred, info) triples, as EpochLog sums them."""
    return np.stack([np.asarray(t, np.float32).astype(np.float64) for t in triples]).mean(0)


def kernel_nodes(dot_text):
    """The (mangled) kernel names of a hipGraphDebugDotPrint dump in node order, which is the order of capture; None when there is no
    dump or it holds no kernel node in the form this reads."""
    if dot_text is None:
        return None
    found = re.findall(r"\{ID \| (\d+) \| (.*?)\\<\\<\\<", dot_text)
    ids = [int(i) for i, _ in found]
    assert ids == sorted(set(ids)), "the dump lists its nodes by ascending id"          # ids count the other node kinds (memcpy) too
    return [name.strip() for _, name in found] or None


def kept_debug_graph():
    """A torch.cuda.CUDAGraph that keeps its hipGraph (``keep_graph=True``) with debug mode on: ``debug_dump`` needs the graph itself,
    which a default CUDAGraph gives up when it instantiates at the end of the capture.  None where torch has no ``keep_graph``."""
    try:
        graph = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        return None
    graph.enable_debug_mode()
    return graph


def read_kernel_list(path):
    """(torch version the list was recorded with, kernel names) of a file of tests/golden/: '#' lines are comments, the first of them
    'torch <version>'."""
    lines = open(path).read().splitlines()
    version = next(l.split()[2] for l in lines if l.startswith("# torch "))
    return version, [l for l in lines if l and not l.startswith("#")]


def library_kernels(names):
    return [n for n in names if n.startswith("_ZN4gsat")]


def assert_bitwise(a, b, what=""):
    assert set(a) == set(b), what
    for key in a:
        assert torch.equal(a[key], b[key]), f"{what}{key}"
