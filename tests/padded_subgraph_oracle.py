"""CPU oracle of the padded extraction (gsat_subgraph_padded; dp_gsat_amd.edge_subgraph_padded / node_subgraph_padded), numpy: the real
part is tests.subgraph_oracle.subgraph_oracle on the counted nodes and edges of the input, the slack is laid out by the padding rule of
tests.padded_oracle.collate_padded -- the extracted graph is handed to it as a one-graph dataset."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from tests import padded_oracle as po
from tests import subgraph_oracle as so


def subgraph_padded_oracle(edge_index, N, batch, G, keep, mode, drop_isolated, capacity, valid_in=None, pad_graph=None):
    """``edge_index`` [2, E], ``batch`` [N] and ``keep`` ([E], mode "edge"; [N], mode "node") of the input at its full shape; ``valid_in``
    (N_real, E_real, graphs, overflow) of a padded input or None; ``pad_graph`` defaults to ``G``, the graph id behind an unpadded
    input's graphs.  Entries of ``keep`` at or beyond the counts are never looked at.  Returns int64 arrays ``node_id`` / ``batch``
    [N_cap], ``edge_id`` [E_cap], ``edge_index`` [2, E_cap], uint8 ``edge_mask`` [E] and ``valid`` [4]."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    E = ei.shape[1]
    batch = np.asarray(batch, dtype=np.int64)
    keep = np.asarray(keep).reshape(-1) != 0
    N_cap, E_cap = capacity
    pad_graph = G if pad_graph is None else pad_graph
    Nv, Ev, g, spoiled = N, E, G, False
    if valid_in is not None:
        spoiled = int(valid_in[3]) != 0
        Nv = 0 if spoiled else min(max(int(valid_in[0]), 0), N)
        Ev = 0 if spoiled else min(max(int(valid_in[1]), 0), E)
        g = int(valid_in[2])
    real_ei = ei[:, :Ev].copy()
    bad = ((real_ei < 0) | (real_ei >= Nv)).any(axis=0)
    real_ei[:, bad] = 0                                        # never dereferenced; their mask entries are forced to 0 below
    if Nv == 0:
        o = dict(node_id=np.zeros(0, np.int64), edge_id=np.zeros(0, np.int64), edge_index=np.zeros((2, 0), np.int64),
                 batch=np.zeros(0, np.int64), edge_mask=np.zeros(Ev, np.uint8))
    else:
        k = keep[:Ev].copy() if mode == "edge" else keep[:Nv]
        if mode == "edge":
            k[bad] = False
        o = so.subgraph_oracle(real_ei, Nv, batch[:Nv], None, k, mode, drop_isolated)
        if bad.any():                                          # the result is all padding anyway; only the mask is compared
            o["edge_mask"][bad] = 0
    n_out, e_out = len(o["node_id"]), len(o["edge_id"])
    overflow = n_out + 2 > N_cap or e_out > E_cap or spoiled or bool(bad.any())
    if overflow:
        n_out = e_out = 0
    graph = NS(x=torch.zeros(n_out, 1), edge_index=torch.from_numpy(np.ascontiguousarray(o["edge_index"][:, :e_out])))
    lay = po.collate_padded([graph], [0], capacity)            # the padding rule, and the real edges at offset 0
    assert lay["valid"].tolist() == [n_out, e_out, 1, 0]
    node_id = np.full(N_cap, -1, np.int64)
    out_batch = np.full(N_cap, pad_graph, np.int64)
    edge_id = np.full(E_cap, -1, np.int64)
    node_id[:n_out] = o["node_id"][:n_out]
    out_batch[:n_out] = o["batch"][:n_out]
    edge_id[:e_out] = o["edge_id"][:e_out]
    edge_mask = np.zeros(E, np.uint8)
    edge_mask[:Ev] = o["edge_mask"]
    valid = np.array([0, 0, 0, 1] if overflow else [n_out, e_out, g, 0], np.int64)
    return dict(node_id=node_id, batch=out_batch, edge_id=edge_id, edge_index=lay["edge_index"], edge_mask=edge_mask, valid=valid)


def check_invariants(o, capacity, pad_graph):
    """tests.padded_oracle.check_invariants on an oracle (or device) result: symmetric padding set, no edge between a real and a padding
    node, at least two padding nodes, padding rows marked -1 and owned by ``pad_graph``."""
    valid = np.asarray(o["valid"]).copy()
    valid[2] = pad_graph                                        # check_invariants looks for the padding nodes' graph id there
    po.check_invariants(dict(batch=o["batch"], node_src_row=o["node_id"], edge_index=o["edge_index"], edge_src_slot=o["edge_id"],
                             valid=valid), capacity)


def keep_capacity(E_cap, batch_size, k=None, ratio=None):
    """The derived edge capacity of the explanation side (dp_gsat_amd.replay.keep_capacity), restated."""
    if k is not None:
        return k * batch_size
    return min(E_cap, int(np.ceil(ratio * E_cap)) + batch_size)
