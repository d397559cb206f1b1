"""not gpu: identities of the CPU oracle the GPU subgraph tests compare against, the public surface of dp_gsat_amd.subgraph and its
error convention."""
import numpy as np
import pytest
import torch

from tests import subgraph_oracle as so
from tests.graphs import random_batch

NAMES = ["edge_subgraph", "node_subgraph", "explanation_subgraph", "explanation_fidelity", "gather_rows", "SubgraphBatch"]


def _case(seed, G=7):
    ei, batch, N = random_batch(seed, G, 2, 40)
    return ei.numpy(), batch.numpy(), N, so.node_ptr_of(batch.numpy(), G)


def test_all_true_mask_is_the_identity():
    ei, batch, N, ptr = _case(0)
    E = ei.shape[1]
    for mode, keep, drop in (("edge", np.ones(E), False), ("node", np.ones(N), False)):
        o = so.subgraph_oracle(ei, N, batch, ptr, keep, mode, drop)
        assert np.array_equal(o["node_id"], np.arange(N)) and np.array_equal(o["edge_id"], np.arange(E))
        assert np.array_equal(o["edge_index"], ei) and np.array_equal(o["batch"], batch) and np.array_equal(o["node_ptr"], ptr)
        assert o["edge_mask"].all() and o["counts"] == (N, E)


def test_relabelling_is_strictly_monotone_and_inverts_node_id():
    ei, batch, N, ptr = _case(1)
    keep = np.random.RandomState(1).rand(N) < 0.6
    o = so.subgraph_oracle(ei, N, batch, ptr, keep, "node")
    assert np.all(np.diff(o["node_id"]) > 0) and np.all(np.diff(o["edge_id"]) > 0)
    assert np.array_equal(o["node_id"][o["edge_index"]], ei[:, o["edge_id"]])         # new ids map back to the old endpoints
    assert o["edge_index"].max(initial=-1) < len(o["node_id"])


def test_edge_mode_drop_isolated_keeps_only_touched_nodes():
    ei, batch, N, ptr = _case(2)
    keep = np.random.RandomState(2).rand(ei.shape[1]) < 0.4
    o = so.subgraph_oracle(ei, N, batch, ptr, keep, "edge", True)
    touched = np.zeros(len(o["node_id"]), dtype=bool)
    touched[o["edge_index"].reshape(-1)] = True
    assert touched.all() and len(o["node_id"]) < N
    all_nodes = so.subgraph_oracle(ei, N, batch, ptr, keep, "edge", False)
    assert np.array_equal(all_nodes["node_id"], np.arange(N)) and np.array_equal(all_nodes["edge_index"], ei[:, keep])
    assert np.array_equal(all_nodes["edge_id"], o["edge_id"])


def test_node_mode_equals_edge_mode_on_the_induced_mask():
    ei, batch, N, ptr = _case(3)
    keep = np.random.RandomState(3).rand(N) < 0.7
    node = so.subgraph_oracle(ei, N, batch, ptr, keep, "node")
    edge = so.subgraph_oracle(ei, N, batch, ptr, keep[ei[0]] & keep[ei[1]], "edge", False)
    assert np.array_equal(node["edge_id"], edge["edge_id"]) and np.array_equal(node["edge_mask"], edge["edge_mask"])
    # edge mode kept every node: restricted to the kept ones, its endpoints are node mode's relabelled by rank
    rank = np.cumsum(keep) - 1
    assert np.array_equal(rank[edge["edge_index"]], node["edge_index"])


def test_node_ptr_is_consistent_with_batch_also_for_emptied_graphs():
    ei, batch, N, ptr = _case(4, G=9)
    keep = np.random.RandomState(4).rand(N) < 0.5
    keep[(batch == 3) | (batch == 8)] = False                                           # a graph in the middle and the last one
    o = so.subgraph_oracle(ei, N, batch, ptr, keep, "node")
    assert len(o["node_ptr"]) == 10 and o["node_ptr"][-1] == len(o["node_id"])
    assert np.array_equal(np.diff(o["node_ptr"]), np.bincount(o["batch"], minlength=9))
    assert o["node_ptr"][3] == o["node_ptr"][4] and o["node_ptr"][8] == o["node_ptr"][9]


def test_subgraph_names_are_public_and_symbols_bound():
    import dp_gsat_amd as G
    from dp_gsat_amd import _lib
    for name in NAMES:
        assert name in G.__all__ and hasattr(G, name), name
    for sym in ("gsat_subgraph_index", "gsat_subgraph_workspace_bytes", "gsat_subgraph_block_items", "gsat_gather_rows"):
        assert sym in _lib.SIGNATURES, sym


def _cpu_batch():
    from dp_gsat_amd.synth import Batch
    ei = torch.tensor([[0, 1, 2], [1, 0, 0]])
    return Batch(x=torch.zeros(3, 2), edge_index=ei, batch=torch.zeros(3, dtype=torch.int64), edge_attr=None, y=torch.zeros(1, 1), num_graphs=1)


def test_cpu_tensors_raise():
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import GsatHipError
    b = _cpu_batch()
    with pytest.raises(GsatHipError):
        G.edge_subgraph(b, torch.tensor([True, False, True]))
    with pytest.raises(GsatHipError):
        G.node_subgraph(b, torch.tensor([True, False, True]))
    with pytest.raises(GsatHipError):
        G.node_subgraph(b, torch.tensor([0, 2]))
    with pytest.raises(GsatHipError):
        G.explanation_subgraph(torch.rand(3), b, k=1)
    with pytest.raises(GsatHipError):
        G.gather_rows(torch.zeros(3, 2), torch.tensor([0]))
    clf = G.get_model(2, 0, 2, False, dict(model_name="GIN", n_layers=1, hidden_size=8, dropout_p=0.0), "cpu").train()
    with pytest.raises(GsatHipError):
        G.explanation_fidelity(clf, b, torch.rand(3), k=1)
    assert clf.training                                                                # the mode is restored on the way out


def test_argument_errors_raise_value_error():
    import dp_gsat_amd as G
    b = _cpu_batch()
    with pytest.raises(ValueError):
        G.explanation_subgraph(torch.rand(3), b)
    with pytest.raises(ValueError):
        G.explanation_subgraph(torch.rand(3), b, k=1, ratio=0.5)
    with pytest.raises(ValueError):
        G.explanation_subgraph(torch.rand(4), b, k=1)
    with pytest.raises(ValueError):
        G.edge_subgraph(b, torch.tensor([True, False]))
    with pytest.raises(ValueError):
        G.node_subgraph(b, torch.tensor([True, False, True, True]))
