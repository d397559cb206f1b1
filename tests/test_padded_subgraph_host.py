"""not gpu: the oracles of the padded extraction and of the fidelity log vetted on the host -- padding invariants on every oracle output,
the derived keep capacity, the fp64 fidelity oracle against a torch restatement -- and the public surface of the feature."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import fidelity_oracle as fo
from tests import padded_subgraph_oracle as pso
from tests import subgraph_oracle as so
from tests.graphs import random_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gsat_subgraph_padded": 21, "gsat_fidelity_append": 11, "gsat_fidelity_reduce": 6, "gsat_fidelity_reset": 2}
NAMES = ["edge_subgraph_padded", "node_subgraph_padded", "PaddedSubgraphBatch", "FidelityLog", "ReplayedFidelity"]


def _case(seed, G=6):
    ei, batch, N = random_batch(seed, G, 2, 30)
    return ei.numpy(), batch.numpy(), N


def _modes(E, N, rng):
    return [("edge", rng.rand(E) < 0.5, True), ("edge", rng.rand(E) < 0.5, False), ("node", rng.rand(N) < 0.6, False)]


def test_real_part_is_the_unpadded_oracle_and_the_slack_is_inert():
    ei, batch, N = _case(0)
    E, G = ei.shape[1], 6
    rng = np.random.RandomState(0)
    for mode, keep, drop in _modes(E, N, rng):
        ref = so.subgraph_oracle(ei, N, batch, None, keep, mode, drop)
        n, e = ref["counts"]
        for cap in [(n + 2, e), (n + 2, e + 1), (n + 5, e + 9), (n + 2, e + 40), (n + 30, e + 6)]:
            o = pso.subgraph_padded_oracle(ei, N, batch, G, keep, mode, drop, cap)
            assert o["valid"].tolist() == [n, e, G, 0]
            assert np.array_equal(o["node_id"][:n], ref["node_id"]) and np.array_equal(o["edge_id"][:e], ref["edge_id"])
            assert np.array_equal(o["edge_index"][:, :e], ref["edge_index"]) and np.array_equal(o["batch"][:n], ref["batch"])
            assert np.array_equal(o["edge_mask"], ref["edge_mask"])
            assert (o["node_id"][n:] == -1).all() and (o["edge_id"][e:] == -1).all() and (o["batch"][n:] == G).all()
            pso.check_invariants(o, cap, G)


def test_a_padded_input_never_keeps_its_padding_and_never_reads_keep_there():
    ei, batch, N = _case(1)
    E, G = ei.shape[1], 6
    rng = np.random.RandomState(1)
    # the input as a padded batch: 7 padding nodes of graph G, 5 padding edges among them
    pad_ei = np.array([[N, N + 1, N + 1, N + 2, N + 2], [N + 1, N, N + 2, N + 1, N + 2]])
    ei_p = np.concatenate([ei, pad_ei], axis=1)
    batch_p = np.concatenate([batch, np.full(7, G)])
    valid = [N, E, G, 0]
    for mode, keep, drop in _modes(E, N, rng):
        ref = so.subgraph_oracle(ei, N, batch, None, keep, mode, drop)
        n, e = ref["counts"]
        cap = (n + 3, e + 4)
        tail = 5 if mode == "edge" else 7
        for garbage in (np.zeros(tail, bool), np.ones(tail, bool)):
            o = pso.subgraph_padded_oracle(ei_p, N + 7, batch_p, G, np.concatenate([keep, garbage]), mode, drop, cap, valid, pad_graph=G)
            assert o["valid"].tolist() == [n, e, G, 0] and np.array_equal(o["edge_index"][:, :e], ref["edge_index"])
            assert not o["edge_mask"][E:].any() and np.array_equal(o["edge_mask"][:E], ref["edge_mask"])
            pso.check_invariants(o, cap, G)
    # a ragged input: 6 slots of which 4 are filled -- valid[2] is carried, the padding graph is the slot count
    o = pso.subgraph_padded_oracle(ei_p, N + 7, batch_p, G, np.ones(E + 5, bool), "edge", False, (N + 7, E + 5), [N, E, 4, 0], pad_graph=G)
    assert o["valid"].tolist() == [N, E, 4, 0] and (o["batch"][N:] == G).all()
    pso.check_invariants(o, (N + 7, E + 5), G)


def test_overflow_gives_an_all_padding_layout():
    ei, batch, N = _case(2)
    E, G = ei.shape[1], 6
    keep = np.random.RandomState(2).rand(E) < 0.5
    n, e = so.subgraph_oracle(ei, N, batch, None, keep, "edge", True)["counts"]
    bad = ei.copy()
    bad[1, 3] = N
    cases = [(ei, (n + 1, e), None), (ei, (n + 2, e - 1), None), (ei, (n + 2, e), [N, E, G, 1]), (bad, (n + 9, e + 9), None)]
    for edges, cap, valid in cases:
        o = pso.subgraph_padded_oracle(edges, N, batch, G, keep | (edges is bad), "edge", True, cap, valid)
        assert o["valid"].tolist() == [0, 0, 0, 1]
        assert (o["node_id"] == -1).all() and (o["edge_id"] == -1).all() and (o["batch"] == G).all()
        assert o["edge_index"].min(initial=0) >= 0 and o["edge_index"].max(initial=0) < cap[0]
        pso.check_invariants(o, cap, G)
    assert pso.subgraph_padded_oracle(bad, N, batch, G, np.ones(E, bool), "edge", True, (N + 9, E + 9))["edge_mask"][3] == 0


def test_the_derived_keep_capacity_bounds_every_batch_that_fits():
    from dp_gsat_amd.replay import keep_capacity
    rng = np.random.RandomState(3)
    for trial in range(400):
        B = int(rng.randint(1, 33))
        sizes = rng.randint(0, 200, size=int(rng.randint(1, B + 1)))                  # a ragged batch fills 1 .. B slots
        E_cap = int(sizes.sum() + rng.randint(0, 50))
        for ratio in (0.01, 0.3, 1.0 / 3.0, 0.5, 0.999, 1.0):
            cap = keep_capacity(E_cap, B, ratio=ratio)
            assert cap == pso.keep_capacity(E_cap, B, ratio=ratio) == min(E_cap, int(np.ceil(ratio * E_cap)) + B)
            assert int(np.ceil(ratio * sizes.astype(np.float64)).sum()) <= cap, (sizes, E_cap, ratio)
        k = int(rng.randint(1, 20))
        assert keep_capacity(E_cap, B, k=k) == k * B >= int(np.minimum(sizes, k).sum())
    for bad in (dict(), dict(k=3, ratio=0.5)):
        with pytest.raises(ValueError):
            keep_capacity(100, 4, **bad)


@pytest.mark.parametrize("C", [1, 2, 3, 10])
def test_fidelity_oracle_equals_a_torch_restatement(C):
    g = torch.Generator().manual_seed(C)
    full, keep, drop = (torch.randn(65, C, generator=g) * 3 for _ in range(3))
    full[0], full[1] = 0.0, 2.5                                                        # z = 0 / a tie over every class
    cls, p = fo.rows(full.numpy(), keep.numpy(), drop.numpy())
    if C == 1:
        want_cls = [(z[:, 0] >= 0).int() for z in (full, keep, drop)]
        sign = torch.where(full >= 0, 1.0, -1.0).double()
        want_p = [torch.sigmoid(sign * z.double()).view(-1) for z in (full, keep, drop)]
    else:
        want_cls = [z.argmax(dim=1).int() for z in (full, keep, drop)]
        assert want_cls[0][0] == 0 and want_cls[0][1] == 0                             # lowest index on ties
        pick = want_cls[0].long().view(-1, 1)
        want_p = [torch.softmax(z.double(), dim=1).gather(1, pick).view(-1) for z in (full, keep, drop)]
    assert np.array_equal(cls, torch.stack(want_cls, dim=1).numpy())
    assert np.allclose(p, torch.stack(want_p, dim=1).numpy(), rtol=1e-14, atol=0)
    res = fo.compute(cls, p)
    assert res["n"] == 65 and abs(res["fidelity_plus"] - float((want_p[0] - want_p[2]).mean())) < 1e-15
    assert res["flip_minus"] == float((want_cls[1] != want_cls[0]).sum()) / 65
    assert -1.0 <= res["fidelity_minus"] <= 1.0 and 0.0 <= res["flip_plus"] <= 1.0


def test_header_signatures_and_library_agree_on_the_new_symbols():
    import __graft_entry__ as ge
    ge.build()
    from dp_gsat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsat_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert decl, f"{name} is not declared in include/gsat_hip.h"
        assert len(decl.group(1).split(",")) == nargs, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.load().gsat_abi_version() == 4                                         # symbols were only added


def test_names_are_public_and_argument_errors_raise():
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import GsatHipError
    from dp_gsat_amd.synth import Batch
    for name in NAMES:
        assert name in G.__all__ and hasattr(G, name), name
    b = Batch(x=torch.zeros(3, 2), edge_index=torch.tensor([[0, 1, 2], [1, 0, 0]]), batch=torch.zeros(3, dtype=torch.int64), edge_attr=None,
              y=torch.zeros(1, 1), num_graphs=1)
    with pytest.raises(GsatHipError):
        G.edge_subgraph_padded(b, torch.tensor([True, False, True]), (5, 3))
    with pytest.raises(GsatHipError):
        G.node_subgraph_padded(b, torch.tensor([True, False, True]), (5, 3))
    with pytest.raises(ValueError):
        G.edge_subgraph_padded(b, torch.tensor([True, False]), (5, 3))
    with pytest.raises(ValueError):
        G.edge_subgraph_padded(b, torch.tensor([True, False, True]), (1, 3))           # no room for two padding nodes
    with pytest.raises(ValueError):
        G.node_subgraph_padded(b, torch.tensor([0, 2]), (5, 3))                        # an id list has no capacity-shaped form
    with pytest.raises(ValueError):
        G.topk_edge_mask(torch.rand(3), b.edge_index, b.batch)                         # still: exactly one of k and ratio
    # ranked_graphs exists on the fused ranking only: without a declared bound, or forced onto the radix path, it is refused outright
    with pytest.raises(ValueError, match="ranked_graphs"):
        G.topk_edge_mask(torch.rand(3), b.edge_index, b.batch, k=1, ranked_graphs=1)
    with pytest.raises(ValueError, match="ranked_graphs"):
        G.topk_edge_mask(torch.rand(3), b.edge_index, b.batch, ratio=0.5, path="general", ranked_graphs=1)
    with pytest.raises(ValueError, match="general"):
        G.topk_edge_mask(torch.rand(3), b.edge_index, b.batch, k=1, path="general", max_seg_edges=3, ranked_graphs=1)
    with pytest.raises(ValueError):
        G.FidelityLog(-1, 2, "cuda")
    with pytest.raises(ValueError):
        G.FidelityLog(4, 0, "cuda")
