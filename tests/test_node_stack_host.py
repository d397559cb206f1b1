"""not gpu: the invariants of tests/node_stack_oracle.py -- nested levels, keep-variant nodes plus drop-variant nodes = the real nodes,
an edge in at most one of the two --, the ranking rule on ties and signed zeros, and the C ABI of gsat_fidelity_stack_nodes."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import node_stack_oracle as nso
from tests.graphs import random_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gsat_fidelity_stack_nodes", "gsat_fidelity_stack_nodes_workspace_bytes")


def _random_input(seed, padded):
    rng = np.random.RandomState(seed)
    ei, batch, N = random_batch(seed, rng.randint(1, 7), 1, 12)
    ei, batch = ei.numpy(), batch.numpy()
    G, E = int(batch.max()) + 1, ei.shape[1]
    if not padded:
        return ei, N, batch, G, None, G + 1, N + 2, E
    n_slack, e_slack = rng.randint(2, 6), rng.randint(0, 9)
    ei = np.concatenate([ei, rng.randint(0, N + n_slack, size=(2, e_slack))], axis=1)
    batch = np.concatenate([batch, np.full(n_slack, G, np.int64)])
    return ei, N + n_slack, batch, G, [N, E, G, 0], G + 1, N + n_slack, E


def test_ranking_rule_higher_first_lower_id_on_ties_signed_zeros_equal():
    att = np.array([0.5, -0.0, 0.0, 0.5, 0.25, 0.0, -0.0, 1.0], np.float32)
    batch = np.array([0, 0, 0, 0, 0, 1, 1, 1])
    order, rank, ptr = nso.rank_nodes_oracle(att, batch, 2)
    assert order.tolist() == [0, 3, 4, 1, 2, 7, 5, 6] and ptr.tolist() == [0, 5, 8]
    assert rank.tolist() == [0, 3, 4, 1, 2, 1, 2, 0]
    assert nso.topk_node_mask_oracle(att, batch, 2, k=2).tolist() == [True, False, False, True, False, True, False, True]
    assert nso.topk_node_mask_oracle(att, batch, 2, ratio=0.5).tolist() == [True, False, False, True, True, True, False, True]
    assert nso.topk_node_mask_oracle(att, batch, 1, k=9).tolist() == [True] * 5 + [False] * 3          # an unranked graph keeps nothing
    lab = np.array([1, 0, 0, 0, 1, 1, 0, 0])                                               # best three: 0, 3, 4 and 7, 5, 6
    assert nso.node_precision_oracle(att, lab, 3, batch, 2).tolist() == [np.float32(2 / 3), np.float32(1 / 3)]


@pytest.mark.parametrize("by_ratio", [False, True])
def test_levels_are_nested_and_equal_the_masks(by_ratio):
    for seed in range(8):
        rng = np.random.RandomState(seed)
        _, N, batch, G, *_ = _random_input(seed, False)
        att = (np.round(rng.rand(N) * 4) / 4).astype(np.float32)
        kw = dict(ratios=[0.2, 0.5, 1.0]) if by_ratio else dict(ks=[1, 3, 50])
        lv = nso.node_levels_oracle(att, batch, G, **kw)
        for s, l in enumerate(next(iter(kw.values()))):
            one = dict(ratio=l) if by_ratio else dict(k=l)
            assert np.array_equal(lv <= s, nso.topk_node_mask_oracle(att, batch, G, **one)), (seed, s)
        assert lv.max() < 3                                                            # ratio 1.0 / k = 50 keeps every node


@pytest.mark.parametrize("padded", [False, True])
def test_stack_oracle_invariants(padded):
    for seed in range(10):
        rng = np.random.RandomState(50 + seed)
        S = int(rng.choice([1, 3, 16]))
        ei, N, batch, G, valid_in, Gp, N_cap, Ev = _random_input(seed, padded)
        Nv = N if valid_in is None else valid_in[0]
        level = rng.randint(0, S + 2, size=N).astype(np.uint8)                         # S + 1 counts as S
        E = ei.shape[1]
        o = nso.node_stack_oracle(ei, N, batch, G, level, S, [E] * (2 * S + 1), N_cap, valid_in, Gp)
        assert not o["valid"][:, 3].any() and o["valid"][0].tolist() == [Nv, Ev, G, 0], seed
        nid = o["node_id"].reshape(2 * S + 1, N_cap)
        eid = o["edge_id"].reshape(2 * S + 1, E)
        assert np.array_equal(nid[0][:Nv], np.arange(Nv)) and (nid[0][Nv:] == -1).all()
        for s in range(S):
            keep, drop = nid[1 + s], nid[1 + S + s]
            both = np.sort(np.concatenate([keep[keep >= 0], drop[drop >= 0]]))
            assert np.array_equal(both, np.arange(Nv)), (seed, s)                      # keep nodes + drop nodes = the real nodes
            ke, de = eid[1 + s], eid[1 + S + s]
            assert not np.intersect1d(ke[ke >= 0], de[de >= 0]).size, (seed, s)        # an edge is in at most one of the two
            if s:
                assert np.isin(nid[s][nid[s] >= 0], keep).all() and np.isin(eid[s][eid[s] >= 0], ke).all(), (seed, s)          # nested
            # an edge is kept iff both ends are
            kept_nodes = np.zeros(N, bool)
            kept_nodes[keep[keep >= 0]] = True
            want = np.nonzero(kept_nodes[ei[0, :Ev]] & kept_nodes[ei[1, :Ev]])[0]
            assert np.array_equal(ke[ke >= 0], want), (seed, s)
            assert o["valid"][1 + s, 0] + o["valid"][1 + S + s, 0] == Nv


def test_header_declares_the_new_symbols_and_signatures_match():
    import __graft_entry__ as ge
    ge.build()
    from dp_gsat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsat_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/gsat_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        args = [a.strip() for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        res, sig = _lib.SIGNATURES[name]
        assert len(sig) == len(args), (name, len(sig), args)
        for a, c in zip(args, sig):
            want = _lib.P if "*" in a else {"int64_t": _lib.I64, "size_t": _lib.SZ, "int": _lib.INT, "double": _lib.F64}[a.split()[0]]
            assert c is want, (name, a, c)
        assert res is {"int": _lib.INT, "int64_t": _lib.I64, "size_t": _lib.SZ}[m.group(1)], name
    assert _lib.load().gsat_abi_version() == 4
    size = _lib.load().gsat_fidelity_stack_nodes_workspace_bytes
    assert int(size(10, 10, 0)) == 0 and int(size(10, 10, 17)) == 0 and int(size(1 << 31, 10, 3)) == 0 and int(size(10, -1, 3)) == 0
    assert int(size(5000, 9000, 16)) >= 5000 * 17 * 4


def test_public_names_are_exported():
    import dp_gsat_amd as G
    for name in ("rank_nodes", "topk_node_mask", "node_levels", "node_precision_at_k", "explanation_node_subgraph", "explanation_stack_nodes",
                 "explanation_node_fidelity_curve", "NodeRanking"):
        assert hasattr(G, name) and name in G.__all__, name
