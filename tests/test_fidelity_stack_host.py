"""not gpu: the stack oracle of tests/fidelity_stack_oracle.py against tests/padded_subgraph_oracle.py variant by variant; the C ABI of the
fidelity-curve entry points; what the level lists refuse."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import fidelity_stack_oracle as fso
from tests import padded_subgraph_oracle as pso
from tests.graphs import random_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gsat_fidelity_levels", "gsat_fidelity_stack", "gsat_fidelity_stack_workspace_bytes", "gsat_fidelity_stack_block_items",
               "gsat_fidelity_curve_append", "gsat_fidelity_curve_reduce", "gsat_fidelity_curve_reset")


def _random_input(seed, padded, spoiled=False, bad=False):
    """(edge_index, N, batch, G, valid_in, Gp, N_cap, E_cap, Ev) of a random small batch, unpadded or with slack rows and slots whose
    contents are garbage the oracles must not look at."""
    rng = np.random.RandomState(seed)
    ei, batch, N = random_batch(seed, rng.randint(1, 7), 2, 12)
    ei, batch = ei.numpy(), batch.numpy()
    G, E = int(batch.max()) + 1, ei.shape[1]
    if bad and E:
        ei = ei.copy()
        ei[rng.randint(2), rng.randint(E)] = N + 3
    if not padded:
        return ei, N, batch, G, None, G + 1, N + 2, E, E
    n_slack, e_slack = rng.randint(2, 6), rng.randint(0, 9)
    ei = np.concatenate([ei, rng.randint(0, N + n_slack, size=(2, e_slack))], axis=1)
    batch = np.concatenate([batch, np.full(n_slack, G, np.int64)])
    return ei, N + n_slack, batch, G, [N, E, G, int(spoiled)], G + 1, N + n_slack, E + e_slack, E


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("by_ratio", [False, True])
def test_stack_oracle_equals_the_padded_subgraph_oracle_per_variant(padded, by_ratio):
    for seed in range(12):
        rng = np.random.RandomState(100 + seed)
        S = int(rng.choice([1, 2, 3, 16]))
        ei, N, batch, G, valid_in, Gp, N_cap, E_cap, Ev = _random_input(seed, padded, spoiled=seed == 10, bad=seed == 11)
        levels = sorted(rng.choice(np.arange(1, 40), size=S, replace=False).tolist())
        kw = dict(ratios=[l / 40 for l in levels]) if by_ratio else dict(ks=[int(l) for l in levels])
        # a batch_size below the graph count makes some keep segments too small: those variants overflow on their own
        caps = fso.segment_capacities(E_cap, max(G - (seed % 3 == 2), 1), **kw)
        level = rng.randint(0, S + 1, size=ei.shape[1]).astype(np.uint8)
        level[Ev:] = rng.randint(0, 256, size=ei.shape[1] - Ev)                        # behind the counted edges: never read
        o = fso.stack_oracle(ei, N, batch, G, level, S, caps, N_cap, valid_in, Gp)
        assert o["offsets"] == np.concatenate([[0], np.cumsum(caps)]).tolist() and o["valid"].shape == (2 * S + 1, 4)
        counted = np.minimum(level[:Ev], S)
        full = np.zeros(ei.shape[1], bool)
        for v, mask in enumerate(fso.variant_masks(counted, S)):
            full[:Ev] = mask
            want = pso.subgraph_padded_oracle(ei, N, batch, G, full, "edge", False, (N_cap, caps[v]), valid_in, pad_graph=Gp - 1)
            lo, hi = o["offsets"][v], o["offsets"][v + 1]
            shift = v * N_cap
            assert np.array_equal(o["edge_index"][:, lo:hi], want["edge_index"] + shift), (seed, v)
            assert np.array_equal(o["edge_id"][lo:hi], want["edge_id"]) and np.array_equal(o["valid"][v], want["valid"]), (seed, v)
            if valid_in is None or not want["valid"][3]:       # an overflowed padded input keeps its own batch vector (shared rows)
                assert np.array_equal(o["batch"][shift:shift + N_cap], want["batch"] + v * Gp), (seed, v)
            else:
                assert np.array_equal(o["batch"][shift:shift + N_cap], batch + v * Gp), (seed, v)
        if not o["valid"][:, 3].any():
            real = int(o["valid"][0, 1])
            assert real == Ev and int(o["valid"][:, 1].sum()) == (S + 1) * real          # every edge goes to S + 1 variants
            assert int((o["edge_id"] >= 0).sum()) == (S + 1) * real
        elif seed in (10, 11) and (padded or seed == 11):
            assert (o["valid"] == [0, 0, 0, 1]).all() and (o["edge_id"] == -1).all()


def test_levels_oracle_is_the_count_of_levels_that_do_not_keep_an_edge():
    from tests import explain_oracle as xo
    b = xo.custom_batch([0, 1, 2, 9, 30], seed=3)
    att = np.random.RandomState(5).rand(b.num_edges).astype(np.float32)
    att[::3] = 0.5                                                                     # ties: lower edge id first
    for kw in (dict(ks=[1, 2, 5, 40]), dict(ratios=[0.1, 0.35, 1.0])):
        lv = fso.levels_oracle(att, b.edge_index.numpy(), b.batch.numpy(), 5, **kw)
        S = len(next(iter(kw.values())))
        assert lv.dtype == np.uint8 and lv.max() <= S
        if "ratios" in kw:
            assert lv.max() < S                                                        # ratio 1.0 keeps every edge
        else:
            top1 = xo.rank_oracle(att, b.edge_index.numpy(), b.batch.numpy(), 5, 1)[2].astype(bool)
            assert np.array_equal(lv == 0, top1)


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
    assert int(lib.gsat_fidelity_stack_block_items()) > 0


def test_level_lists_that_are_refused():
    from dp_gsat_amd.explain import check_levels
    assert check_levels(ks=[1, 2, 9]) == ([1, 2, 9], None) and check_levels(ratios=(0.25, 1.0)) == (None, [0.25, 1.0])
    assert check_levels(ks=range(1, 17))[0] == list(range(1, 17))
    for kw in (dict(), dict(ks=[1], ratios=[0.5]), dict(ks=[]), dict(ks=[2, 2]), dict(ks=[3, 1]), dict(ks=[0, 1]), dict(ks=[1.5]),
               dict(ks=list(range(1, 18))), dict(ratios=[0.0, 0.5]), dict(ratios=[0.5, 1.1]), dict(ratios=[0.5, 0.5]), dict(ks=[True])):
        with pytest.raises(ValueError):
            check_levels(**kw)
