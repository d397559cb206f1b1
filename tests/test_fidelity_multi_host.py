"""not gpu: the multi-ranking stack oracle (tests/fidelity_multi_oracle.py) against the single-ranking oracle and the padded subgraph
oracle variant by variant; the overlap counts against sets; the C ABI of the new entry points; which ranking counts are refused."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import fidelity_multi_cases as fc
from tests import fidelity_multi_oracle as fmo
from tests import fidelity_stack_oracle as fso
from tests import padded_subgraph_oracle as pso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gsat_fidelity_stack_multi", "gsat_fidelity_stack_multi_workspace_bytes", "gsat_level_overlap", "gsat_level_overlap_reset")


@pytest.mark.parametrize("E", [0, 1, 61, 300])
@pytest.mark.parametrize("R,S", [(1, 3), (2, 1), (3, 5), (2, 8)])
@pytest.mark.parametrize("padded", [False, True])
def test_variant_r_s_is_the_single_oracles_variant_s_of_ranking_r(E, R, S, padded):
    ks = list(range(2, 2 + 3 * S, 3))
    levels, ei, batch, counts = fc.ranking_levels(E, R, ks, seed=S)
    G, N = len(counts), len(batch)
    valid_in, Gp, N_cap = None, G + 1, N + 2
    if padded:                                             # slack rows and slots whose contents the oracles must not look at
        rng = np.random.RandomState(E + R)
        ei = np.concatenate([ei, rng.randint(0, N + 4, size=(2, 5))], axis=1)
        levels = np.concatenate([levels, rng.randint(0, 256, size=(R, 5)).astype(np.uint8)], axis=1)
        batch = np.concatenate([batch, np.full(4, G, np.int64)])
        valid_in, N_cap, N = [N, E, G, 0], N + 4, N + 4
    caps = fmo.segment_capacities(ei.shape[1], max(G - 1, 1), R, ks=ks)          # one graph short: some keep segments overflow alone
    o = fmo.stack_oracle(ei, N, batch, G, levels, S, caps, N_cap, valid_in, Gp)
    assert o["valid"].shape == (1 + 2 * R * S, 4) and o["offsets"][-1] == sum(caps)
    for r in range(R):
        place = [0] + [fmo.variant_index(R, S, r, s, True) for s in range(S)] + [fmo.variant_index(R, S, r, s, False) for s in range(S)]
        one = fso.stack_oracle(ei, N, batch, G, levels[r], S, [caps[v] for v in place], N_cap, valid_in, Gp)
        masks = fso.variant_masks(levels[r][:E], S)
        for u, v in enumerate(place):
            lo, hi = o["offsets"][v], o["offsets"][v + 1]
            slo, shi = one["offsets"][u], one["offsets"][u + 1]
            assert np.array_equal(o["edge_index"][:, lo:hi] - v * N_cap, one["edge_index"][:, slo:shi] - u * N_cap), (r, u)
            assert np.array_equal(o["edge_id"][lo:hi], one["edge_id"][slo:shi]) and np.array_equal(o["valid"][v], one["valid"][u]), (r, u)
            assert np.array_equal(o["batch"][v * N_cap:(v + 1) * N_cap] - v * Gp, one["batch"][u * N_cap:(u + 1) * N_cap] - u * Gp), (r, u)
            full = np.zeros(ei.shape[1], bool)
            full[:E] = masks[u]
            want = pso.subgraph_padded_oracle(ei, N, batch, G, full, "edge", False, (N_cap, caps[v]), valid_in, pad_graph=Gp - 1)
            assert np.array_equal(o["edge_index"][:, lo:hi], want["edge_index"] + v * N_cap), (r, u)
            assert np.array_equal(o["edge_id"][lo:hi], want["edge_id"]) and np.array_equal(o["valid"][v], want["valid"]), (r, u)
    if R == 3:                                             # rankings 0 and 2 are equal: so are their variants, up to the offsets
        for s in range(S):
            for keep in (True, False):
                a, b = fmo.variant_index(R, S, 0, s, keep), fmo.variant_index(R, S, 2, s, keep)
                assert np.array_equal(o["edge_id"][o["offsets"][a]:o["offsets"][a + 1]], o["edge_id"][o["offsets"][b]:o["offsets"][b + 1]])
    if R >= 2 and E >= 300:                                # a ranking and its reverse keep disjoint sets at the smallest level
        a = o["edge_id"][o["offsets"][1]:o["offsets"][2]]
        b = o["edge_id"][o["offsets"][1 + S]:o["offsets"][2 + S]]
        big = np.repeat(np.asarray(counts), counts) >= 2 * ks[0]
        assert not (set(a[a >= 0][big[a[a >= 0]]]) & set(b[b >= 0][big[b[b >= 0]]]))


@pytest.mark.parametrize("E", fc.EDGE_COUNTS)
@pytest.mark.parametrize("S", [1, 5, 16])
def test_overlap_counts_equal_the_intersection_of_the_kept_sets(E, S):
    rng = np.random.RandomState(E + S)
    a = rng.randint(0, S + 1, size=E).astype(np.uint8)
    b = np.where(rng.rand(E) < 0.5, a, rng.randint(0, S + 1, size=E)).astype(np.uint8)
    for count in (None, E // 2, E + 5, -1):
        got, want = fmo.overlap_counts(a, b, S, count), fmo.overlap_counts_by_sets(a, b, S, count)
        assert got.shape == (S, 3) and np.array_equal(got, want), (E, S, count)
    c = fmo.overlap_counts(a, a, S)
    assert np.array_equal(c[:, 0], c[:, 1]) and np.array_equal(c[:, 1], c[:, 2]) and (np.diff(c[:, 0]) >= 0).all()
    assert int(c[-1, 1]) == int((a < S).sum())                                      # level S -- in no level -- is never counted


def test_ranking_counts_that_are_refused():
    from dp_gsat_amd.explain import check_levels, check_rankings
    for R, S in ((1, 16), (2, 8), (4, 4), (16, 1), (3, 5)):
        assert check_rankings(R, S) == R
        assert len(check_levels(ks=range(1, S + 1))[0]) == S
    for R, S in ((17, 1), (2, 9), (3, 6), (0, 1), (-1, 2), (1.5, 2), (True, 2)):
        with pytest.raises(ValueError):
            check_rankings(R, S)
    with pytest.raises(ValueError):
        check_levels(ks=range(1, 18))                                               # R = 1, S = 17


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
            want = _lib.P if "*" in a else {"int64_t": _lib.I64, "size_t": _lib.SZ, "int": _lib.INT}[a.split()[0]]
            assert c is want, (name, a, c)
        assert res is {"int": _lib.INT, "size_t": _lib.SZ}[m.group(1)], name
    assert _lib.load().gsat_abi_version() == 4
    ws = lib.gsat_fidelity_stack_multi_workspace_bytes
    ws.restype, ws.argtypes = ctypes.c_size_t, [ctypes.c_int64] * 3
    assert ws(2049, 2, 8) > 0 and ws(2049, 16, 1) > 0 and ws(2049, 17, 1) == 0 and ws(2049, 2, 9) == 0 and ws(2049, 0, 1) == 0
