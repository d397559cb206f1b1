"""Host tests of the ragged dual/primal work: PackedDataset.budget_batches(..., dual=) against the per-graph restatement of the three-budget
rule in tests/ragged_pair_oracle.py, and the new symbol in the header, the binding and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import dual_oracle as do
from tests import padded_oracle as po
from tests import ragged_oracle as ro
from tests import ragged_pair_oracle as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, CAP = rp.PAIR_SLOTS, rp.PAIR_CAPACITY


@pytest.fixture(scope="module")
def pair():
    import dp_gsat_amd as G
    graphs = do.labelled_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, "cpu")
    return graphs, ds, rp.host_dual_dataset(graphs, ds)


def _check_rule(graphs, rows, perm, cap, slots):
    n, e, d = rp.pair_sizes(graphs)
    got = ro.rows_to_lists(rows)
    want, why = rp.budget_batches(n, e, d, perm, cap, slots)
    assert rows.dtype == torch.int64 and rows.shape[1] == slots
    assert got == want
    assert [g for b in got for g in b] == list(perm), "order is kept and every graph is batched once"
    fits = lambda c: len(c) <= slots and n[c].sum() + 2 <= cap[0] and e[c].sum() <= cap[1] and d[c].sum() <= cap[2]
    for k, b in enumerate(got):
        assert b and fits(b), (k, b)
        if k + 1 < len(got):                                  # maximal: the next batch's first graph would not have fitted
            assert not fits(b + got[k + 1][:1]), (k, b)
    return [len(b) for b in got], why


def test_the_shared_case_binds_every_budget(pair):
    graphs, ds, dual = pair
    n, e, d = rp.pair_sizes(graphs)
    assert int(n[:SLOTS].sum()) == 506 and 506 + 2 > CAP[0], "graphs 0..15 must not fit: the replay constructors have to cope"
    sizes, why = _check_rule(graphs, ds.budget_batches(range(48), CAP, SLOTS, dual=dual), list(range(48)), CAP, SLOTS)
    assert sizes == rp.PAIR_SIZES and sizes[-1] == 1
    assert why == rp.PAIR_CLOSED_BY and set(why) == {"N", "E", "D"}


def test_three_budget_batches_follow_the_rule_on_shuffles(pair):
    graphs, ds, dual = pair
    rng = np.random.RandomState(11)
    bound = ds.pair_capacity_for(dual, SLOTS)
    for cap, slots in [(CAP, SLOTS), (CAP, SLOTS), ((400, 900, 700), SLOTS), ((167, 212, 366), SLOTS), (bound, SLOTS), (bound, 1)]:
        perm = rng.permutation(48)[: int(rng.randint(1, 49))].tolist()
        _check_rule(graphs, ds.budget_batches(torch.tensor(perm), cap, slots, dual=dual), perm, cap, slots)
    assert ds.budget_batches([], CAP, SLOTS, dual=dual).shape == (0, SLOTS)


def test_the_slot_limit_binds_with_four_slots(pair):
    graphs, ds, dual = pair
    sizes, why = _check_rule(graphs, ds.budget_batches(range(48), CAP, 4, dual=dual), list(range(48)), CAP, 4)
    assert max(sizes) == 4 and "S" in why
    bound = ds.pair_capacity_for(dual, 4)
    sizes, why = _check_rule(graphs, ds.budget_batches(range(46), bound, 4, dual=dual), list(range(46)), bound, 4)
    assert sizes == [4] * 11 + [2] and set(why) == {"S"}


def test_a_graph_beyond_the_dual_budget_alone_is_refused(pair):
    graphs, ds, dual = pair
    n, e, d = rp.pair_sizes(graphs)
    g = int(d.argmax())
    assert (g, int(n[g]), int(e[g]), int(d[g])) == (40, 94, 194, 366)
    cap = (CAP[0], CAP[1], 365)                               # its nodes and edges fit
    with pytest.raises(ValueError, match=r"graph 40 .*366 dual edges.*\(320, 620, 365\)"):
        ds.budget_batches(range(48), cap, SLOTS, dual=dual)
    _check_rule(graphs, ds.budget_batches(range(40), cap, SLOTS, dual=dual), list(range(40)), cap, SLOTS)      # the others fit
    with pytest.raises(ValueError, match="graph 27"):
        ds.budget_batches(range(48), (166, 620, 1000), SLOTS, dual=dual)
    with pytest.raises(ValueError, match="E_dual_cap"):
        ds.budget_batches(range(48), CAP[:2], SLOTS, dual=dual)
    import dp_gsat_amd as G
    other = G.PackedDataset.from_data_list(graphs, "cpu")     # node counts are not ds.edge_counts: check_pair runs first
    with pytest.raises(ValueError, match="not a dual"):
        ds.budget_batches(range(48), CAP, SLOTS, dual=other)


def test_without_a_dual_nothing_changes(pair):
    graphs, ds, dual = pair
    n, e = po.sizes(graphs)
    for cap in (ro.RAGGED_CAPACITY, ro.TIGHT_CAPACITY):
        two = ds.budget_batches(range(48), cap, SLOTS)
        assert torch.equal(two, ds.budget_batches(range(48), cap, SLOTS, dual=None))
        assert torch.equal(two, ds.budget_batches(range(48), cap + (10 ** 9,), SLOTS))          # a third entry is not read without a dual
        assert ro.rows_to_lists(two) == ro.budget_batches(n, e, range(48), cap, SLOTS)
        # a dual budget that never binds gives the two-budget batches
        assert torch.equal(two, ds.budget_batches(range(48), cap + (10 ** 9,), SLOTS, dual=dual))
    with pytest.raises(ValueError, match=r"graph 27 \(165 nodes \+ 2 padding nodes, 212 edges\) does not fit the capacity \(N_cap, E_cap\)"):
        ds.budget_batches(range(48), (166, 300), SLOTS)


def test_header_binding_and_library_agree_on_the_pair_scan():
    import __graft_entry__ as ge
    ge.build()
    from dp_gsat_amd import _lib
    name = "gsat_ragged_pair_scan"
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsat_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, name + " is not declared in include/gsat_hip.h"
    kinds = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        kinds.append(_lib.P if "*" in arg else {"int64_t": _lib.I64}[arg.split()[0]])
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.INT and args == kinds and len(args) == 16
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.load().gsat_abi_version() == 4
