"""Host tests of the ragged-batch work: PackedDataset.budget_batches against the numpy restatement of its rule, and the fp64 criterion
oracle of tests/ragged_oracle.py against torch.nn.functional on the [:b] slice."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import padded_oracle as po
from tests import ragged_oracle as ro


@pytest.fixture(scope="module")
def step_dataset():
    import dp_gsat_amd as G
    graphs = po.mutag_graphs(**po.STEP_GRAPHS)
    return graphs, G.PackedDataset.from_data_list(graphs, "cpu")


def _check_rule(graphs, rows, perm, cap, slots):
    n, e = po.sizes(graphs)
    got = ro.rows_to_lists(rows)
    assert rows.dtype == torch.int64 and rows.shape[1] == slots
    assert got == ro.budget_batches(n, e, perm, cap, slots)
    assert [g for b in got for g in b] == list(perm), "order is kept and every graph is batched once"
    for k, b in enumerate(got):
        assert 1 <= len(b) <= slots and n[b].sum() + 2 <= cap[0] and e[b].sum() <= cap[1], (k, b)
        if k + 1 < len(got):                                  # maximal: the next batch's first graph would not have fitted
            c = b + got[k + 1][:1]
            assert len(c) > slots or n[c].sum() + 2 > cap[0] or e[c].sum() > cap[1], (k, b)
    return [len(b) for b in got]


@pytest.mark.parametrize("cap,count,sizes", [(ro.RAGGED_CAPACITY, 48, ro.RAGGED_SIZES), (ro.TIGHT_CAPACITY, 48, ro.TIGHT_SIZES),
                                             ((900, 1726), 48, [16, 16, 16]), ((900, 1726), 40, [16, 16, 8])])
def test_budget_batches_follow_the_rule(step_dataset, cap, count, sizes):
    graphs, ds = step_dataset
    perm = list(range(count))
    assert _check_rule(graphs, ds.budget_batches(perm, cap, ro.RAGGED_SLOTS), perm, cap, ro.RAGGED_SLOTS) == sizes


def test_budget_batches_bound_capacity_and_shuffles(step_dataset):
    graphs, ds = step_dataset
    n, e = po.sizes(graphs)
    assert po.capacity_for(n, e, 16) == ds.capacity_for(16) == (900, 1726)
    rng = np.random.RandomState(5)
    for cap, slots in [(ro.RAGGED_CAPACITY, 16), (ro.TIGHT_CAPACITY, 16), ((167, 212), 16), ((400, 900), 3), ((900, 1726), 1)]:
        perm = rng.permutation(48)[: int(rng.randint(1, 49))].tolist()
        _check_rule(graphs, ds.budget_batches(torch.tensor(perm), cap, slots), perm, cap, slots)
    assert ds.budget_batches([], ro.RAGGED_CAPACITY, 16).shape == (0, 16)


def test_budget_batches_refuse_a_graph_that_fits_no_batch(step_dataset):
    graphs, ds = step_dataset
    n, e = po.sizes(graphs)
    assert int(n.argmax()) == 27 and (int(n[27]), int(e[27])) == (165, 212)
    with pytest.raises(ValueError, match="graph 27"):
        ds.budget_batches(range(48), (166, 300), 16)
    with pytest.raises(ValueError, match="graph 27"):
        ds.budget_batches(range(48), (300, 211), 16)
    with pytest.raises(ValueError):
        ds.budget_batches([48], ro.RAGGED_CAPACITY, 16)


def test_budget_batches_do_not_walk_the_graphs_in_python():
    """A 4337-graph epoch (Mutagenicity's size): the numpy restatement takes one Python step per graph, budget_batches one per batch."""
    import dp_gsat_amd as G
    rng = np.random.RandomState(0)
    n = rng.randint(5, 60, 4337)
    e = 2 * n + rng.randint(0, 8, 4337)
    zero = torch.zeros(1, dtype=torch.int64)
    ds = G.PackedDataset(torch.zeros(int(n.sum()), 1), torch.zeros(2, int(e.sum()), dtype=torch.int64),
                         torch.cat([zero, torch.from_numpy(n).cumsum(0)]), torch.cat([zero, torch.from_numpy(e).cumsum(0)]),
                         torch.zeros(4337, 1))
    perm = rng.permutation(4337)
    ds.budget_batches(perm[:10], (4000, 9000), 128)            # the one host copy of the sizes
    t0 = time.perf_counter()
    rows = ds.budget_batches(perm, (4000, 9000), 128)
    t1 = time.perf_counter()
    want = ro.budget_batches(n, e, perm.tolist(), (4000, 9000), 128)
    t2 = time.perf_counter()
    assert ro.rows_to_lists(rows) == want and len(want) < 60
    assert t1 - t0 < t2 - t1, f"budget_batches {t1 - t0:.4f} s, one Python step per graph {t2 - t1:.4f} s"


@pytest.mark.parametrize("b", [None, 1, 37, 63, 64])
def test_criterion_oracle_matches_torch_on_the_slice(b):
    G = 64
    s = slice(None) if b is None else slice(0, b)
    z, y = ro.criterion_case(G, 1, 0, 1)
    assert abs(float(ro.criterion64(z, y, 0, b)) - float(F.binary_cross_entropy_with_logits(z[s].double(), y[s].double()))) < 1e-12
    for C in (2, 3, 7, 130):
        z, y = ro.criterion_case(G, C, 1, C)
        assert abs(float(ro.criterion64(z, y, 1, b)) - float(F.cross_entropy(z[s].double(), y[s].long()))) < 1e-12
    for C in (1, 12):
        z, y = ro.criterion_case(G, C, 2, C)
        full = y == y
        assert 0.5 < float(full.float().mean()) < 0.8 and not full[G // 2].any() and (C == 1 or not full[:, C - 1].any())
        zs, ys = z[s].double(), y[s].double()
        lab = ys == ys
        if lab.any():
            assert abs(float(ro.criterion64(z, y, 2, b)) - float(F.binary_cross_entropy_with_logits(zs[lab], ys[lab]))) < 1e-12
        else:                                                 # torch's mean over nothing is NaN; the clamped divisor gives 0
            assert float(ro.criterion64(z, y, 2, b)) == 0.0


def test_criterion_oracle_gradient_and_empty_selection():
    z, y = ro.criterion_case(9, 12, 2, 3)
    for mode, (zz, yy) in ((0, ro.criterion_case(9, 1, 0, 3)), (1, ro.criterion_case(9, 5, 1, 3)), (2, (z, y))):
        a = zz.double().requires_grad_(True)
        ro.criterion64(a, yy, mode, 4).backward()
        assert not a.grad[4:].any() and a.grad[:4].any()
        assert float(ro.criterion64(zz, yy, mode, 0)) == 0.0
    assert torch.isfinite(ro.criterion64(*ro.criterion_case(64, 1, 0, 1), 0))
