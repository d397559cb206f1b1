"""gpu: ``connectivity=True`` of ReplayedFidelityCurve and ReplayedDualFidelityCurve -- the four connectivity lists against
tests/components_oracle.py run on the levels and batches the replays publish, accumulated over the epoch; every other returned value
bitwise what ``connectivity=False`` returns; the training run left bitwise alone; the refusal of ``unit="node"``."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import components_oracle as co
from tests.replay import pin_seed_stream
from tests.test_gpu_dual_eval import BASE, MIX, _set_counter
from tests.test_gpu_dual_replay import _dual_gsat, _pair_datasets
from tests.test_gpu_eval_log import _training_state
from tests.test_gpu_replayed_fidelity import IDS, SLOTS, _graphs, _gsat
from tests.test_gpu_replayed_fidelity_curve import _ragged_capacity

pytestmark = pytest.mark.gpu
KEYS = ("components", "largest_edge_share", "largest_node_share", "connected_fraction")
RATIOS = [0.3, 0.7, 1.0]
DUAL_BATCH, DUAL_RATIOS = 5, [0.2, 0.5, 0.8]
DUAL_IDS = [3, 7, 0, 9, 5, 1, 11, 4, 8, 2]                 # two full batches
DUAL_TAIL = DUAL_IDS + [6, 10]                             # and a tail of two


def _padded_counts(b, level, S, bound):
    """The oracle's accumulator for one published padded batch and one level row."""
    Gp = int(b.num_graphs)
    return co.batch_components(b.edge_index.cpu().numpy(), b.batch.cpu().numpy(), Gp, level.cpu().numpy(), S, bound, Gp - 1,
                               b.valid.tolist())["acc"]


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed-with-tail", "ragged"])
def test_single_curve_equals_the_oracle_and_leaves_the_curve_alone(dev, ragged):
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat, _ = _gsat(dev, "GIN", True, graphs)
    capacity = _ragged_capacity(graphs) if ragged else None
    S, bound = len(RATIOS), int(ds.node_counts.max())
    off = G.ReplayedFidelityCurve(gsat, ds, SLOTS, ratios=RATIOS, capacity=capacity, ragged=ragged)
    on = G.ReplayedFidelityCurve(gsat, ds, SLOTS, ratios=RATIOS, capacity=capacity, ragged=ragged, connectivity=True)
    assert off.components is None and tuple(on.components.shape) == (S, 8) and not on.components.any()
    plain, got = off.run(np.asarray(IDS)), on.run(np.asarray(IDS))
    assert set(got) == set(plain) | set(KEYS)
    for key in plain:
        assert got[key] == plain[key], key                                             # bitwise: lists of Python floats
    assert on.run(np.asarray(IDS)) == got and not on.overflowed()
    if ragged:
        rows = [[int(i) for i in row.tolist() if i >= 0] for row in on.batches(IDS)]
        replayed = [True] * len(rows)
    else:
        rows = [IDS[s:s + SLOTS] for s in range(0, len(IDS), SLOTS)]
        replayed = [len(r) == SLOTS for r in rows]
        assert replayed == [True, True, False]
    acc = np.zeros((S, 8), np.int64)
    for row, is_replay in zip(rows, replayed):
        if is_replay:
            on.step(row, 0)
            assert on.batch.valid.tolist()[2:] == [len(row), 0]
            acc += _padded_counts(on.batch, on.edge_level, S, bound)
        else:
            ub = ds.collate(torch.tensor(row, device=dev))
            gsat.eval()                                                                # the eager tail, through the code run() takes
            _, stack, _ = on._forward(ub, 0)
            gsat.train()
            acc += co.batch_components(ub.edge_index.cpu().numpy(), ub.batch.cpu().numpy(), len(row), stack.edge_level.cpu().numpy(), S)["acc"]
    want = co.scores(acc)
    assert acc[0, 0] == len(IDS) and acc[0, 7] == 0 and (acc[:, 0] == len(IDS)).all()
    for key in KEYS:
        assert got[key] == want[key], (key, got[key], want[key])
    assert got["largest_edge_share"][-1] <= 1.0 and got["components"][-1] >= 1.0      # ratio 1.0 keeps every edge of every graph
    with pytest.raises(ValueError, match="unit='edge' only"):
        G.ReplayedFidelityCurve(gsat, ds, SLOTS, ratios=RATIOS, unit="node", connectivity=True)
    G.clear_cache()


@pytest.mark.parametrize("ragged", [False, True], ids=["fixed", "ragged"])
def test_dual_curve_equals_the_oracle_unmixed_and_mixed(dev, ragged):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=12)
    _, _, dg, _ = _dual_gsat(dev, "GIN", graphs, False, **MIX)
    S, bound = len(DUAL_RATIOS), int(ds.node_counts.max())
    kw = dict(ratios=DUAL_RATIOS, seed=BASE, ragged=ragged, capacity=ds.pair_capacity_for(dual, 3) if ragged else None)
    off = G.ReplayedDualFidelityCurve(dg, ds, dual, DUAL_BATCH, **kw)
    on = G.ReplayedDualFidelityCurve(dg, ds, dual, DUAL_BATCH, connectivity=True, **kw)
    assert off.components is None and tuple(on.components.shape) == (2, S, 8) and not on.components.any()
    for epoch in (0, 2):                                                               # mix_after_epoch = 1: epoch 2 replays the mixed graph
        plain, got = off.run(DUAL_TAIL, epoch), on.run(DUAL_TAIL, epoch)
        assert set(got) == set(plain)
        for key in plain:
            if key in ("primal", "dual"):
                assert set(got[key]) == set(plain[key]) | set(KEYS)
                assert all(got[key][k] == plain[key][k] for k in plain[key]), (epoch, key)
            else:
                assert got[key] == plain[key], (epoch, key)
        assert on.run(DUAL_TAIL, epoch) == got
        # the oracle on what the replays of the full batches publish; the same seed words as run() drew
        ids = DUAL_TAIL if ragged else DUAL_IDS
        got = on.run(ids, epoch)
        rows = list(on.batches(torch.tensor(ids))) if ragged else [ids[s:s + DUAL_BATCH] for s in range(0, len(ids), DUAL_BATCH)]
        acc = np.zeros((2, S, 8), np.int64)
        for j, row in enumerate(rows):
            _set_counter(on, (epoch << 32) + j)
            on.step(row, epoch)
            filled = int((torch.as_tensor(row) >= 0).sum())
            assert tuple(on.edge_level.shape[:1]) == (2,) and on.batch.valid.tolist()[2:] == [filled, 0]
            for r in range(2):
                acc[r] += _padded_counts(on.batch, on.edge_level[r], S, bound)
        assert (acc[:, :, 0] == len(ids)).all() and not acc[:, 0, 7].any()
        for r, name in enumerate(("primal", "dual")):
            want = co.scores(acc[r])
            for key in KEYS:
                assert got[name][key] == want[key], (epoch, name, key, got[name][key], want[key])
    G.clear_cache()


def test_a_connectivity_epoch_does_not_disturb_dual_training(dev):
    """Three ReplayedDualStep steps (the third on the mixed graph) with a connectivity curve epoch after each, and the same steps
    without: parameters, BatchNorm buffers, both Adam states, the device seed stream and torch's CUDA generator end bitwise equal."""
    import dp_gsat_amd as G
    from tests.replay import seed_state
    graphs, ds, dual = _pair_datasets(dev, count=12)
    train_ids = [[4, 5, 6, 10, 1], DUAL_IDS[:5], DUAL_IDS[5:]]
    runs = []
    for with_curve in (True, False):
        torch.manual_seed(99)
        _, _, dg, opts = _dual_gsat(dev, "GIN", graphs, True, **MIX)
        rs = G.ReplayedDualStep(dg, ds, dual, DUAL_BATCH)
        ev = G.ReplayedDualFidelityCurve(dg, ds, dual, DUAL_BATCH, ratios=DUAL_RATIOS, connectivity=True) if with_curve else None
        pin_seed_stream(dev, 0x5EED)
        for epoch, ids in enumerate(train_ids):
            rs.step(ids, epoch)
            if ev is not None:
                cpu_rng = torch.get_rng_state()
                res = ev.run(np.asarray(DUAL_TAIL), epoch)
                assert len(res["primal"]["components"]) == 3 and dg.training and torch.equal(torch.get_rng_state(), cpu_rng)
        torch.cuda.synchronize()
        state = {}
        for side, opt in (("primal", opts[0]), ("dual", opts[1])):
            got, _ = _training_state(NS(optimizer=opt, named_parameters=dg.named_parameters, named_buffers=dg.named_buffers), dev)
            state.update({side + "." + k if k.startswith("adam.") else k: v for k, v in got.items()})
        runs.append((state, seed_state(dev), torch.cuda.get_rng_state()))
    (a, seed_a, cuda_a), (b, seed_b, cuda_b) = runs
    assert set(a) == set(b) and any(k.startswith("primal.adam.") for k in a)
    assert seed_a == seed_b and seed_a[1] > 0 and torch.equal(cuda_a, cuda_b)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()
