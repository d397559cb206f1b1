"""-m gpu: the training pass logs itself -- ReplayedStep / ReplayedDualStep(..., log_k=5) append every replay's training-mode attention,
logits and loss dict to an EpochLog inside the captured graph, and epoch_scores() scores them.  The scores are compared with
tests/eval_log_oracle.py fed the outputs each replay left behind (copied to the host by the test, never by the product); the keys that
are functions of integer counts match exactly, the continuous ones at tests.util.TOL (tests.test_gpu_ragged._match).  Model builders,
graphs, slots and capacities are those of tests/test_gpu_ragged.py and tests/test_gpu_ragged_pair.py."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import padded_oracle as po
from tests import ragged_oracle as ro
from tests import ragged_pair_oracle as rp
from tests import train_log as tl
from tests.replay import pin_seed_stream, seed_state
from tests.test_gpu_dual_eval import DUAL_KEYS, MIX, _debug_graphs
from tests.test_gpu_dual_replay import _dual_gsat, _pair_datasets
from tests.test_gpu_dual_replay import _dump as _dump_pair
from tests.test_gpu_eval_log import HITS_KEY, _gsat, _labelled_graphs, _training_state
from tests.test_gpu_ragged import _debug_graph, _dump, _match
from tests.util import TOL, assert_no_memset_nodes

pytestmark = pytest.mark.gpu
SLOTS, CAP = ro.RAGGED_SLOTS, ro.RAGGED_CAPACITY
K = tl.K


def _state(gsat):
    return {k: v.detach().clone() for k, v in gsat.state_dict().items()}


def _check_losses(rs, loss):
    """``losses`` is the step's own loss dict: its first entry is the returned loss, bit for bit, and the fp32 sum of the other two."""
    assert rs.losses.shape == (3,) and rs.losses.dtype == torch.float32
    assert torch.equal(rs.losses[0], loss) and torch.equal(rs.losses[1] + rs.losses[2], rs.losses[0])


# ---- 1. the scores of a training epoch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])
def test_training_epoch_scores_what_its_replays_produced(dev, backbone, edge):
    """ReplayedStep(ragged=True, keep_edge_att=True, log_k=5) at the capacity (300, 620) with 16 slots: begin_epoch(), the six budget batches
    of range(48) (7, 10, 10, 6, 9 and 6 graphs) as replays at epochs 0..5, epoch_scores() against the oracle on their concatenation; then
    begin_epoch() and three replays, which are scored alone."""
    import dp_gsat_amd as G
    graphs = _labelled_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = _gsat(dev, backbone, edge, graphs)
    before = _state(gsat)
    graph = _debug_graph()
    rs = G.ReplayedStep(gsat, ds, SLOTS, capacity=CAP, keep_edge_att=True, graph=graph, ragged=True, log_k=K)
    assert not G.graph_index.sync_free() and gsat.sync_loss_dict
    for k, v in gsat.state_dict().items():                   # capturing (three warm-up steps) did not train ...
        assert torch.equal(v, before[k]), k
    log = rs.log                                             # ... and left the log empty
    assert isinstance(log, G.EpochLog) and rs.dual_log is None and log.state.tolist() == [0, 0, 0, 0] and log.loss_sums.tolist() == [0.0] * 3
    assert (log.k, log.bins, log.multi_label, log.logit_cols, log.y_cols) == (K, 64, False, 1, 1)
    assert (log.max_graphs, log.max_edges, log.max_batches) == (48, int(ds.edge_local_all.shape[1]), 48)
    assert_no_memset_nodes(_dump(graph), "ReplayedStep(log_k)")
    with pytest.raises(ValueError, match="before any append"):
        rs.epoch_scores()
    rows = rs.batches(range(48))
    lists = ro.rows_to_lists(rows)
    assert [len(r) for r in lists] == ro.RAGGED_SIZES
    for picked in (range(6), (4, 1, 3)):
        rs.begin_epoch()
        assert rs.log is log and log.state.tolist() == [0, 0, 0, 0]
        oracle, triples, edges = tl.new_oracle(ds), [], 0
        for epoch, j in enumerate(picked):
            ids = lists[j]
            N, E = po.totals(graphs, ids)
            loss = rs.step(rows[j], epoch)
            torch.cuda.synchronize()
            assert rs.batch.valid.tolist() == [N, E, len(ids), 0]
            assert rs.edge_att.shape == (CAP[1], 1) and rs.clf_logits.shape == (SLOTS + 1, 1)
            _check_losses(rs, loss)
            tl.feed_padded(oracle, rs.edge_att, rs.batch, rs.clf_logits, rs.losses, len(ids))
            triples.append(tl.cpu(rs.losses))
            edges += E
        assert log.state.tolist() == [edges, sum(len(lists[j]) for j in picked), len(picked), 0]
        got = rs.epoch_scores()
        what = f"{backbone} batches {list(picked)}: "
        _match(got, oracle.compute(), what + "epoch_scores against the oracle")
        for key, mean in zip(("loss", "pred", "info"), tl.loss_means(triples)):          # the means over the steps
            assert abs(got[key] - mean) <= 1e-12 * max(1.0, abs(mean)), what + key
        assert not rs.overflowed()
    G.clear_cache()


def test_fixed_count_instance_takes_the_callers_tail(dev):
    """ReplayedStep(gsat, ds, 8, log_k=5): two replays of eight graphs and the eager tail of five, appended by the caller as the class
    docstring shows; epoch_scores() scores all 21 graphs."""
    import dp_gsat_amd as G
    graphs = _labelled_graphs(40, self_loop=(5,))
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = _gsat(dev, "GIN", True, graphs)
    rs = G.ReplayedStep(gsat, ds, 8, keep_edge_att=True, log_k=K)
    ids = [33, 5, 12, 0, 27, 39, 8, 19, 2, 30, 31, 7, 22, 14, 36, 9, 11, 3, 25, 38, 17]
    assert rs.log.max_batches == 5 and rs.log.state.tolist() == [0, 0, 0, 0]
    oracle = tl.new_oracle(ds)
    rs.begin_epoch()
    for s in (0, 8):
        loss = rs.step(ids[s:s + 8], 0)
        torch.cuda.synchronize()
        _check_losses(rs, loss)
        tl.feed_padded(oracle, rs.edge_att, rs.batch, rs.clf_logits, rs.losses, 8)
    tail = ds.collate(torch.tensor(ids[16:], device=dev))
    gsat.sync_loss_dict = False
    try:
        att, loss, ld, logits = gsat.forward_pass(tail, 0, True)
    finally:
        gsat.sync_loss_dict = True
    gsat.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    gsat.optimizer.step()
    losses = torch.stack([ld["loss"], ld["pred"], ld["info"]])
    rs.log.append(att, tail, logits, losses)
    oracle.append(tl.cpu(att), tl.cpu(tail.edge_label), tl.cpu(tail.edge_index), tl.cpu(tail.batch), 5, tl.cpu(logits), tl.cpu(tail.y),
                  tl.cpu(losses))
    assert rs.log.state.tolist()[1:] == [21, 3, 0]
    _match(rs.epoch_scores(), oracle.compute(), "two replays and the eager tail")
    G.clear_cache()


# ---- 2. the pair ------------------------------------------------------------------------------------------------------------------------------
def test_dual_training_epoch_scores_both_attentions(dev):
    """ReplayedDualStep(ragged=True, keep_edge_att=True, log_k=5, score_dual=True) with mix_after_epoch=1 over the seven three-budget
    batches of range(48): one epoch on the unmixed graph (epoch number 0) and one on the mixed graph (2)."""
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, **po.STEP_GRAPHS)
    omods, mods, dg, opts = _dual_gsat(dev, "GIN", graphs, True, **MIX)
    before = _state(dg)
    dbg = _debug_graphs()
    pcap = rp.PAIR_CAPACITY
    rs = G.ReplayedDualStep(dg, ds, dual, rp.PAIR_SLOTS, capacity=pcap, keep_edge_att=True, graphs=dbg, ragged=True, log_k=K, score_dual=True)
    assert not G.graph_index.sync_free() and dg.sync_loss_dict and dg.keep_dual_att is False and dg.dual_att is None
    for k, v in dg.state_dict().items():
        assert torch.equal(v, before[k]), k
    for which, gr in zip(("unmixed", "mixed"), dbg):
        assert_no_memset_nodes(_dump_pair(gr), "ReplayedDualStep(log_k) " + which)
    for log in (rs.log, rs.dual_log):
        assert isinstance(log, G.EpochLog) and log.state.tolist() == [0, 0, 0, 0] and log.loss_sums.tolist() == [0.0] * 3
        assert (log.k, log.multi_label, log.max_graphs, log.max_batches) == (K, False, 48, 48)
    assert rs.log is not rs.dual_log
    rows = rs.batches(range(48))
    lists = ro.rows_to_lists(rows)
    assert [len(r) for r in lists] == rp.PAIR_SIZES
    from tests import dual_oracle as do
    for epoch in (0, 2):
        rs.begin_epoch()
        assert rs.log.state.tolist() == [0, 0, 0, 0] and rs.dual_log.state.tolist() == [0, 0, 0, 0]
        oracle, oracle_d, triples = tl.new_oracle(ds), tl.new_oracle(ds), []
        for j, ids in enumerate(lists):
            N, E, Ed = do.pair_totals(graphs, ids)
            loss = rs.step(rows[j], epoch)
            torch.cuda.synchronize()
            assert rs.batch.valid.tolist() == [N, E, len(ids), 0] and rs.dual_batch.valid.tolist() == [E, Ed, len(ids), 0]
            assert rs.edge_att.shape == (pcap[1], 1) and rs.dual_att.shape == (pcap[1], 1) and rs.losses.shape == (3,)
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(rs.losses).all())
            assert not torch.equal(rs.edge_att[:E], rs.dual_att[:E])
            tl.feed_padded(oracle, rs.edge_att, rs.batch, rs.clf_logits, rs.losses, len(ids))
            tl.feed_padded(oracle_d, rs.dual_att, rs.batch, rs.clf_logits, rs.losses, len(ids))
            triples.append(tl.cpu(rs.losses))
        assert rs.log.state.tolist()[1:] == [48, len(lists), 0] and rs.dual_log.state.tolist() == rs.log.state.tolist()
        got = rs.epoch_scores()
        want, want_d = oracle.compute(), oracle_d.compute()
        assert set(got) == set(want) | {"dual_" + key for key in DUAL_KEYS}
        _match({k: v for k, v in got.items() if not k.startswith("dual_")}, want, f"epoch {epoch}: epoch_scores against the oracle")
        for key, mean in zip(("loss", "pred", "info"), tl.loss_means(triples)):
            assert abs(got[key] - mean) <= 1e-12 * max(1.0, abs(mean)), (epoch, key)
        for key in DUAL_KEYS:
            exact = key in ("att_auroc", HITS_KEY)                # functions of integer counts
            assert abs(got["dual_" + key] - want_d[key]) <= (1e-12 if exact else TOL * max(1.0, abs(want_d[key]))), (epoch, key)
        assert dg.keep_dual_att is False and dg.dual_att is None
    assert not rs.overflowed()
    G.clear_cache()


# ---- 3. logging does not move training ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])
def test_logging_does_not_move_training(dev, backbone, edge):
    """Two fresh, identically seeded models, one with log_k=5 and one without: after the same six replays parameters, BatchNorm buffers,
    Adam state and the device seed stream's state are bitwise equal, and so were the returned losses."""
    import dp_gsat_amd as G
    graphs = _labelled_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    runs = []
    for log_k in (K, None):
        torch.manual_seed(99)
        gsat = _gsat(dev, backbone, edge, graphs)
        rs = G.ReplayedStep(gsat, ds, SLOTS, capacity=CAP, ragged=True, log_k=log_k)
        assert rs.edge_att is None
        pin_seed_stream(dev, 0x5EED)
        rs.begin_epoch()                                      # without a log: nothing to empty
        losses = []
        for epoch, row in enumerate(rs.batches(range(48))):
            losses.append(rs.step(row, epoch).clone())
            assert rs.edge_att is None                        # what a step publishes does not change
        torch.cuda.synchronize()
        assert not rs.overflowed() and len(losses) == 6
        if log_k is None:
            assert rs.log is None and rs.losses is None
            with pytest.raises(ValueError, match="without log_k"):
                rs.epoch_scores()
        else:
            assert rs.log.state.tolist()[1:] == [48, 6, 0] and np.isfinite(rs.epoch_scores()["loss"])
        runs.append((_training_state(gsat, dev), losses))
    ((a, seed_a), la), ((b, seed_b), lb) = runs
    assert any(k.startswith("adam.") for k in a) and any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0
    tl.assert_bitwise(a, b)
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    G.clear_cache()


def test_logging_does_not_move_dual_training(dev):
    """The same for the pair, with both logs, over four three-budget batches: two on the unmixed and two on the mixed graph."""
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, **po.STEP_GRAPHS)
    runs = []
    for log_k in (K, None):
        torch.manual_seed(99)
        omods, mods, dg, opts = _dual_gsat(dev, "GIN", graphs, True, **MIX)
        rs = G.ReplayedDualStep(dg, ds, dual, rp.PAIR_SLOTS, capacity=rp.PAIR_CAPACITY, ragged=True, log_k=log_k, score_dual=log_k is not None)
        pin_seed_stream(dev, 0x5EED)
        rs.begin_epoch()
        losses = [rs.step(row, epoch).clone() for epoch, row in zip((0, 1, 2, 3), rs.batches(range(48)))]
        torch.cuda.synchronize()
        assert not rs.overflowed()
        if log_k is not None:
            assert rs.log.state.tolist()[2:] == [4, 0] and rs.dual_log.state.tolist() == rs.log.state.tolist()
            assert np.isfinite(rs.epoch_scores()["dual_delta_kl"])
        state = {}
        for side, opt in (("primal", opts[0]), ("dual", opts[1])):
            got, _ = _training_state(NS(optimizer=opt, named_parameters=dg.named_parameters, named_buffers=dg.named_buffers), dev)
            state.update({side + "." + k if k.startswith("adam.") else k: v for k, v in got.items()})
        runs.append((state, seed_state(dev), losses))
    (a, seed_a, la), (b, seed_b, lb) = runs
    assert any(k.startswith("primal.adam.") for k in a) and any(k.startswith("dual.adam.") for k in a)
    assert seed_a == seed_b and seed_a[1] > 0
    tl.assert_bitwise(a, b)
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    G.clear_cache()


# ---- 4. overflow -------------------------------------------------------------------------------------------------------------------------------
def test_an_overflowed_step_makes_epoch_scores_raise(dev):
    import dp_gsat_amd as G
    graphs = _labelled_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = _gsat(dev, "GIN", True, graphs)
    rs = G.ReplayedStep(gsat, ds, SLOTS, capacity=CAP, ragged=True, log_k=K)
    rows = rs.batches(range(48))
    n16, e16 = po.totals(graphs, range(SLOTS))
    assert n16 + 2 > CAP[0] or e16 > CAP[1]
    rs.begin_epoch()
    rs.step(rows[0], 0)
    rs.step(list(range(SLOTS)), 0)                            # does not fit: appends nothing, sets the log's flag bit 0
    rs.step(rows[1], 0)
    torch.cuda.synchronize()
    assert rs.log.state.tolist()[1:] == [sum(ro.RAGGED_SIZES[:2]), 2, 1]
    with pytest.raises(ValueError, match="flag bit 0"):
        rs.epoch_scores()
    assert rs.overflowed() and not rs.overflowed()            # the step's own flag still reports it, once
    with pytest.raises(ValueError, match="flag bit 0"):      # the log keeps its flag until the next epoch begins
        rs.epoch_scores()
    rs.begin_epoch()
    rs.step(rows[2], 1)
    assert np.isfinite(rs.epoch_scores()["loss"]) and not rs.overflowed()
    G.clear_cache()


# ---- 5. the default graph ----------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])
def test_without_log_k_the_captured_graph_is_the_parents(dev, backbone, edge, monkeypatch):
    """Without log_k the dumped graph of ReplayedStep holds the kernel nodes it held before the training-pass log existed, in the same
    order: tests/golden/replayed_step_kernels_*.txt, recorded on an MI355X from the commit before.  The library's own kernels are
    compared always, torch's (whose names belong to the torch build) when torch is the version of the recording.  With log_k the graph is
    that list with kernels added behind the optimizer's -- the last two are the library's append -- and nothing removed or reordered.
    The lists were recorded in a process that had met no hub rows (an earlier batch with some routes every later sync-free batch to the
    chunked aggregation kernels): that state is pinned here."""
    import dp_gsat_amd as G
    monkeypatch.setattr("dp_gsat_amd.graph_index._HUBS_SEEN", [False])
    graphs = _labelled_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    version, want = tl.read_kernel_list(os.path.join(GOLDEN, f"replayed_step_kernels_{backbone}.txt"))
    lists = {}
    for log_k in (None, K):
        graph = tl.kept_debug_graph()
        assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
        torch.manual_seed(7)
        gsat = _gsat(dev, backbone, edge, graphs)
        rs = G.ReplayedStep(gsat, ds, SLOTS, capacity=CAP, graph=graph, ragged=True, log_k=log_k)
        text = _dump(graph)
        assert text is not None, "no dump of a kept graph"
        assert_no_memset_nodes(text, f"ReplayedStep(log_k={log_k})")
        lists[log_k] = tl.kernel_nodes(text)
        assert np.isfinite(float(rs.step(rs.batches(range(48))[0], 0)))         # the kept graph instantiates at its first replay
        G.clear_cache()
    got, logged = lists[None], lists[K]
    assert tl.library_kernels(got) == tl.library_kernels(want)
    if torch.__version__ == version:
        assert got == want
    else:
        assert len(got) == len(want)
    assert logged[:len(got)] == got and len(logged) > len(got)
    added = tl.library_kernels(logged[len(got):])          # gsat_eval_log_append: k_log_copy, k_log_commit -- last of all
    assert [("k_log_copy" in n, "k_log_commit" in n) for n in added[-2:]] == [(True, False), (False, True)], added
    assert "k_log_commit" in logged[-1] and sum("k_log_" in n for n in logged) == 2


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_training_log_refusals(dev):
    import dp_gsat_amd as G
    graphs = _labelled_graphs(12)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    unlabelled = G.PackedDataset.from_data_list(po.mutag_graphs(count=12), dev)
    gsat = _gsat(dev, "GIN", True, graphs)
    before = _state(gsat)
    for kw, match in ((dict(log_k=0), "log_k"), (dict(log_k=-3), "log_k"), (dict(log_k=2.5), "log_k"), (dict(log_k=K, bins=0), "bins")):
        with pytest.raises(ValueError, match=match):
            G.ReplayedStep(gsat, ds, 5, **kw)
    with pytest.raises(ValueError, match="edge labels"):
        G.ReplayedStep(gsat, unlabelled, 5, log_k=K)
    for k, v in gsat.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not G.graph_index.sync_free() and gsat.sync_loss_dict
    rs = G.ReplayedStep(gsat, ds, 5, log_k=K, bins=16, max_graphs=10, max_edges=400)
    assert (rs.log.bins, rs.log.max_graphs, rs.log.max_edges, rs.log.max_batches) == (16, 10, 400, 2)
    G.clear_cache()
