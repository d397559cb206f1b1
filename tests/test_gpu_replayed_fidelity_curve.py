"""gpu: ReplayedFidelityCurve -- a fidelity curve over S sparsity levels as replays of one captured graph -- against the log oracle on the
logits it publishes, against S single-level ``ReplayedFidelity`` runs (the path as it was), that a curve epoch between training steps
changes nothing, and its refusals."""
import numpy as np
import pytest
import torch

from tests import fidelity_curve_oracle as fco
from tests import padded_oracle as po
from tests import train_log as tl
from tests.replay import pin_seed_stream
from tests.test_gpu_fidelity_curve_log import P_RTOL
from tests.test_gpu_replayed_fidelity import H, IDS, SLOTS, _dump, _graphs, _gsat, _training_state
from tests.util import TOL, assert_no_memset_nodes

pytestmark = pytest.mark.gpu
CASES = [("GIN", True, dict(ks=[2, 5]), False), ("GIN", True, dict(ratios=[0.3, 0.7]), True), ("PNA", False, dict(ratios=[0.3, 0.7]), False),
         ("PNA", False, dict(ks=[2, 5]), True)]


def _ragged_capacity(graphs):
    nodes, edges = po.sizes(graphs)
    return int(nodes.mean() * 10) + 2, int(edges.mean() * 10)          # room for about ten mean graphs: batches of differing graph counts


@pytest.mark.parametrize("backbone,edge,levels,ragged", CASES, ids=["GIN-ks-fixed", "GIN-ratios-ragged", "PNA-ratios-fixed", "PNA-ks-ragged"])
def test_run_equals_the_log_oracle_and_the_single_level_replays(dev, backbone, edge, levels, ragged):
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat, _ = _gsat(dev, backbone, edge, graphs)
    capacity = _ragged_capacity(graphs) if ragged else None
    values = next(iter(levels.values()))
    S, V = len(values), 2 * len(values) + 1
    graph = tl.kept_debug_graph()
    assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
    modes = [m.training for m in gsat.modules()]
    before = {n: t.detach().clone() for n, t in list(gsat.named_parameters()) + list(gsat.named_buffers())}
    rc = G.ReplayedFidelityCurve(gsat, ds, SLOTS, capacity=capacity, ragged=ragged, graph=graph, **levels)
    assert [m.training for m in gsat.modules()] == modes and not G.graph_index.sync_free() and gsat.sync_loss_dict
    assert rc.log.state.tolist() == [0] * 20 and not rc.overflowed()
    assert all(torch.equal(t, before[n]) for n, t in list(gsat.named_parameters()) + list(gsat.named_buffers()))
    text = _dump(graph)
    assert text is not None, "no dump of a kept graph"
    assert assert_no_memset_nodes(text, "ReplayedFidelityCurve")
    names = tl.library_kernels(tl.kernel_nodes(text))
    mine = [n for n in names if "k_stk_" in n]
    assert len(mine) == 5 and "k_stk_levels" in mine[0] and "k_stk_fill" in mine[-1], mine          # a launch count that does not depend on S
    assert not any("k_subp_" in n for n in names) and "k_fidc_commit" in names[-1], names[-6:]       # no per-level extraction; the append last

    got = rc.run(np.asarray(IDS))
    again = rc.run(np.asarray(IDS))
    assert got == again                                                                # bitwise repeatable
    if ragged:
        rows = [[int(i) for i in row.tolist() if i >= 0] for row in rc.batches(IDS)]
        replayed = [True] * len(rows)
        assert len({len(r) for r in rows}) > 1 and all(1 <= len(r) <= SLOTS for r in rows), [len(r) for r in rows]
    else:
        rows = [IDS[s:s + SLOTS] for s in range(0, len(IDS), SLOTS)]
        replayed = [len(r) == SLOTS for r in rows]
        assert [len(r) for r in rows] == [16, 16, 11]
    assert got["n"] == len(IDS) and rc.log.state.tolist()[:3] == [len(IDS), len(rows), 0] and got["levels"] == values

    cls, p, kept, edges, top = [], [], np.zeros(S, np.int64), 0, 1.0
    for row, is_replay in zip(rows, replayed):
        ub = ds.collate(torch.tensor(row, device=dev))
        if is_replay:
            rc.step(row, 0)
            assert rc.batch.valid.tolist() == [ub.num_nodes, ub.num_edges, len(row), 0]
            logits, stack = rc.logits.clone(), rc.stack
            assert stack.graphs_per_variant == SLOTS + 1 and stack.node_capacity == rc.capacity[0]
        else:
            gsat.eval()                                                                # the eager tail, through the code run() takes
            _, stack, logits = rc._forward(ub, 0)
            gsat.train()
            assert stack.graphs_per_variant == len(row) + 1 and stack.node_capacity == ub.num_nodes + 2
        sv = stack.valid.cpu().numpy()
        assert logits.shape[0] == V * stack.graphs_per_variant and (sv[:, 3] == 0).all() and (sv[:, 0] == ub.num_nodes).all()
        assert sv[0, 1] == ub.num_edges and (sv[1:1 + S, 1] + sv[1 + S:, 1] == ub.num_edges).all() and (sv[:, 2] == len(row)).all()
        c, q = fco.rows(logits.cpu().numpy(), stack.graphs_per_variant, S, len(row))
        cls.append(c)
        p.append(q)
        kept += sv[1:1 + S, 1]
        edges += int(sv[0, 1])
        top = max(top, float(logits.view(V, stack.graphs_per_variant, -1)[:, :len(row)].abs().max()))
    assert gsat.training
    cls, p = np.concatenate(cls), np.concatenate(p)
    want = fco.compute(cls, p, S, kept, edges, values)
    for key in fco.EXACT_KEYS:                                                         # integers and their quotients: exact
        assert got[key] == want[key], (key, got[key], want[key])
    n = len(IDS)
    for key in fco.PROB_KEYS:                                                          # the bound of tests/test_gpu_fidelity_curve_log.py
        a, b = np.atleast_1d(got[key]), np.atleast_1d(want[key])
        print(f"{backbone} {key}: {got[key]!r} / {want[key]!r}")
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 2 * (P_RTOL + n * 2.0 ** -53), (key, got[key], want[key])
    assert not rc.overflowed()

    # the path as it was: one ReplayedFidelity per level on the same ids.  Softmax and sigmoid are 1-Lipschitz in the logits, so the
    # forward tolerance carries over to every probability and to their means; flip rates are not compared across the two paths
    bound = TOL * top
    for s, l in enumerate(values):
        one = dict(k=l) if "ks" in levels else dict(ratio=l)
        rf = G.ReplayedFidelity(gsat, ds, SLOTS, capacity=capacity, ragged=ragged, **one)
        single = rf.run(np.asarray(IDS))
        assert single["n"] == got["n"]
        for key, mine in (("p_full", got["p_full"]), ("p_keep", got["p_keep"][s]), ("p_drop", got["p_drop"][s])):
            print(f"{backbone} level {l} {key}: stacked {mine!r} / single {single[key]!r}; bound {bound:.2e}")
            assert abs(mine - single[key]) <= bound, (l, key, mine, single[key])
    G.clear_cache()


def test_one_level_keeps_the_fraction_of_edges_the_single_level_extraction_keeps(dev):
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat, _ = _gsat(dev, "GIN", True, graphs)
    capacity = _ragged_capacity(graphs)
    rc = G.ReplayedFidelityCurve(gsat, ds, SLOTS, ratios=[0.3], capacity=capacity, ragged=True)
    got = rc.run(np.asarray(IDS))
    rf = G.ReplayedFidelity(gsat, ds, SLOTS, ratio=0.3, capacity=capacity, ragged=True)
    kept = edges = 0
    for row in rf.batches(IDS):
        rf.step(row, 0)
        kept += int(rf.keep_batch.valid[1])
        edges += int(rf.batch.valid[1])
    assert edges > 0 and got["kept_fraction"] == [kept / edges] and got["levels"] == [0.3]
    G.clear_cache()


def test_a_curve_epoch_does_not_disturb_training(dev):
    """Three replayed training steps with a replayed curve epoch after each, and the same steps without: parameters, BatchNorm buffers,
    Adam state, the device seed state and torch's generator states are bitwise equal."""
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    steps = [IDS[:16], IDS[16:32], IDS[8:24]]
    runs = []
    for with_curve in (True, False):
        torch.manual_seed(99)
        torch.cuda.manual_seed(99)
        G.ops.device_seed(dev)              # the seed stream re-bases itself from the CPU generator after a manual_seed: once here in BOTH runs
        gsat, _ = _gsat(dev, "PNA", False, graphs)
        torch.manual_seed(7)
        rs = G.ReplayedStep(gsat, ds, SLOTS)
        rc = G.ReplayedFidelityCurve(gsat, ds, SLOTS, ratios=[0.2, 0.5, 0.8]) if with_curve else None
        pin_seed_stream(dev, 0x5EED)
        for epoch, ids in enumerate(steps):
            rs.step(ids, epoch)
            if rc is not None:
                res = rc.run(np.asarray(IDS))
                assert np.isfinite(res["fidelity_plus"]).all() and res["n"] == len(IDS) and gsat.training
        torch.cuda.synchronize()
        runs.append(_training_state(gsat, dev))
    (a, seed_a, cuda_a, cpu_a), (b, seed_b, cuda_b, cpu_b) = runs
    assert set(a) == set(b) and any(k.startswith("adam.") for k in a) and any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0                              # the training steps drew, the curve epochs did not
    assert torch.equal(cuda_a, cuda_b) and torch.equal(cpu_a, cpu_b)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()


def test_replayed_fidelity_curve_refusals(dev, monkeypatch):
    import dp_gsat_amd as G
    from dp_gsat_amd import explain
    from dp_gsat_amd.encoders import BatchNorm1d
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat, _ = _gsat(dev, "GIN", True, graphs)
    modes = [m.training for m in gsat.modules()]

    def refused(match, model=gsat, dataset=ds, **kw):
        with pytest.raises(ValueError, match=match):
            G.ReplayedFidelityCurve(model, dataset, SLOTS, **kw)
        assert not G.graph_index.sync_free() and [m.training for m in gsat.modules()] == modes

    refused("exactly one of ks and ratios")
    refused("exactly one of ks and ratios", ks=[5], ratios=[0.3])
    refused("strictly increasing", ks=[5, 5])
    refused("strictly increasing", ratios=[0.5, 0.3])
    refused("1 to 16 levels", ks=list(range(1, 18)))
    refused("1 to 16 levels", ratios=[])
    refused("multi-label", model=G.GSAT(gsat.clf, gsat.extractor, G.Criterion(2, True), None, learn_edge_att=True), ks=[5])
    bns = [m for m in gsat.modules() if isinstance(m, BatchNorm1d)]
    bns[0].sync_group = True
    refused("sync_group", ks=[5])
    del bns[0].sync_group
    shared = {"learn_edge_att": False, "extractor_dropout_p": 0.5}
    mcfg = dict(pred_loss_coef=1, info_loss_coef=1, fix_r=False, decay_interval=10, decay_r=0.1, final_r=0.5)
    dual = G.DualGSAT(gsat.clf, G.ExtractorMLP(H, shared, "primal").to(dev), None, gsat.clf, G.ExtractorMLP(H, shared, "dual").to(dev), None,
                      mcfg, mcfg, False, False)
    refused("DualGSAT", model=dual, ks=[5])
    unlabelled = G.PackedDataset(ds.x_all, ds.edge_local_all, ds.node_ptr_all, ds.edge_ptr_all, None)
    refused("graph labels", dataset=unlabelled, ks=[5])
    with monkeypatch.context() as mp:                                                  # a dataset whose largest graph the fused ranking cannot take
        mp.setattr(explain, "rank_edges_lds_cap", lambda: int(ds.edge_counts.max()) - 1)
        refused("rank_edges_lds_cap", ks=[5])
    n, e = po.totals(graphs, list(range(SLOTS)))
    for cap in ((n + 1, e), (n + 2, e - 1)):                                           # a capacity the first batch does not fit
        refused("do not fit the capacity", ks=[5], capacity=cap)
    rc = G.ReplayedFidelityCurve(gsat, ds, 5, ks=[2, 5])                               # and the plain model is taken
    with pytest.raises(ValueError, match="captured for 5"):
        rc.step([0, 1, 2], 0)
    rc.check_epoch(list(range(ds.num_graphs)))
    assert not G.graph_index.sync_free() and gsat.training
    G.clear_cache()
