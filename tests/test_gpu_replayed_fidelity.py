"""gpu: ReplayedFidelity -- a fidelity epoch as replays of one captured graph -- against the per-batch eager ``explanation_fidelity`` and
against the fp64 oracle backbones on oracle-extracted graphs; that a fidelity epoch between training steps changes nothing; its
refusals.  Floating-point comparisons follow tests.util.close (TOL = 1e-4)."""
import copy
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import modules as om
from tests import explain_oracle as xo
from tests import padded_oracle as po
from tests import subgraph_oracle as so
from tests import train_log as tl
from tests.replay import pin_seed_stream, seed_state
from tests.util import TOL, assert_no_memset_nodes, close

pytestmark = pytest.mark.gpu
H, SLOTS = 32, 16
GRAPHS = dict(count=48, self_loop=(5,))
IDS = [int(i) for i in np.random.RandomState(11).permutation(48)[:43]]                 # fixed count: 16 + 16 and an eager tail of 11
# The model seeds, picked on the CPU (tests/test_gpu_replayed_fidelity.py::margins, run by hand): with them every graph's full-graph logit
# of the fp64 oracle backbone lies more than 100 x TOL x max(1, |logits|_inf) from the class boundary.  The test asserts it.
SEEDS = {"GIN": 0, "PNA": 3}
CASES = [("GIN", True, 5, None, False), ("GIN", True, None, 0.3, True), ("PNA", False, None, 0.3, False), ("PNA", False, 5, None, True)]


def _graphs():
    return po.mutag_graphs(**GRAPHS)


def _oracle_models(backbone, edge, graphs, seed=None):
    """(oracle backbone, oracle extractor) on the CPU, drawn from torch's generator at the backbone's seed."""
    torch.manual_seed(SEEDS[backbone] if seed is None else seed)
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=0.3, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=deg)
    oclf = (om.GIN if backbone == "GIN" else om.PNA)(14, 0, 2, False, cfg)
    return oclf, om.ExtractorMLP(H, edge), cfg


def _gsat(dev, backbone, edge, graphs, capturable=True):
    import dp_gsat_amd as G
    oclf, oext, cfg = _oracle_models(backbone, edge, graphs)
    clf = G.get_model(14, 0, 2, False, cfg, dev)
    clf.load_state_dict(oclf.state_dict())
    ext = G.ExtractorMLP(H, edge).to(dev)
    ext.load_state_dict(oext.state_dict())
    opt = torch.optim.Adam(list(clf.parameters()) + list(ext.parameters()), lr=1e-2, weight_decay=3e-6, capturable=capturable, fused=capturable)
    return G.GSAT(clf, ext, G.Criterion(2, False), opt, learn_edge_att=edge, decay_interval=1).train(), oclf.eval()


def _cpu_batch(graphs, ids):
    """``PackedDataset.collate(ids)`` on the host."""
    from dp_gsat_amd.synth import Batch
    n = np.cumsum([0] + [graphs[g].x.shape[0] for g in ids])
    return Batch(x=torch.cat([graphs[g].x for g in ids]), edge_index=torch.cat([graphs[g].edge_index + int(o) for g, o in zip(ids, n)], dim=1),
                 batch=torch.repeat_interleave(torch.arange(len(ids)), torch.tensor(np.diff(n))), edge_attr=None,
                 y=torch.cat([graphs[g].y for g in ids]), num_graphs=len(ids))


def _bound(*logits):
    return TOL * max(1.0, max(float(z.abs().max()) for z in logits))


def margins(backbone, edge=None, seed=None):
    """Smallest |full-graph logit| of the fp64 oracle backbone over the 48 graphs, and the bound it is held against (CPU only)."""
    graphs = _graphs()
    oclf, _, _ = _oracle_models(backbone, backbone == "GIN" if edge is None else edge, graphs, seed)
    cb = _cpu_batch(graphs, list(range(48)))
    with torch.no_grad():
        z = copy.deepcopy(oclf).eval().double()(cb.x.double(), cb.edge_index, cb.batch, None)
    return float(z.abs().min()), _bound(z)


def _probs(full, keep, drop):
    """fp64 (classes [G, 3], probabilities [G, 3]) from one-logit blocks, by the rule of explanation_fidelity."""
    full, keep, drop = (z.detach().cpu().double().view(-1) for z in (full, keep, drop))
    sign = torch.where(full >= 0, 1.0, -1.0).double()
    return (torch.stack([(z >= 0).long() for z in (full, keep, drop)], dim=1),
            torch.stack([torch.sigmoid(sign * z) for z in (full, keep, drop)], dim=1))


def _summary(cls, p):
    return {"fidelity_plus": float((p[:, 0] - p[:, 2]).mean()), "fidelity_minus": float((p[:, 0] - p[:, 1]).mean()),
            "p_full": float(p[:, 0].mean()), "p_keep": float(p[:, 1].mean()), "p_drop": float(p[:, 2].mean()),
            "flip_plus": int((cls[:, 2] != cls[:, 0]).sum()) / len(cls), "flip_minus": int((cls[:, 1] != cls[:, 0]).sum()) / len(cls),
            "n": len(cls)}


def _dump(graph):
    try:
        path = os.path.join(tempfile.mkdtemp(), "graph.dot")
        graph.debug_dump(path)
        if os.path.exists(path) and os.path.getsize(path) > 0:
            return open(path, errors="replace").read()
    except Exception:
        pass
    return None


@pytest.mark.parametrize("backbone,edge,k,ratio,ragged", CASES, ids=["GIN-k5-fixed", "GIN-r0.3-ragged", "PNA-r0.3-fixed", "PNA-k5-ragged"])
def test_run_equals_the_eager_fidelity_and_the_oracle(dev, backbone, edge, k, ratio, ragged):
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat, oclf = _gsat(dev, backbone, edge, graphs)
    oclf64 = copy.deepcopy(oclf).double()
    nodes, edges = po.sizes(graphs)
    # ragged: room for about ten mean graphs, so that budget batching cuts batches of differing graph counts
    capacity = (int(nodes.mean() * 10) + 2, int(edges.mean() * 10)) if ragged else None
    graph = tl.kept_debug_graph()                                                       # a default CUDAGraph gives its hipGraph up: no dump
    assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
    modes = [m.training for m in gsat.modules()]
    before = {n: t.detach().clone() for n, t in list(gsat.named_parameters()) + list(gsat.named_buffers())}
    rf = G.ReplayedFidelity(gsat, ds, SLOTS, k=k, ratio=ratio, capacity=capacity, ragged=ragged, graph=graph)
    assert [m.training for m in gsat.modules()] == modes and not G.graph_index.sync_free() and gsat.sync_loss_dict
    assert rf.log.state.tolist() == [0, 0, 0, 0] and not rf.overflowed()
    assert all(torch.equal(t, before[n]) for n, t in list(gsat.named_parameters()) + list(gsat.named_buffers()))
    text = _dump(graph)
    assert text is not None, "no dump of a kept graph"
    assert assert_no_memset_nodes(text, "ReplayedFidelity")
    names = tl.library_kernels(tl.kernel_nodes(text))
    assert sum("k_subp_fill" in n for n in names) == 2 and "k_fid_commit" in names[-1], names[-6:]      # two extractions; the append comes last
    N_cap, E_cap = rf.capacity
    assert rf.keep_capacity == (N_cap, 5 * SLOTS if k is not None else min(E_cap, int(np.ceil(0.3 * E_cap)) + SLOTS))

    got = rf.run(np.asarray(IDS))
    again = rf.run(np.asarray(IDS))
    assert got == again                                                                # bitwise repeatable
    if ragged:
        rows = [[int(i) for i in row.tolist() if i >= 0] for row in rf.batches(IDS)]
        replayed = [True] * len(rows)
        assert len({len(r) for r in rows}) > 1 and all(1 <= len(r) <= SLOTS for r in rows), [len(r) for r in rows]
    else:
        rows = [IDS[s:s + SLOTS] for s in range(0, len(IDS), SLOTS)]
        replayed = [len(r) == SLOTS for r in rows]
        assert [len(r) for r in rows] == [16, 16, 11]
    assert sum(len(r) for r in rows) == len(IDS) == got["n"] and rf.log.state.tolist() == [len(IDS), len(rows), 0, 0]

    own, eager, oracle, bound = [], [], [], 0.0
    for row, is_replay in zip(rows, replayed):
        b = len(row)
        ub = ds.collate(torch.tensor(row, device=dev))
        cb = _cpu_batch(graphs, row)
        E = ub.num_edges
        assert torch.equal(ub.edge_index.cpu(), cb.edge_index) and torch.equal(ub.x.cpu(), cb.x)
        if is_replay:
            rf.step(row, 0)
            assert rf.batch.valid.tolist() == [ub.num_nodes, E, b, 0]
            att = rf.edge_att[:E].clone()
        else:
            gsat.eval()                                                                # the eager tail, through the code run() takes
            att, _, _, _, mine = rf._forward(ub, 0)
            gsat.train()
        # the selection, on equal inputs: the bits the replay published go to the oracle's top-k (ties: lower edge id first)
        a = att.view(-1).cpu().numpy()
        top = xo.rank_oracle(a, cb.edge_index.numpy(), cb.batch.numpy(), b, k)[2].astype(bool) if k is not None else \
            xo.topk_ratio_oracle(a, cb.edge_index.numpy(), cb.batch.numpy(), b, ratio)
        with torch.no_grad():
            o_full = oclf64(cb.x.double(), cb.edge_index, cb.batch, None)
            o_keep, o_drop = (oclf64(s.x.double(), s.edge_index, s.batch, None)
                              for s in (so.extract_batch(cb, top, "edge", False)[0], so.extract_batch(cb, ~top, "edge", False)[0]))
        batch_bound = _bound(o_full, o_keep, o_drop)
        bound = max(bound, batch_bound)
        margin = float(o_full.abs().min())
        print(f"{backbone} batch of {b}: smallest |full logit| {margin:.4f}, |keep| {float(o_keep.abs().min()):.4f}, "
              f"|drop| {float(o_drop.abs().min()):.4f}; bound {batch_bound:.2e}")
        assert margin > 100 * batch_bound, "the margin condition the seed was picked for does not hold"
        if is_replay:
            assert np.array_equal(rf.topk[:E].cpu().numpy(), top)
            assert np.array_equal(rf.keep_batch.edge_mask[:E].cpu().numpy(), top) and not rf.keep_batch.edge_mask[E:].any()
            assert rf.keep_batch.valid.tolist() == [ub.num_nodes, int(top.sum()), b, 0]
            assert rf.drop_batch.valid.tolist() == [ub.num_nodes, E - int(top.sum()), b, 0]
            mine = (rf.logits_full[:b].clone(), rf.logits_keep[:b].clone(), rf.logits_drop[:b].clone())
            for name, z, ref in zip(("full", "keep", "drop"), mine, (o_full, o_keep, o_drop)):
                close(z, ref, what=f"{backbone} replayed logits_{name} vs the fp64 oracle")
        res = G.explanation_fidelity(gsat.clf, ub, att, k=k, ratio=ratio)
        theirs = (res["logits_full"], res["logits_keep"], res["logits_drop"])
        for name, z, ref in zip(("full", "keep", "drop"), theirs, (o_full, o_keep, o_drop)):
            close(z, ref, what=f"{backbone} eager logits_{name} vs the fp64 oracle")
        own.append(_probs(*mine))
        eager.append(_probs(*theirs))
        oracle.append(_probs(o_full, o_keep, o_drop))
        cls, p = eager[-1]
        assert abs(float(res["fidelity_plus"]) - float((p[:, 0] - p[:, 2]).mean())) <= 1e-6        # the existing function's own means
    assert gsat.training
    cat = lambda parts: _summary(torch.cat([c for c, _ in parts]), torch.cat([p for _, p in parts]))
    # through the replay's own logits the log must agree to fp64 rounding: this is the log's arithmetic alone
    for key, want in cat(own).items():
        assert abs(got[key] - want) <= 1e-12, ("own", key, got[key], want)
    # sigmoid is 1/4-Lipschitz: the logits' bound carries over to every probability and so to their means
    for name, want in (("eager", cat(eager)), ("oracle", cat(oracle))):
        for key in ("fidelity_plus", "fidelity_minus", "p_full", "p_keep", "p_drop"):
            print(f"{backbone} {name} {key}: {got[key]!r} / {want[key]!r}")
            assert abs(got[key] - want[key]) <= bound, (name, key, got[key], want[key])
        assert got["flip_plus"] == want["flip_plus"] and got["flip_minus"] == want["flip_minus"] and got["n"] == want["n"], name
    assert not rf.overflowed()
    G.clear_cache()


def _training_state(gsat, dev):
    opt = gsat.optimizer
    out = {"param." + n: p.detach().clone() for n, p in gsat.named_parameters()}
    out.update({"buffer." + n: b.detach().clone() for n, b in gsat.named_buffers()})
    for i, p in enumerate(p for grp in opt.param_groups for p in grp["params"]):
        for key, v in opt.state[p].items():
            if isinstance(v, torch.Tensor):
                out[f"adam.{i}.{key}"] = v.detach().clone()
    return out, seed_state(dev), torch.cuda.get_rng_state(dev).clone(), torch.get_rng_state().clone()


def test_a_fidelity_epoch_does_not_disturb_training(dev):
    """Three replayed training steps with a replayed fidelity epoch after each, and the same steps without: parameters, BatchNorm buffers,
    Adam state, the device seed state and torch's generator states are bitwise equal."""
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    steps = [IDS[:16], IDS[16:32], IDS[8:24]]
    runs = []
    for with_fidelity in (True, False):
        torch.manual_seed(99)
        torch.cuda.manual_seed(99)
        G.ops.device_seed(dev)              # the seed stream re-bases itself from the CPU generator after a manual_seed: once here in BOTH runs
        gsat, _ = _gsat(dev, "PNA", False, graphs)
        torch.manual_seed(7)
        rs = G.ReplayedStep(gsat, ds, SLOTS)
        rf = G.ReplayedFidelity(gsat, ds, SLOTS, ratio=0.3) if with_fidelity else None
        pin_seed_stream(dev, 0x5EED)
        for epoch, ids in enumerate(steps):
            rs.step(ids, epoch)
            if rf is not None:
                res = rf.run(np.asarray(IDS))
                assert np.isfinite(res["fidelity_plus"]) and res["n"] == len(IDS) and gsat.training
        torch.cuda.synchronize()
        runs.append(_training_state(gsat, dev))
    (a, seed_a, cuda_a, cpu_a), (b, seed_b, cuda_b, cpu_b) = runs
    assert set(a) == set(b) and any(k.startswith("adam.") for k in a) and any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0                              # the training steps drew, the fidelity epochs did not
    assert torch.equal(cuda_a, cuda_b) and torch.equal(cpu_a, cpu_b)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()


def test_ranked_graphs_leaves_the_padding_graph_out_and_needs_the_fused_path(dev):
    """On a padded batch whose padding edges carry the HIGHEST attention: with ``max_seg_edges`` and ``ranked_graphs`` the real slots of the
    mask are the top-k of the unpadded batch, in sync-free mode too; ``ranked_graphs`` without the bound, or on the radix path, raises
    instead of ranking padding edges inside the last real graph."""
    import dp_gsat_amd as G
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    ids = torch.tensor(IDS[:7], device=dev)
    ub = ds.collate(ids)
    E = ub.num_edges
    pb = ds.collate_padded(ids, (ub.num_nodes + 6, E + 37))
    bound = int(ds.edge_counts.max())
    att = torch.cat([torch.rand(E, generator=torch.Generator().manual_seed(4)), torch.full((37,), 2.0)]).to(dev)
    for k, ratio in ((5, None), (None, 0.3)):
        want = G.topk_edge_mask(att[:E], ub.edge_index, ub.batch, k=k, ratio=ratio, num_graphs=7)
        for sync_free in (False, True):
            G.clear_cache()
            G.set_sync_free(sync_free)
            try:
                got = G.topk_edge_mask(att, pb.edge_index, pb.batch, k=k, ratio=ratio, num_graphs=8, max_seg_edges=bound, ranked_graphs=7)
                for kw in (dict(ranked_graphs=7), dict(ranked_graphs=7, path="general"), dict(ranked_graphs=7, path="fused"),
                           dict(ranked_graphs=7, max_seg_edges=bound, path="general"), dict(ranked_graphs=9, max_seg_edges=bound)):
                    with pytest.raises(ValueError):
                        G.topk_edge_mask(att, pb.edge_index, pb.batch, k=k, ratio=ratio, num_graphs=8, **kw)
            finally:
                G.set_sync_free(False)
            assert torch.equal(got[:E], want), (k, ratio, sync_free)
    G.clear_cache()


def test_replayed_fidelity_refusals(dev, monkeypatch):
    import dp_gsat_amd as G
    from dp_gsat_amd import explain
    from dp_gsat_amd.encoders import BatchNorm1d
    graphs = _graphs()
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat, _ = _gsat(dev, "GIN", True, graphs)
    for kw in (dict(), dict(k=5, ratio=0.3)):
        with pytest.raises(ValueError, match="exactly one of k and ratio"):
            G.ReplayedFidelity(gsat, ds, SLOTS, **kw)
    with pytest.raises(ValueError, match="multi-label"):
        G.ReplayedFidelity(G.GSAT(gsat.clf, gsat.extractor, G.Criterion(2, True), None, learn_edge_att=True), ds, SLOTS, k=5)
    bns = [m for m in gsat.modules() if isinstance(m, BatchNorm1d)]
    bns[0].sync_group = True
    with pytest.raises(ValueError, match="sync_group"):
        G.ReplayedFidelity(gsat, ds, SLOTS, k=5)
    del bns[0].sync_group
    shared = {"learn_edge_att": False, "extractor_dropout_p": 0.5}
    mcfg = dict(pred_loss_coef=1, info_loss_coef=1, fix_r=False, decay_interval=10, decay_r=0.1, final_r=0.5)
    dual = G.DualGSAT(gsat.clf, G.ExtractorMLP(H, shared, "primal").to(dev), None, gsat.clf, G.ExtractorMLP(H, shared, "dual").to(dev), None,
                      mcfg, mcfg, False, False)
    with pytest.raises(ValueError, match="DualGSAT"):
        G.ReplayedFidelity(dual, ds, SLOTS, k=5)
    unlabelled = G.PackedDataset(ds.x_all, ds.edge_local_all, ds.node_ptr_all, ds.edge_ptr_all, None)
    with pytest.raises(ValueError, match="graph labels"):
        G.ReplayedFidelity(gsat, unlabelled, SLOTS, k=5)
    with monkeypatch.context() as mp:                                                  # a dataset whose largest graph the fused ranking cannot take
        mp.setattr(explain, "rank_edges_lds_cap", lambda: int(ds.edge_counts.max()) - 1)
        with pytest.raises(ValueError, match="rank_edges_lds_cap"):
            G.ReplayedFidelity(gsat, ds, SLOTS, k=5)
    n, e = po.totals(graphs, list(range(SLOTS)))
    for cap in ((n + 1, e), (n + 2, e - 1)):                                           # a capacity the first batch does not fit
        with pytest.raises(ValueError, match="do not fit the capacity"):
            G.ReplayedFidelity(gsat, ds, SLOTS, k=5, capacity=cap)
    assert ds.edge_label_all is None                                                   # no edge labels anywhere: ReplayedEval refuses this dataset
    with pytest.raises(ValueError):
        G.ReplayedEval(gsat, ds, SLOTS, 5)
    rf = G.ReplayedFidelity(gsat, ds, 5, k=5)                                          # and the plain model is taken
    with pytest.raises(ValueError, match="captured for 5"):
        rf.step([0, 1, 2], 0)
    rf.check_epoch(list(range(ds.num_graphs)))
    assert not G.graph_index.sync_free() and gsat.training
    G.clear_cache()
