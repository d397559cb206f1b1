"""gpu: the fidelity curves of the dual/primal pair's two explanations as replays of ReplayedDualFidelityCurve's two captured graphs --
against the eager ``explanation_fidelity_curves`` on the same batches with the same seed words, repeatability, the training run left
bitwise alone, the mixed graph, ragged batches, and the refusals.

The probability bound is measured, not derived: the rows of a graph sit at other positions of the stacked GEMMs in the replay's
13-variant padded stack than in the eager unpadded stacks, so their logits round differently.  An MI355X run of
``test_run_equals_the_eager_curves_on_the_same_batches`` printed the worst relative gap of a graph's probability between the multi stack
of the replay and ``explanation_fidelity_curve`` run per ranking: 0.000e+00 on every batch of both epochs (and 0.000e+00 against the eager
multi stack) -- at these shapes a row's logits do not depend on its position.  The bound is 4 x that, the margin of
tests/test_gpu_fidelity_curve_log.py, so the probabilities are asserted bitwise equal.  The closest a graph's
probability came to the decision boundary was 4.2e-05, so no class sits on a rounding edge either."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import dual_oracle as do
from tests import fidelity_curve_oracle as fco
from tests import fidelity_multi_oracle as fmo
from tests import padded_oracle as po
from tests.replay import pin_seed_stream, seed_next_ref
from tests.test_gpu_dual_eval import BASE, MIX, _reported_noise, _set_counter
from tests.test_gpu_dual_replay import _dual_gsat, _pair_datasets
from tests.test_gpu_eval_log import _training_state
from tests.util import TOL, close

pytestmark = pytest.mark.gpu
BATCH, RATIOS, S, R = 5, [0.2, 0.5, 0.8], 3, 2
V = 1 + 2 * R * S
IDS = [3, 7, 0, 9, 5, 1, 11, 4, 8, 2]                      # two full batches
TAIL = IDS + [6, 10]                                       # and a tail of two
P_GAP = 0.0                                                # measured on an MI355X: every probability came out bitwise equal
P_RTOL = 4 * P_GAP
PER_LEVEL = ("fidelity_plus", "fidelity_minus", "p_keep", "p_drop", "flip_plus", "flip_minus", "kept_fraction")


def _make(dev, count=12, **kw):
    graphs, ds, dual = _pair_datasets(dev, count=count)
    omods, mods, dg, opts = _dual_gsat(dev, "GIN", graphs, kw.pop("optimizers", False), **kw)
    return graphs, ds, dual, mods, dg, opts


def _same_result(a, b):
    """Bitwise: every float of the nested result, as its int64 pattern."""
    if isinstance(a, dict):
        assert set(a) == set(b)
        for key in a:
            _same_result(a[key], b[key])
    else:
        x, y = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64)), (a, b)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b))) if b.size else 0.0


def test_run_equals_the_eager_curves_on_the_same_batches(dev):
    import dp_gsat_amd as G
    graphs, ds, dual, mods, dg, _ = _make(dev, **MIX)
    before = {k: v.detach().clone() for k, v in dg.state_dict().items()}
    modes = [m.training for m in dg.modules()]
    ev = G.ReplayedDualFidelityCurve(dg, ds, dual, BATCH, ratios=RATIOS, seed=BASE)
    assert [m.training for m in dg.modules()] == modes and not G.graph_index.sync_free() and dg.sync_loss_dict
    assert not dg.keep_dual_att and dg.dual_att is None and ev.seed_state.tolist() == [BASE, 0]
    for k, v in dg.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert ev.log.state.tolist() == [0] * 20 and not ev.overlap.any() and ev.log.rankings == 2 and ev.log.variants == V
    Np, Ep, _ = ev.capacity
    clf = dg.primal_clf
    worst_multi = worst_single = 0.0
    for epoch in (0, 2):
        got = ev.run(np.asarray(IDS), epoch)
        assert ev.seed_state.tolist() == [BASE, (epoch << 32) + 2] and dg.training and not ev.overflowed()
        assert set(got) == {"primal", "dual", "jaccard", "overlap", "p_full", "n"} and got["n"] == len(IDS)
        log_cls, log_p = ev.log.cls[:len(IDS)].cpu().numpy(), ev.log.p[:len(IDS)].cpu().numpy()
        sums = {key: np.zeros((R, S)) for key in PER_LEVEL}
        p_full, edges, counts = 0.0, 0, np.zeros((S, 3), np.int64)
        for j in range(2):
            part = IDS[j * BATCH:(j + 1) * BATCH]
            idt = torch.tensor(part, device=dev)
            _set_counter(ev, (epoch << 32) + j)                                        # the word run() drew for batch j
            ev.step(part, epoch)
            ub, ud = ds.collate(idt), dual.collate(idt)
            E, what = ub.num_edges, f"epoch {epoch} batch {j}"
            assert ev.batch.valid.tolist()[1:] == [E, BATCH, 0] and ev.edge_att.shape == ev.dual_att.shape == (Ep, 1)
            assert tuple(ev.edge_level.shape) == (R, Ep) and ev.logits.shape[0] == V * (BATCH + 1) and ev.stack.variants == V
            # the attentions are those of the eager evaluation fed the noise of the same seed word
            U = _reported_noise(seed_next_ref(BASE, (epoch << 32) + j), E, dev)
            dg.eval()
            dg.keep_dual_att = True
            try:
                with torch.no_grad():
                    att_e = G.ops.edge_tensor(dg.dual_forward_pass(ub, ud, epoch, False, dual_noise=U)[0]).clone()
                    datt_e = dg.dual_att[:E].clone()
            finally:
                dg.keep_dual_att, dg.dual_att = False, None
                dg.train()
            close(ev.edge_att[:E], att_e, TOL, what=what + ": edge_att")
            close(ev.dual_att[:E], datt_e, TOL, what=what + ": dual_att")
            atts = [ev.edge_att[:E].clone(), ev.dual_att[:E].clone()]
            eager = G.explanation_fidelity_curves(clf, ub, atts, ratios=RATIOS, batch_size=BATCH)
            assert tuple(eager["fidelity_plus"].shape) == (R, S) and float(eager["n"]) == BATCH
            cls_r, p_r = fco.rows(ev.logits.cpu().numpy(), BATCH + 1, R * S, BATCH)
            cls_e, p_e = fco.rows(eager["logits"].reshape(V * (BATCH + 1), -1).cpu().numpy(), BATCH + 1, R * S, BATCH)
            gap = _rel(p_r, p_e)
            worst_multi = max(worst_multi, gap)
            print(what, f"worst relative gap of a probability, replayed stack against the eager multi stack: {gap:.3e}")
            margin = float(np.min(np.abs(p_e - 0.5)))
            print(what, f"closest probability to the decision boundary: {margin:.3e}")
            for r in range(R):
                one = G.explanation_fidelity_curve(clf, ub, atts[r], ratios=RATIOS)
                cls_1, p_1 = fco.rows(one["logits"].reshape((2 * S + 1) * (BATCH + 1), -1).cpu().numpy(), BATCH + 1, S, BATCH)
                place = [0] + [fmo.variant_index(R, S, r, s, True) for s in range(S)] + [fmo.variant_index(R, S, r, s, False) for s in range(S)]
                gap = _rel(p_r[:, place], p_1)
                worst_single = max(worst_single, gap)
                print(what, f"ranking {r}: worst relative gap to explanation_fidelity_curve on its own: {gap:.3e}")
                assert np.array_equal(cls_r[:, place], cls_1), (what, r)
                assert gap <= P_RTOL, (what, r, gap)
            assert np.array_equal(cls_r, cls_e), what                                  # classes are exact
            assert np.array_equal(log_cls[j * BATCH:(j + 1) * BATCH], cls_r), what     # and run() logged this very batch
            assert _rel(log_p[j * BATCH:(j + 1) * BATCH], p_r) <= 1e-14, what
            for key in PER_LEVEL[:6]:
                sums[key] += eager[key].cpu().numpy() * BATCH
            kept = eager["kept_fraction"].cpu().numpy() * E
            assert np.max(np.abs(kept - np.round(kept))) < 1e-9 and int(ev.stack.valid[0, 1]) == E
            assert np.array_equal(np.round(kept).astype(np.int64).reshape(-1), ev.stack.valid[1:1 + R * S, 1].cpu().numpy())     # exact
            sums["kept_fraction"] += np.round(kept)
            p_full += float(eager["p_full"]) * BATCH
            edges += E
            counts += fmo.overlap_counts(ev.edge_level[0].cpu().numpy(), ev.edge_level[1].cpu().numpy(), S, E)
            c = fmo.overlap_counts(ev.edge_level[0].cpu().numpy(), ev.edge_level[1].cpu().numpy(), S, E).astype(np.float64)
            close(eager["jaccard"], torch.from_numpy(c[:, 0] / np.maximum(c[:, 1] + c[:, 2] - c[:, 0], 1)), 1e-12, what=what + ": jaccard")
            close(eager["overlap"], torch.from_numpy(c[:, 0] / np.maximum(np.minimum(c[:, 1], c[:, 2]), 1)), 1e-12, what=what + ": overlap")
        n = len(IDS)
        for r, name in enumerate(("primal", "dual")):
            res = got[name]
            assert res["levels"] == RATIOS and res["n"] == n and res["p_full"] == got["p_full"]
            for key in ("flip_plus", "flip_minus"):
                assert res[key] == [int(round(v)) / n for v in sums[key][r]], (epoch, name, key)
            assert res["kept_fraction"] == [int(v) / edges for v in sums["kept_fraction"][r]], (epoch, name)
            for key in ("fidelity_plus", "fidelity_minus", "p_keep", "p_drop"):
                # a mean of probabilities each within P_RTOL of the eager one's; a fidelity is a difference of two such
                assert np.max(np.abs(np.asarray(res[key]) - sums[key][r] / n)) <= 2 * (P_RTOL + n * 2.0 ** -53), (epoch, name, key)
        assert abs(got["p_full"] - p_full / n) <= P_RTOL + n * 2.0 ** -53
        assert got["jaccard"] == [c[0] / (c[1] + c[2] - c[0]) if c[1] + c[2] - c[0] else 0.0 for c in counts.tolist()]
        assert got["overlap"] == [c[0] / min(c[1], c[2]) if min(c[1], c[2]) else 0.0 for c in counts.tolist()]
        assert 0.0 < got["jaccard"][-1] <= 1.0 and all(0.0 <= v <= 1.0 for v in got["jaccard"] + got["overlap"])
    print(f"worst relative gap over the file: multi against eager multi {worst_multi:.3e}, multi against per-ranking {worst_single:.3e}")
    assert worst_multi <= P_RTOL
    G.clear_cache()


def test_a_curve_epoch_is_repeatable(dev):
    import dp_gsat_amd as G
    graphs, ds, dual, mods, dg, _ = _make(dev, **MIX)
    ev = G.ReplayedDualFidelityCurve(dg, ds, dual, BATCH, ratios=RATIOS, seed=BASE)
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    a = ev.run(TAIL, 0)
    other = ev.run(TAIL, 1)
    b = ev.run(TAIL, 0)
    _same_result(a, b)                                                                 # bitwise, the eager tail included
    assert a["n"] == len(TAIL) and ev.seed_state.tolist() == [BASE, 3]
    assert other["dual"] != a["dual"], "another epoch must draw other noise"
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    G.clear_cache()


def test_a_curve_epoch_does_not_disturb_training(dev):
    """Three ReplayedDualStep steps (the third on the mixed graph) with a curve epoch after each, and the same steps without:
    parameters, BatchNorm buffers, both Adam states, the device seed stream and torch's CUDA generator end bitwise equal."""
    import dp_gsat_amd as G
    from tests.replay import seed_state
    graphs, ds, dual = _pair_datasets(dev, count=12)
    train_ids = [[4, 5, 6, 10, 1], IDS[:5], IDS[5:]]
    runs = []
    for with_curve in (True, False):
        torch.manual_seed(99)
        omods, mods, dg, opts = _dual_gsat(dev, "GIN", graphs, True, **MIX)
        rs = G.ReplayedDualStep(dg, ds, dual, BATCH)
        ev = G.ReplayedDualFidelityCurve(dg, ds, dual, BATCH, ratios=RATIOS) if with_curve else None
        pin_seed_stream(dev, 0x5EED)
        for epoch, ids in enumerate(train_ids):
            rs.step(ids, epoch)
            if ev is not None:
                cpu_rng = torch.get_rng_state()
                res = ev.run(np.asarray(TAIL), epoch)
                assert np.isfinite(res["p_full"]) and dg.training and torch.equal(torch.get_rng_state(), cpu_rng)
        torch.cuda.synchronize()
        state = {}
        for side, opt in (("primal", opts[0]), ("dual", opts[1])):
            got, _ = _training_state(NS(optimizer=opt, named_parameters=dg.named_parameters, named_buffers=dg.named_buffers), dev)
            state.update({side + "." + k if k.startswith("adam.") else k: v for k, v in got.items()})
        runs.append((state, seed_state(dev), torch.cuda.get_rng_state()))
    (a, seed_a, cuda_a), (b, seed_b, cuda_b) = runs
    assert set(a) == set(b) and any(k.startswith("primal.adam.") for k in a) and any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0 and torch.equal(cuda_a, cuda_b)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()


def test_the_mixed_graph_runs_after_mix_after_epoch(dev):
    import dp_gsat_amd as G
    graphs, ds, dual, mods, dg, _ = _make(dev, **MIX)
    ev = G.ReplayedDualFidelityCurve(dg, ds, dual, BATCH, ratios=RATIOS, seed=BASE)
    part = IDS[:BATCH]
    E = ds.collate(torch.tensor(part, device=dev)).num_edges
    seen = {}
    for epoch in (0, 1, 2):                                # mix_after_epoch = 1: only epoch 2 is mixed
        _set_counter(ev, 7)                                # the same seed word: the dual attention is the same
        ev.step(part, epoch)
        seen[epoch] = (ev.edge_att[:E].clone(), ev.dual_att[:E].clone(), ev.edge_level[:, :E].clone())
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][2], seen[1][2])
    assert torch.equal(seen[0][1], seen[2][1]) and torch.equal(seen[0][2][1], seen[2][2][1])
    close(seen[2][0], dg.mix_alpha * seen[2][1] + (1 - dg.mix_alpha) * seen[0][0], 1e-6, what="the mixed primal attention")
    assert not torch.equal(seen[0][0], seen[2][0]) and not torch.equal(seen[0][2][0], seen[2][2][0])          # ranking 0 moves with the mix
    assert ev.run(IDS, 0)["primal"] != ev.run(IDS, 2)["primal"]
    G.clear_cache()


def test_ragged_mode_replays_every_batch(dev):
    import dp_gsat_amd as G
    graphs, ds, dual, mods, dg, _ = _make(dev, **MIX)
    cap = ds.pair_capacity_for(dual, 3)                    # room for about three graphs in five slots
    ev = G.ReplayedDualFidelityCurve(dg, ds, dual, BATCH, ratios=RATIOS, capacity=cap, seed=BASE, ragged=True)
    perm = torch.tensor([3, 7, 0, 9, 5, 1, 11, 4, 8, 2, 6, 10])
    rows = ev.batches(perm)
    assert rows.shape[1] == BATCH and int((rows >= 0).sum()) == 12
    a = ev.run(perm, 0)
    assert a["n"] == 12 and ev.log.state.tolist()[:3] == [12, rows.shape[0], 0] and not ev.overflowed()
    assert ev.seed_state.tolist() == [BASE, rows.shape[0]]
    _same_result(a, ev.run(perm, 0))
    with pytest.raises(ValueError, match="capacity"):      # check_epoch takes full batches of five: they do not fit room for three
        ev.check_epoch(perm[:10])
    N, E, Ed = do.pair_totals(graphs, range(BATCH))
    with pytest.raises(ValueError, match="do not fit"):
        G.ReplayedDualFidelityCurve(dg, ds, dual, BATCH, ratios=RATIOS, capacity=(N + 2, E, Ed - 1))
    fixed = G.ReplayedDualFidelityCurve(dg, ds, dual, BATCH, ratios=RATIOS, capacity=(N + 2, E, Ed), seed=BASE)
    big = [0, 1, 2, 6, 7]
    assert po.totals(graphs, big)[0] > N
    fixed.check_epoch([0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="capacity"):
        fixed.check_epoch(big)
    with pytest.raises(ValueError, match="bit 0"):
        fixed.run(big, 0)
    assert fixed.overflowed() and not fixed.overflowed()
    assert fixed.run([4, 3, 2, 1, 0], 0)["n"] == BATCH     # and the next run starts clean
    G.clear_cache()


def test_refusals(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd.encoders import BatchNorm1d
    graphs, ds, dual, mods, dg, _ = _make(dev)
    mk = lambda **kw: G.DualGSAT(mods[0], mods[1], None, mods[2], mods[3], None, do.MCFG, do.MCFG, kw.pop("pe", False), kw.pop("de", False),
                                 **kw).train()
    before = {k: v.detach().clone() for k, v in dg.state_dict().items()}
    other = G.PackedDataset.from_data_list(do.labelled_graphs(count=12), dev)          # node counts are not ds.edge_counts
    unlabelled = G.PackedDataset.from_data_list(po.mutag_graphs(count=12), dev)         # no edge labels
    no_y = G.PackedDataset(ds.x_all, ds.edge_local_all, ds.node_ptr_all, ds.edge_ptr_all, None, None, ds.edge_label_all)
    plain = G.GSAT(mods[0], G.ExtractorMLP(do.H, False).to(dev), G.Criterion(2, False), None, learn_edge_att=False)
    new = G.ReplayedDualFidelityCurve
    cases = [("multi-label", lambda: new(mk(primal_multi_label=True), ds, dual, 5, ratios=RATIOS)),
             ("multi-label", lambda: new(mk(dual_multi_label=True), ds, dual, 5, ratios=RATIOS)),
             ("edge attention", lambda: new(mk(pe=True), ds, dual, 5, ratios=RATIOS)),
             ("edge attention", lambda: new(mk(de=True), ds, dual, 5, ratios=RATIOS)),
             ("dual_forward_pass", lambda: new(plain, ds, dual, 5, ratios=RATIOS)),
             ("edge_label", lambda: new(dg, unlabelled, unlabelled.line_graph_dataset(), 5, ratios=RATIOS)),
             ("graph labels", lambda: new(dg, no_y, no_y.line_graph_dataset(), 5, ratios=RATIOS)),
             ("not a dual", lambda: new(dg, ds, other, 5, ratios=RATIOS)),
             ("capacity is", lambda: new(dg, ds, dual, 5, ratios=RATIOS, capacity=(400, 800))),
             ("batch_size", lambda: new(dg, ds, dual, 0, ratios=RATIOS)),
             ("at most 16", lambda: new(dg, ds, dual, 5, ks=list(range(1, 10)))),                   # 2 * S = 18
             ("exactly one", lambda: new(dg, ds, dual, 5)),
             ("exactly one", lambda: new(dg, ds, dual, 5, ks=[1], ratios=[0.5])),
             ("strictly increasing", lambda: new(dg, ds, dual, 5, ratios=[0.5, 0.5])),
             ("ratios must lie", lambda: new(dg, ds, dual, 5, ratios=[0.5, 1.5]))]
    for match, make in cases:
        with pytest.raises(ValueError, match=match):
            make()
    bns = [m for m in dg.modules() if isinstance(m, BatchNorm1d)]
    bns[0].sync_group = True
    try:
        with pytest.raises(ValueError, match="sync_group"):
            new(dg, ds, dual, 5, ratios=RATIOS)
    finally:
        del bns[0].sync_group
    import dp_gsat_amd.explain as X
    cap_fn = X.rank_edges_lds_cap
    X.rank_edges_lds_cap = lambda: 3                       # every graph here has more edges than that
    try:
        with pytest.raises(ValueError, match="rank_edges_lds_cap"):
            new(dg, ds, dual, 5, ratios=RATIOS)
    finally:
        X.rank_edges_lds_cap = cap_fn
    for k, v in dg.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not G.graph_index.sync_free() and dg.sync_loss_dict and dg.training
    with pytest.raises(ValueError, match="DualGSAT fidelity is not covered"):           # the single-model class keeps refusing the pair
        G.ReplayedFidelityCurve(dg, ds, 5, ratios=RATIOS)
    with pytest.raises(ValueError, match="DualGSAT fidelity is not covered"):
        G.ReplayedFidelity(dg, ds, 5, ratio=0.5)
    ev = new(dg, ds, dual, 5, ks=list(range(1, 9)))                                      # 2 * S = 16: the limit is taken
    assert ev.log.variants == 33
    with pytest.raises(ValueError, match="captured for 5"):
        ev.step([0, 1, 2], 0)
    G.clear_cache()
