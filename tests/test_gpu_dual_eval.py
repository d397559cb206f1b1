"""-m gpu: dual/primal evaluation epochs as replays of ReplayedDualEval's two captured graphs -- against the eager unpadded evaluation fed
the same Gumbel noise (regenerated from the predicted seed words), repeatability, the training run left bitwise alone, the dual
attention's scores, overflow and the refusals.  Floating-point comparisons follow tests.util.close (TOL = 1e-4)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import dual_oracle as do
from tests import padded_oracle as po
from tests.replay import pin_seed_stream, seed_next_ref
from tests.test_gpu_dual_replay import _dual_gsat, _dump, _pair_datasets
from tests.test_gpu_eval_log import HITS_KEY, _compare, _hits_differ_only_at_near_ties, _log_of, _training_state
from tests.util import TOL, assert_no_memset_nodes, close

pytestmark = pytest.mark.gpu
BATCH, K = 8, 5
EVAL_IDS = [33, 5, 12, 0, 27, 39, 8, 19, 2, 30, 31, 7, 22, 14, 36, 9, 11, 3, 25]          # two full batches and a tail of three
TRAIN_IDS = [[4, 5, 16, 20, 1, 37, 28, 10], EVAL_IDS[:8], EVAL_IDS[8:16]]
BASE = 0x1234_5678_9ABC_DEF1                                                               # above 2^32: both Philox key words matter
DUAL_KEYS = ("att_auroc", HITS_KEY, "delta_kl", "avg_signal_att_weights", "avg_bkg_att_weights")
MIX = dict(mix_after_epoch=1, dual_cfg=dict(decay_interval=1))                             # epochs 0 and 2: the unmixed and the mixed graph


def _reported_noise(word, M, dev):
    from dp_gsat_amd._lib import call, ptr, stream
    u = torch.empty(M, 1, device=dev)
    call("gsat_philox_gumbel_noise", int(word), M, ptr(u), stream())
    return u


def _eager_dual_eval(dg, ds, dual, ids, epoch, base, dev):
    """[(unpadded primal batch, primal edge attention [E, 1], logits, losses fp32[3])] of the eval-mode dual_forward_pass on the unpadded
    batches, batch j with the noise the sampler kernel draws for the seed word of counter (epoch << 32) + j, passed as a tensor."""
    import dp_gsat_amd as G
    out = []
    dg.eval()
    try:
        with torch.no_grad():
            for j, s in enumerate(range(0, len(ids), BATCH)):
                idt = torch.tensor(ids[s:s + BATCH], device=dev)
                ub, ud = ds.collate(idt), dual.collate(idt)
                U = _reported_noise(seed_next_ref(base, (epoch << 32) + j), ub.num_edges, dev)
                att, _, ld, logits = dg.dual_forward_pass(ub, ud, epoch, False, dual_noise=U)
                losses = torch.tensor([ld["loss"], ld["pred"], ld["info"]], dtype=torch.float32, device=dev)
                out.append((ub, G.ops.edge_tensor(att).clone(), logits.clone(), losses))
    finally:
        dg.train()
    return out


def _set_counter(ev, counter):
    ev.seed_state.copy_(torch.tensor([BASE, counter], dtype=torch.int64))


def _debug_graphs():
    out = []
    for _ in range(2):
        gr = torch.cuda.CUDAGraph()
        try:
            gr.enable_debug_mode()
        except Exception:
            pass
        out.append(gr)
    return out


def _same_result(a, b):
    assert set(a) == set(b)
    for key, v in a.items():
        if isinstance(v, dict):
            _same_result(v, b[key])
        elif isinstance(v, np.ndarray):
            assert v.dtype == b[key].dtype and np.array_equal(v.view(np.int64), b[key].view(np.int64)), key
        else:
            assert np.float64(v).view(np.int64) == np.float64(b[key]).view(np.int64), key


# ---- 1. replay against eager -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", ["GIN", "PNA"])
def test_replayed_dual_eval_scores_what_the_eager_evaluation_scores(dev, backbone):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=40)
    omods, mods, dg, _ = _dual_gsat(dev, backbone, graphs, False, **MIX)
    before = {k: v.detach().clone() for k, v in dg.state_dict().items()}
    modes = [m.training for m in dg.modules()]
    dbg = _debug_graphs()
    ev = G.ReplayedDualEval(dg, ds, dual, BATCH, K, seed=BASE, graphs=dbg)
    assert [m.training for m in dg.modules()] == modes and all(modes) and not G.graph_index.sync_free() and dg.sync_loss_dict
    assert not dg.keep_dual_att and dg.dual_att is None
    for k, v in dg.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert ev.log.state.tolist() == [0, 0, 0, 0] and ev.seed_state.tolist() == [BASE, 0] and ev.dual_log is None
    for which, gr in zip(("unmixed", "mixed"), dbg):
        assert_no_memset_nodes(_dump(gr), "ReplayedDualEval " + which)
    Np, Ep, Edc = cap = ds.pair_capacity_for(dual, BATCH)
    assert ev.capacity == cap
    first = None
    for epoch in (0, 2):
        got = ev.run(np.asarray(EVAL_IDS), epoch)
        assert ev.log.state.tolist()[1:] == [len(EVAL_IDS), 3, 0] and not any(k.startswith("dual_") for k in got)
        assert ev.seed_state.tolist() == [BASE, (epoch << 32) + 3] and dg.training and dg.sync_loss_dict
        eager = _eager_dual_eval(dg, ds, dual, EVAL_IDS, epoch, BASE, dev)
        want = _log_of(eager, ds, dev, K)
        own, moved = [], 0
        for j, (ub, att, logits, losses) in enumerate(eager[:2]):
            _set_counter(ev, (epoch << 32) + j)                           # the word run() drew for batch j
            ev.step(EVAL_IDS[j * BATCH:(j + 1) * BATCH], epoch)
            E, what = ub.num_edges, f"{backbone} epoch {epoch} batch {j}"
            N, E_, Ed = do.pair_totals(graphs, EVAL_IDS[j * BATCH:(j + 1) * BATCH])
            assert ev.batch.valid.tolist() == [N, E, BATCH, 0] and ev.dual_batch.valid.tolist() == [E, Ed, BATCH, 0] and E == E_
            assert ev.edge_att.shape == (Ep, 1) and ev.dual_att.shape == (Ep, 1) and ev.clf_logits.shape == (BATCH + 1, 1)
            assert abs(float(ev.r) - G.get_r(1, 0.1, epoch, final_r=0.5)) < 1e-6
            print(what, "max |edge_att - eager|", float((ev.edge_att[:E] - att).abs().max()), "losses", ev.losses.tolist(), losses.tolist())
            close(ev.edge_att[:E], att, TOL, what=what + ": edge_att")
            close(ev.clf_logits[:BATCH], logits, TOL, what=what + ": clf_logits")
            close(ev.losses, losses, TOL, what=what + ": losses")
            moved += _hits_differ_only_at_near_ties(ub, att, ev.edge_att[:E].clone(), K, what)
            own.append((ub, ev.edge_att[:E].clone(), ev.clf_logits[:BATCH].clone(), ev.losses.clone()))
        own.append(eager[2])                                               # the tail runs eagerly inside run(), too
        _compare(got, _log_of(own, ds, dev, K), True, f"{backbone} epoch {epoch} against the replay's own outputs")
        _compare(got, want, False, f"{backbone} epoch {epoch} against the eager evaluation")
        assert abs(got[HITS_KEY] - want[HITS_KEY]) <= moved / float(len(EVAL_IDS)) + 1e-12
        first = first or got
    assert first["loss"] != got["loss"] and first["info"] != got["info"]   # another r, and the mixed graph
    G.clear_cache()


# ---- 2. repeatability --------------------------------------------------------------------------------------------------------------------------
def test_an_evaluation_epoch_is_a_function_of_weights_ids_epoch_and_base(dev):
    """Default schedule (decay_interval 10, mix after epoch 50): epochs 0 and 1 have the same r and the same graph, so they differ through the
    noise alone."""
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=40)
    omods, mods, dg, _ = _dual_gsat(dev, "GIN", graphs, False)
    ev = G.ReplayedDualEval(dg, ds, dual, BATCH, K, seed=BASE)
    a = ev.run(EVAL_IDS, 0)
    other = ev.run(EVAL_IDS, 1)
    b = ev.run(EVAL_IDS, 0)
    _same_result(a, b)
    assert other["loss"] != a["loss"], "another epoch must draw other noise"
    assert G.ReplayedDualEval(dg, ds, dual, BATCH, K, seed=BASE + 1).run(EVAL_IDS, 0)["loss"] != a["loss"], "another base, other noise"
    # no noise in eval mode: nothing is drawn, the counter stays where run() put it, and the epoch no longer matters
    omods, mods, quiet, _ = _dual_gsat(dev, "GIN", graphs, False, gumbel_noise_in_eval=False)
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    ev = G.ReplayedDualEval(quiet, ds, dual, BATCH, K)                        # the base comes from torch.initial_seed(), without a draw
    assert ev.base == G.ReplayedDualEval(quiet, ds, dual, BATCH, K).base
    a = ev.run(EVAL_IDS, 3)
    assert ev.seed_state.tolist() == [ev.base, 3 << 32]
    _same_result(a, ev.run(EVAL_IDS, 4))
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    G.clear_cache()


# ---- 3. evaluation does not disturb training ---------------------------------------------------------------------------------------------------
def test_dual_evaluation_does_not_disturb_training(dev):
    """Three unpinned ReplayedDualStep steps (the third on the mixed graph) with a ReplayedDualEval.run after each, and the same steps
    without: parameters, buffers, both Adam states, the device seed stream and torch's CUDA generator state are bitwise equal.  (The CPU generator is checked around every evaluation instead:
    between the two runs it differs by the one draw that re-bases the device seed stream after the first torch.manual_seed(99).)"""
    import dp_gsat_amd as G
    from tests.replay import seed_state
    graphs, ds, dual = _pair_datasets(dev, count=40)
    runs = []
    for with_eval in (True, False):
        torch.manual_seed(99)
        omods, mods, dg, opts = _dual_gsat(dev, "GIN", graphs, True, **MIX)
        rs = G.ReplayedDualStep(dg, ds, dual, BATCH)
        ev = G.ReplayedDualEval(dg, ds, dual, BATCH, K) if with_eval else None
        pin_seed_stream(dev, 0x5EED)
        for epoch, ids in enumerate(TRAIN_IDS):
            rs.step(ids, epoch)
            if ev is not None:
                cpu_rng = torch.get_rng_state()
                res = ev.run(np.asarray(EVAL_IDS), epoch)
                assert np.isfinite(res["loss"]) and dg.training and torch.equal(torch.get_rng_state(), cpu_rng)
        torch.cuda.synchronize()
        state = {}
        for side, opt in (("primal", opts[0]), ("dual", opts[1])):
            got, _ = _training_state(NS(optimizer=opt, named_parameters=dg.named_parameters, named_buffers=dg.named_buffers), dev)
            state.update({side + "." + k if k.startswith("adam.") else k: v for k, v in got.items()})
        runs.append((state, seed_state(dev), torch.cuda.get_rng_state()))
    (a, seed_a, cuda_a), (b, seed_b, cuda_b) = runs
    assert set(a) == set(b) and any(k.startswith("primal.adam.") for k in a) and any(k.startswith("dual.adam.") for k in a)
    assert any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0                              # the training steps drew from the device stream, the evaluations did not
    assert torch.equal(cuda_a, cuda_b)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()


# ---- 4. the dual attention's scores -------------------------------------------------------------------------------------------------------------
def test_score_dual_logs_the_dual_attention_on_the_primal_edges(dev):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=40)
    omods, mods, dg, _ = _dual_gsat(dev, "GIN", graphs, False, **MIX)
    ev = G.ReplayedDualEval(dg, ds, dual, BATCH, K, score_dual=True, seed=BASE)
    assert ev.dual_log is not None and ev.dual_log.state.tolist() == [0, 0, 0, 0]
    ids = EVAL_IDS[:2 * BATCH]
    for epoch in (0, 2):
        got = ev.run(ids, epoch)
        assert {"dual_" + k for k in DUAL_KEYS} <= set(got) and ev.dual_log.state.tolist() == ev.log.state.tolist()
        fed, primal = [], []
        for j in range(2):
            part = ids[j * BATCH:(j + 1) * BATCH]
            _set_counter(ev, (epoch << 32) + j)
            ev.step(part, epoch)
            ub = ds.collate(torch.tensor(part, device=dev))
            E = ub.num_edges
            assert ev.dual_att.shape == ev.edge_att.shape and bool(((ev.dual_att >= 0) & (ev.dual_att <= 1)).all())
            if epoch == 2:          # the mixed graph: the primal attention carries mix_alpha of the dual one
                lifted = (ev.edge_att[:E] - dg.mix_alpha * ev.dual_att[:E]) / (1 - dg.mix_alpha)
                assert float(lifted.min()) >= -1e-6 and float(lifted.max()) <= 1 + 1e-6
            fed.append((ub, ev.dual_att[:E].clone(), ev.clf_logits[:BATCH].clone(), ev.losses.clone()))
            primal.append((ub, ev.edge_att[:E].clone(), ev.clf_logits[:BATCH].clone(), ev.losses.clone()))
        want = _log_of(fed, ds, dev, K)
        for key in DUAL_KEYS:
            print(f"epoch {epoch} dual_{key}: {got['dual_' + key]!r} / {want[key]!r}")
            exact = key in ("att_auroc", HITS_KEY)                         # functions of integer counts
            assert abs(got["dual_" + key] - want[key]) <= (1e-12 if exact else TOL * max(1.0, abs(want[key]))), key
        _compare(got, _log_of(primal, ds, dev, K), True, f"epoch {epoch}: the primal scores next to the dual ones")
        assert got["dual_avg_signal_att_weights"] != got["avg_signal_att_weights"]
    G.clear_cache()


# ---- 5. overflow -----------------------------------------------------------------------------------------------------------------------------------
def test_overflow_of_the_joint_capacity_is_flagged_and_raised(dev):
    import dp_gsat_amd as G
    graphs, ds, dual = _pair_datasets(dev, count=12)
    omods, mods, dg, _ = _dual_gsat(dev, "GIN", graphs, False)
    N, E, Ed = do.pair_totals(graphs, range(5))
    before = {k: v.detach().clone() for k, v in dg.state_dict().items()}
    with pytest.raises(ValueError, match="do not fit"):
        G.ReplayedDualEval(dg, ds, dual, 5, K, capacity=(N + 2, E, Ed - 1))
    for k, v in dg.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not G.graph_index.sync_free() and dg.sync_loss_dict and dg.training
    ev = G.ReplayedDualEval(dg, ds, dual, 5, K, capacity=(N + 2, E, Ed))
    big = [0, 1, 2, 6, 7]
    assert po.totals(graphs, big)[0] > N
    with pytest.raises(ValueError, match="capacity"):
        ev.check_epoch(big)
    ev.check_epoch([0, 1, 2, 3, 4])
    assert np.isfinite(ev.run([0, 1, 2, 3, 4], 0)["loss"])
    with pytest.raises(ValueError, match="bit 0"):
        ev.run(big, 0)
    assert ev.batch.valid.tolist() == [0, 0, 5, 1] and ev.dual_batch.valid.tolist() == [0, 0, 5, 1]
    assert ev.log.state.tolist() == [0, 0, 0, 1]                           # nothing was logged, flag bit 0
    assert np.isfinite(ev.run([4, 3, 2, 1, 0], 0)["loss"])                 # and the next run starts clean
    G.clear_cache()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_replayed_dual_eval_refusals(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd.encoders import BatchNorm1d
    graphs, ds, dual = _pair_datasets(dev, count=12)
    omods, mods, dg, _ = _dual_gsat(dev, "GIN", graphs, False)
    mk = lambda **kw: G.DualGSAT(mods[0], mods[1], None, mods[2], mods[3], None, do.MCFG, do.MCFG, kw.pop("pe", False), kw.pop("de", False),
                                 **kw).train()
    before = {k: v.detach().clone() for k, v in dg.state_dict().items()}
    other = G.PackedDataset.from_data_list(do.labelled_graphs(count=12), dev)          # node counts are not ds.edge_counts
    unlabelled = G.PackedDataset.from_data_list(po.mutag_graphs(count=12), dev)         # no edge labels
    no_y = G.PackedDataset(ds.x_all, ds.edge_local_all, ds.node_ptr_all, ds.edge_ptr_all, None, None, ds.edge_label_all)
    plain = G.GSAT(mods[0], G.ExtractorMLP(do.H, False).to(dev), G.Criterion(2, False), None, learn_edge_att=False)
    bns = [m for m in dg.modules() if isinstance(m, BatchNorm1d)]
    assert bns
    cases = [("multi-label", lambda: G.ReplayedDualEval(mk(primal_multi_label=True), ds, dual, 5, K)),
             ("multi-label", lambda: G.ReplayedDualEval(mk(dual_multi_label=True), ds, dual, 5, K)),
             ("edge attention", lambda: G.ReplayedDualEval(mk(pe=True), ds, dual, 5, K)),
             ("edge attention", lambda: G.ReplayedDualEval(mk(de=True), ds, dual, 5, K)),
             ("dual_forward_pass", lambda: G.ReplayedDualEval(plain, ds, dual, 5, K)),
             ("labels", lambda: G.ReplayedDualEval(dg, unlabelled, unlabelled.line_graph_dataset(), 5, K)),
             ("labels", lambda: G.ReplayedDualEval(dg, no_y, no_y.line_graph_dataset(), 5, K)),
             ("not a dual", lambda: G.ReplayedDualEval(dg, ds, other, 5, K)),
             ("capacity is", lambda: G.ReplayedDualEval(dg, ds, dual, 5, K, capacity=(400, 800))),
             ("batch_size", lambda: G.ReplayedDualEval(dg, ds, dual, 0, K)),
             ("batch_size", lambda: G.ReplayedDualEval(dg, ds, dual, 13, K))]
    for match, make in cases:
        with pytest.raises(ValueError, match=match):
            make()
    bns[0].sync_group = True
    try:
        with pytest.raises(ValueError, match="sync_group"):
            G.ReplayedDualEval(dg, ds, dual, 5, K)
    finally:
        del bns[0].sync_group
    for k, v in dg.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not G.graph_index.sync_free() and dg.sync_loss_dict and dg.training
    with pytest.raises(ValueError, match="DualGSAT"):                     # the single-model evaluator keeps refusing the pair
        G.ReplayedEval(dg, ds, 5, K)
    ev = G.ReplayedDualEval(dg, ds, dual, 5, K)                            # and the supported configuration is taken
    with pytest.raises(ValueError, match="captured for 5"):
        ev.step([0, 1, 2], 0)
    G.clear_cache()
