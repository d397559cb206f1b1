"""-m gpu: the device log of an evaluation epoch (EpochLog), the per-segment delta-KL, and evaluation as replays of one captured
hipGraph (ReplayedEval)."""
import os
import tempfile
import warnings

import numpy as np
import pytest
import torch

from tests import eval_log_oracle as lo
from tests import explain_oracle as xo
from tests import padded_oracle as po
from tests.replay import pin_seed_stream, seed_state
from tests.util import TOL, assert_no_memset_nodes, close

pytestmark = pytest.mark.gpu
SENT = lo.LogOracle.SENTINEL
PAD = 64                                   # guard entries in front of and behind every log array
INT_KEYS = ("att_auroc", "bkg_att_hist", "signal_att_hist", "att_outside", "clf_acc", "clf_roc")       # functions of integer counts only
HITS_KEY = "precision@5"                   # mean of the integer per-graph hits / k: a step function of the attention, like the keys above
FLOAT_KEYS = ("delta_kl", "avg_signal_att_weights", "avg_bkg_att_weights", "loss", "pred", "info")       # continuous in the forward's outputs
ARRAYS = ("att", "label", "graph_edge_ptr", "logits", "y", "batch_edge_ptr")


def _guard(log):
    """Move every array of ``log`` into the middle of a larger buffer filled with the sentinel byte; returns name -> buffer."""
    bufs = {}
    for name in ARRAYS:
        t = getattr(log, name)
        big = torch.empty((t.shape[0] + 2 * PAD,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        big.view(torch.uint8).fill_(SENT)
        setattr(log, name, big[PAD:PAD + t.shape[0]])
        assert getattr(log, name).is_contiguous()
        bufs[name] = big
    return bufs


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().reshape(-1)


def _assert_log_equals(log, bufs, oracle, what):
    """Every array bit for bit (the oracle's are prefilled with the same sentinel: this covers the prefix AND everything beyond it), the
    guard entries around the arrays, and the state."""
    torch.cuda.synchronize()
    for name, want in oracle.arrays().items():
        got = _bytes(getattr(log, name))
        assert np.array_equal(got, want.reshape(-1).view(np.uint8)), f"{what}: {name}"
        whole = _bytes(bufs[name])
        row = whole.size // bufs[name].shape[0]
        assert (whole[:PAD * row] == SENT).all() and (whole[whole.size - PAD * row:] == SENT).all(), f"{what}: {name} written out of bounds"
    assert log.state.tolist() == oracle.state.tolist(), what
    np.testing.assert_array_equal(log.loss_sums.cpu().numpy(), oracle.loss_sums, err_msg=what)


# ---- 1. append layout ---------------------------------------------------------------------------------------------------------------------
# edge totals 0, 1, 3, 64, 65, 257 -> running offsets 0, 0, 1, 4, 68, 133: odd byte offsets for the labels, floats off 16-byte alignment;
# graph counts 1, 2, 5
LAYOUT_COUNTS = ([0], [1, 0], [3], [10, 20, 0, 30, 4], [33, 32], [100, 57, 0, 1, 99])


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "counts-from-valid"])
@pytest.mark.parametrize("logit_cols,y_cols", [(1, 1), (3, 2)])
def test_append_layout_is_bit_exact(dev, logit_cols, y_cols, padded):
    """Batches with interleaved edge ids appended one after the other; after each append every array equals the oracle's bit for bit.
    ``padded``: the last graph of every batch plays the padding graph and a ``valid`` tensor gives the counts (a batch of one graph then
    logs nothing but the batch itself)."""
    import dp_gsat_amd as G
    assert [sum(c) for c in LAYOUT_COUNTS] == [0, 1, 3, 64, 65, 257] and sorted({len(c) for c in LAYOUT_COUNTS}) == [1, 2, 5]
    G_all, E_all = sum(len(c) for c in LAYOUT_COUNTS), sum(sum(c) for c in LAYOUT_COUNTS)
    log = G.EpochLog(5, G_all + 2, E_all + 5, len(LAYOUT_COUNTS) + 1, logit_cols, y_cols, device=dev)
    bufs = _guard(log)
    oracle = lo.LogOracle(5, G_all + 2, E_all + 5, len(LAYOUT_COUNTS) + 1, logit_cols, y_cols)
    with_losses = logit_cols == 1
    for i, counts in enumerate(LAYOUT_COUNTS):
        b = xo.custom_batch(counts, seed=100 + i)
        rng = np.random.RandomState(200 + i)
        E, Gb = b.num_edges, b.num_graphs
        if len(counts) > 1 and E > 2:                                      # the edges-by-graph order is a real permutation
            assert not np.array_equal(np.argsort(b.batch.numpy()[b.edge_index.numpy()[0]], kind="stable"), np.arange(E))
        att = rng.rand(E).astype(np.float32)
        lab = (rng.rand(E) < 0.4).astype(np.uint8)
        z = rng.randn(Gb, logit_cols).astype(np.float32)
        y = (rng.rand(Gb, y_cols) < 0.5).astype(np.float32)
        if y_cols > 1:
            y[rng.rand(Gb, y_cols) < 0.3] = np.nan
        losses = rng.rand(3).astype(np.float32) if with_losses else None
        b.edge_label, b.y = torch.from_numpy(lab), torch.from_numpy(y)
        d = b.to(dev)
        real = None
        if padded:
            real = Gb - 1
            d.valid = torch.tensor([6 * real, E - counts[-1], real, 0], dtype=torch.int32, device=dev)
        log.append(torch.from_numpy(att).view(-1, 1).to(dev), d, torch.from_numpy(z).to(dev),
                   torch.from_numpy(losses).to(dev) if with_losses else None)
        oracle.append(att, lab, b.edge_index.numpy(), b.batch.numpy(), Gb, z, y, losses, real_graphs=real)
        _assert_log_equals(log, bufs, oracle, f"append {i} {counts}")
    assert oracle.state[2] == len(LAYOUT_COUNTS) and oracle.state[3] == 0
    log.reset()
    assert log.state.tolist() == [0, 0, 0, 0] and log.loss_sums.tolist() == [0.0, 0.0, 0.0]
    G.clear_cache()


# ---- 2. flags -----------------------------------------------------------------------------------------------------------------------------
def _labelled_graphs(count, **kw):
    graphs = po.mutag_graphs(count, **kw)
    rng = np.random.RandomState(5)
    for g in graphs:
        g.edge_label = torch.from_numpy((rng.rand(g.edge_index.shape[1]) < 0.3).astype(np.float32))
    return graphs


def _random_batch(counts, seed, dev):
    b = xo.custom_batch(counts, seed=seed)
    rng = np.random.RandomState(seed + 1)
    b.edge_label = torch.from_numpy((rng.rand(b.num_edges) < 0.4).astype(np.uint8))
    b.y = torch.from_numpy((rng.rand(b.num_graphs, 1) < 0.5).astype(np.float32))
    att = torch.from_numpy(rng.rand(b.num_edges).astype(np.float32)).to(dev)
    return b.to(dev), att, torch.from_numpy(rng.randn(b.num_graphs, 1).astype(np.float32)).to(dev)


def test_refused_appends_write_nothing_and_set_their_flag(dev):
    """A padded batch whose overflow word is set (a capacity one node short: the existing mechanism) -> flag bit 0; a log with max_edges,
    max_graphs or max_batches one short, in turn -> flag bit 1.  In every case nothing is written (the arrays and the guard entries
    around them keep their bytes), the counts in ``state`` stay and compute() raises."""
    import dp_gsat_amd as G
    graphs = _labelled_graphs(**po.LAYOUT_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    N, E = po.totals(graphs, po.LAYOUT_IDS)
    ids = torch.tensor(po.LAYOUT_IDS, device=dev)
    G.set_sync_free(True)                                    # outside sync-free mode collate_padded raises instead of marking the batch
    try:
        short = ds.collate_padded(ids, (N + 1, E))
    finally:
        G.set_sync_free(False)
    assert short.valid.tolist() == [0, 0, 5, 1]
    log = G.EpochLog(5, 20, 4 * E, 4, 1, device=dev)
    bufs = _guard(log)
    fits = ds.collate_padded(ids, (N + 2, E))
    att, z = torch.rand(E, 1, device=dev), torch.randn(6, 1, device=dev)
    log.append(att, fits, z)
    torch.cuda.synchronize()
    assert log.state.tolist() == [E, 5, 1, 0]
    snap = {n: _bytes(bufs[n]).copy() for n in ARRAYS}
    log.append(att, short, z)
    torch.cuda.synchronize()
    assert log.state.tolist() == [E, 5, 1, 1]
    for n in ARRAYS:
        assert np.array_equal(_bytes(bufs[n]), snap[n]), n
    with pytest.raises(ValueError, match="bit 0"):
        log.compute()

    first, second = _random_batch([5, 7, 3], 300, dev), _random_batch([4, 0, 9, 2], 310, dev)
    (Ea, Ga), (Eb, Gb) = ((b.num_edges, b.num_graphs) for b, _, _ in (first, second))
    for what, caps in (("max_edges", (Ga + Gb, Ea + Eb - 1, 2)), ("max_graphs", (Ga + Gb - 1, Ea + Eb, 2)), ("max_batches", (Ga + Gb, Ea + Eb, 1))):
        log = G.EpochLog(5, caps[0], caps[1], caps[2], 1, device=dev)
        bufs = _guard(log)
        log.append(first[1], first[0], first[2])
        torch.cuda.synchronize()
        assert log.state.tolist() == [Ea, Ga, 1, 0], what
        snap = {n: _bytes(bufs[n]).copy() for n in ARRAYS}
        log.append(second[1], second[0], second[2])
        torch.cuda.synchronize()
        assert log.state.tolist() == [Ea, Ga, 1, 2], what
        for n in ARRAYS:
            assert np.array_equal(_bytes(bufs[n]), snap[n]), f"{what}: {n}"
        with pytest.raises(ValueError, match="bit 1"):
            log.compute()
        log.reset()
        with pytest.raises(ValueError, match="before any append"):
            log.compute()
    G.clear_cache()


# ---- 3. segmented delta-KL ------------------------------------------------------------------------------------------------------------------
def _ulp32(v):
    return float(np.spacing(np.abs(np.float32(v))))


def _check_segments(dev, lengths, att, lab):
    import dp_gsat_amd as G
    from dp_gsat_amd import explain as X
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    a, l, p = torch.from_numpy(att).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(ptr).to(dev)
    got = G.delta_kl_segments(a, l, p, max_seg_len=int(max(lengths, default=0)))
    again = G.delta_kl_segments(a, l, p, max_seg_len=int(max(lengths, default=0)))
    unbounded = G.delta_kl_segments(a, l, p)                               # the bound only sizes the grid
    assert got.shape == (len(lengths), 3) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(got.view(torch.int32), unbounded.view(torch.int32))
    got = got.cpu().numpy()
    for s, n in enumerate(lengths):
        seg = slice(ptr[s], ptr[s + 1])
        ref = xo.delta_kl_oracle(att[seg], lab[seg]) if n else np.zeros(3)
        alone = X.delta_kl_stats(a[seg], l[seg]).cpu().numpy()
        for c in range(3):
            print(f"segment {s} (n={n}) [{c}]: {got[s, c]!r} oracle {ref[c]!r} alone {alone[c]!r}")
            assert abs(float(got[s, c]) - ref[c]) <= TOL * max(1.0, abs(ref[c])), (s, n, c)
            assert abs(float(got[s, c]) - float(alone[c])) <= _ulp32(alone[c]) + 1e-9, (s, n, c)


def test_delta_kl_segments(dev):
    """Segment lengths around the wave and workgroup sizes, an empty one, one longer than the chunk a workgroup handles in a single pass
    (gsat_delta_kl_segments_chunk() = 4096 entries: 2 * 4096 + 17 takes three workgroups) and two with one class only; then S = 1 and S = 0."""
    import dp_gsat_amd as G
    from dp_gsat_amd.eval_log import delta_kl_segments_chunk
    chunk = delta_kl_segments_chunk()
    assert chunk == 4096
    lengths = [0, 1, 2, 63, 64, 65, 255, 256, 257, 2 * chunk + 17, 300, 40]
    E = sum(lengths)
    rng = np.random.RandomState(77)
    att = rng.rand(E).astype(np.float32)
    att[rng.rand(E) < 0.05] = 0.0                                          # values the clamp acts on
    att[rng.rand(E) < 0.05] = 1.0
    lab = (rng.rand(E) < 0.3).astype(np.uint8)
    ptr = np.concatenate([[0], np.cumsum(lengths)])
    lab[ptr[10]:ptr[11]] = 1                                               # only the labelled class
    lab[ptr[11]:ptr[12]] = 0                                               # only the unlabelled class
    _check_segments(dev, lengths, att, lab)
    _check_segments(dev, [E], att, lab)                                    # S = 1: the whole array, many chunks
    empty = G.delta_kl_segments(torch.from_numpy(att).to(dev), torch.from_numpy(lab).to(dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert empty.shape == (0, 3)                                           # S = 0
    none = G.delta_kl_segments(torch.zeros(0, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev),
                               torch.zeros(3, dtype=torch.int64, device=dev))
    assert none.tolist() == [[0.0, 0.0, 0.0]] * 2                          # empty segments of an empty array


# ---- 4. the log against the existing meters ---------------------------------------------------------------------------------------------------
def _symmetrised(b, seed):
    ei = b.edge_index.numpy()
    key = np.minimum(ei[0], ei[1]) * b.num_nodes + np.maximum(ei[0], ei[1])
    _, inv = np.unique(key, return_inverse=True)
    return np.random.RandomState(seed).rand(inv.max() + 1).astype(np.float32)[inv]


def test_log_equals_the_meters_on_the_same_batches(dev):
    """Three unpadded batches with symmetrised attention (every edge tied with its reverse) through EvaluationMeter and EpochLog."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    k, bins = 5, 32
    meter = G.EvaluationMeter(k, bins=bins)
    E_all = sum(synth.ba2motifs_batch(num_graphs=8, seed=20 + i).num_edges for i in range(3))
    log = G.EpochLog(k, 24, E_all, 3, 1, bins=bins, device=dev)
    oracle = lo.LogOracle(k, 24, E_all, 3, 1, bins=bins)
    for i in range(3):
        b = synth.ba2motifs_batch(num_graphs=8, seed=20 + i)
        rng = np.random.RandomState(30 + i)
        att = _symmetrised(b, 40 + i)
        lab = (rng.rand(b.num_edges) < 0.3).astype(np.uint8)
        z = rng.randn(8, 1).astype(np.float32)
        z[np.abs(z) < 1e-3] = 0.5
        b.edge_label = torch.from_numpy(lab)
        d = b.to(dev)
        a, zz = torch.from_numpy(att).view(-1, 1).to(dev), torch.from_numpy(z).to(dev)
        meter.update(a, d, zz)
        log.append(a, d, zz)
        oracle.append(att, lab, b.edge_index.numpy(), b.batch.numpy(), 8, z, b.y.numpy())
    want = meter.compute()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            got = log.compute()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    syncs = [w for w in seen if "synchroniz" in str(w.message).lower()]
    print("synchronising operations in compute():", len(syncs))
    assert len(syncs) == 2, [str(w.message) for w in seen]                    # the counts, then the packed results
    assert set(got) == set(want) | {"loss", "pred", "info"}
    for key in INT_KEYS:
        assert np.array_equal(got[key], want[key]), key
    for name, arr in want["pr_curve"].items():
        if arr.dtype == np.int64:
            assert got["pr_curve"][name].dtype == np.int64 and np.array_equal(got["pr_curve"][name], arr), name
        else:
            assert np.array_equal(got["pr_curve"][name], arr), name           # quotients of the same integers
    print("precision@k", got[f"precision@{k}"], want[f"precision@{k}"], "delta_kl", got["delta_kl"], want["delta_kl"])
    assert abs(got[f"precision@{k}"] - want[f"precision@{k}"]) <= 1e-6
    ref = oracle.compute()
    for key in ("delta_kl", "avg_signal_att_weights", "avg_bkg_att_weights"):
        assert abs(got[key] - ref[key]) <= TOL * max(1.0, abs(ref[key])), key
    for key in ("avg_signal_att_weights", "avg_bkg_att_weights"):
        assert abs(got[key] - want[key]) <= _ulp32(want[key]) + 1e-9, key
    # the mean of three per-batch values, each within one fp32 ulp of itself + 1e-9 of the meter's
    assert abs(got["delta_kl"] - want["delta_kl"]) <= np.mean([_ulp32(v) for v in oracle.delta_kl_per_batch()]) + 1e-9
    assert abs(got[f"precision@{k}"] - ref[f"precision@{k}"]) <= 1e-12 and abs(got["att_auroc"] - ref["att_auroc"]) <= 1e-12
    assert all(np.isnan(got[n]) for n in ("loss", "pred", "info"))           # no losses were given
    G.clear_cache()


# ---- 5. - 7. replayed evaluation ------------------------------------------------------------------------------------------------------------
H = 32
BATCH = 8
EVAL_IDS = [33, 5, 12, 0, 27, 39, 8, 19, 2, 30, 31, 7, 22, 14, 36, 9, 11, 3, 25, 38, 17]          # two full batches and a tail of five
TRAIN_IDS = [4, 5, 16, 20, 1, 37, 28, 10]
# Whether the eval-mode forward of a padded batch equals the unpadded one BIT FOR BIT on the real rows.  Measured on an MI355X: GIN with
# edge attention does (attention and logits of every replayed batch, before and after a training step); PNA with node attention does not
# (it agrees at TOL).  True: the integer keys of ReplayedEval.run are compared with the eager unpadded evaluation directly, and the test
# asserts the bitwise equality it relies on.  False: they are compared after feeding the hand-built log with the replay's own sliced
# outputs, and the forward is compared at TOL.  (The comparison through the replay's own outputs runs in both cases.)
# precision@k goes with the integer keys: it is the mean of integer hit counts, and an attention that moves by rounding can reorder two
# edges around rank k (in node-attention mode the lifted values of neighbouring edges lie close together).  Where the forward is not
# bitwise equal, the test therefore checks graph by graph that the replay's hits differ from the eager ones ONLY where the gap between
# the rank-k and rank-(k+1) attention is within twice the measured difference of the two forwards (_hits_differ_only_at_near_ties).
PADDED_FORWARD_IS_BITWISE = {"GIN": True, "PNA": False}


def _gsat(dev, backbone, edge, graphs, capturable=True):
    import dp_gsat_amd as G
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=0.3, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=deg)
    clf = G.get_model(14, 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(H, edge).to(dev)
    params = list(clf.parameters()) + list(ext.parameters())
    opt = torch.optim.Adam(params, lr=1e-2, weight_decay=3e-6, capturable=capturable, fused=capturable)
    return G.GSAT(clf, ext, G.Criterion(2, False), opt, learn_edge_att=edge, decay_interval=1).train()


def _eager_eval(gsat, ds, ids, epoch, dev):
    """[(unpadded batch, edge attention [E, 1], logits, losses fp32[3])] of the eval-mode forward, batch by batch."""
    import dp_gsat_amd as G
    out = []
    gsat.eval()
    try:
        with torch.no_grad():
            for s in range(0, len(ids), BATCH):
                ub = ds.collate(torch.tensor(ids[s:s + BATCH], device=dev))
                att, _, ld, logits = gsat.forward_pass(ub, epoch, False)
                losses = torch.tensor([ld["loss"], ld["pred"], ld["info"]], dtype=torch.float32, device=dev)
                out.append((ub, G.ops.edge_tensor(att).clone(), logits.clone(), losses))
    finally:
        gsat.train()
    return out


def _log_of(batches, ds, dev, k=5):
    import dp_gsat_amd as G
    log = G.EpochLog(k, ds.num_graphs, int(ds.edge_local_all.shape[1]), len(batches), 1, device=dev)
    for ub, att, logits, losses in batches:
        log.append(att, ub, logits, losses)
    return log.compute()


def _hits_differ_only_at_near_ties(ub, att, att_replay, k, what):
    """Per graph of the unpadded batch ``ub``: hits of the eager attention and of the replay's.  Changing a graph's top-k set needs an edge
    outside it to overtake one inside; with both forwards within ``delta`` of each other that takes a gap of at most 2 * delta between
    the rank-k and the rank-(k+1) value.  Returns the number of graphs whose hits differ."""
    import dp_gsat_amd as G
    args = (ub.edge_label, k, ub.batch, ub.edge_index, ub.num_graphs)
    he = np.rint(G.precision_at_k(att, *args).cpu().numpy().astype(np.float64) * k).astype(np.int64)
    hr = np.rint(G.precision_at_k(att_replay, *args).cpu().numpy().astype(np.float64) * k).astype(np.int64)
    delta = float((att.double() - att_replay.double()).abs().max())
    rk = G.rank_edges(att, ub.edge_index, ub.batch, ub.num_graphs)
    order, ptr, a = rk.order.cpu().numpy(), rk.edge_ptr.cpu().numpy(), att.reshape(-1).cpu().numpy().astype(np.float64)
    differ = 0
    for g in np.flatnonzero(he != hr):
        o = order[ptr[g]:ptr[g + 1]]
        assert len(o) > k, f"{what}: graph {g} has no edge outside its top {k}, yet hits {he[g]} != {hr[g]}"
        gap = a[o[k - 1]] - a[o[k]]
        print(f"{what}: graph {g} hits {he[g]} (eager) / {hr[g]} (replay), gap at rank {k}: {gap:.3e}, forwards differ by {delta:.3e}")
        assert 0.0 <= gap <= 2.0 * delta, f"{what}: graph {g}: hits differ without a near-tie at rank {k}"
        differ += 1
    return differ


def _compare(got, want, exact, what):
    for key in FLOAT_KEYS:
        print(f"{what} {key}: {got[key]!r} / {want[key]!r}")
        assert abs(got[key] - want[key]) <= TOL * max(1.0, abs(want[key])), f"{what}: {key}"
    print(f"{what} {HITS_KEY}: {got[HITS_KEY]!r} / {want[HITS_KEY]!r}")
    if exact:
        assert abs(got[HITS_KEY] - want[HITS_KEY]) <= 1e-12, f"{what}: {HITS_KEY}"          # the same integers, one division
        for key in INT_KEYS:
            assert np.array_equal(got[key], want[key]), f"{what}: {key}"
        for name in ("tp", "fp", "tn", "fn"):
            assert np.array_equal(got["pr_curve"][name], want["pr_curve"][name]), f"{what}: pr_curve {name}"


@pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])
def test_replayed_eval_scores_what_the_eager_evaluation_scores(dev, backbone, edge):
    """ReplayedEval.run over two full batches and a tail against an EpochLog fed by hand; again after one ReplayedStep.step: the graph
    reads the updated weights and running statistics."""
    import dp_gsat_amd as G
    graphs = _labelled_graphs(40, self_loop=(5,))
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = _gsat(dev, backbone, edge, graphs)
    graph = torch.cuda.CUDAGraph()
    try:
        graph.enable_debug_mode()
    except Exception:
        pass
    modes = [m.training for m in gsat.modules()]
    ev = G.ReplayedEval(gsat, ds, BATCH, 5, graph=graph)
    assert [m.training for m in gsat.modules()] == modes and not G.graph_index.sync_free() and gsat.sync_loss_dict
    assert ev.log.state.tolist() == [0, 0, 0, 0]
    text = None
    try:
        path = os.path.join(tempfile.mkdtemp(), "graph.dot")
        graph.debug_dump(path)
        if os.path.exists(path) and os.path.getsize(path) > 0:
            text = open(path, errors="replace").read()
    except Exception:
        text = None
    assert_no_memset_nodes(text, "ReplayedEval")
    rs = G.ReplayedStep(gsat, ds, BATCH)
    bitwise = PADDED_FORWARD_IS_BITWISE[backbone]
    first = None
    for round_, epoch in enumerate((0, 2)):
        got = ev.run(np.asarray(EVAL_IDS), epoch)
        assert ev.log.state.tolist()[1:] == [len(EVAL_IDS), 3, 0]
        eager = _eager_eval(gsat, ds, EVAL_IDS, epoch, dev)
        want = _log_of(eager, ds, dev)
        # the replay's own outputs, sliced to the real rows, through a hand-built log
        own, same, moved = [], True, 0
        for j, (ub, att, logits, losses) in enumerate(eager[:2]):
            ev.step(EVAL_IDS[j * BATCH:(j + 1) * BATCH], epoch)
            E = ub.num_edges
            assert ev.batch.valid.tolist() == [ub.num_nodes, E, BATCH, 0]
            close(ev.edge_att[:E], att, TOL, what=f"round {round_} batch {j}: edge_att")
            close(ev.clf_logits[:BATCH], logits, TOL, what=f"round {round_} batch {j}: clf_logits")
            close(ev.losses, losses, TOL, what=f"round {round_} batch {j}: losses")
            same = same and torch.equal(ev.edge_att[:E], att) and torch.equal(ev.clf_logits[:BATCH], logits)
            moved += _hits_differ_only_at_near_ties(ub, att, ev.edge_att[:E].clone(), 5, f"round {round_} batch {j}")
            own.append((ub, ev.edge_att[:E].clone(), ev.clf_logits[:BATCH].clone(), ev.losses.clone()))
        own.append(eager[2])                                               # the tail runs eagerly inside run(), too
        print(f"{backbone} round {round_}: padded eval forward bitwise equal to the unpadded one on the real rows: {same}")
        assert same or not bitwise, "the padded forward is no longer bitwise equal to the unpadded one: see PADDED_FORWARD_IS_BITWISE"
        _compare(got, _log_of(own, ds, dev), True, f"round {round_} against the replay's own outputs")
        _compare(got, want, bitwise, f"round {round_} against the eager evaluation")
        # the mean of hits / k over the graphs moves by at most 1 / graphs per near-tied graph found above, and not at all without one
        assert abs(got[HITS_KEY] - want[HITS_KEY]) <= moved / float(len(EVAL_IDS)) + 1e-12
        if first is None:
            first = got
            rs.step(TRAIN_IDS, 0)                                          # one training step in between
    assert first["loss"] != got["loss"] and first["info"] != got["info"]   # the second run scored other weights (and another r)
    G.clear_cache()


def _training_state(gsat, dev):
    opt = gsat.optimizer
    out = {"param." + n: p.detach().clone() for n, p in gsat.named_parameters()}
    out.update({"buffer." + n: b.detach().clone() for n, b in gsat.named_buffers()})
    for i, p in enumerate(p for grp in opt.param_groups for p in grp["params"]):
        for key, v in opt.state[p].items():
            if isinstance(v, torch.Tensor):
                out[f"adam.{i}.{key}"] = v.detach().clone()
    return out, seed_state(dev)


def test_evaluation_does_not_disturb_training(dev):
    """Three replayed training steps with a replayed evaluation epoch after each, and the same three steps from the same initial state and
    seed stream without any evaluation: parameters, BatchNorm buffers, Adam state and the device seed counter are bitwise equal."""
    import dp_gsat_amd as G
    graphs = _labelled_graphs(40, self_loop=(5,))
    ds = G.PackedDataset.from_data_list(graphs, dev)
    steps = [TRAIN_IDS, EVAL_IDS[:8], EVAL_IDS[8:16]]
    runs = []
    for with_eval in (True, False):
        torch.manual_seed(99)
        gsat = _gsat(dev, "GIN", True, graphs)
        rs = G.ReplayedStep(gsat, ds, BATCH)
        ev = G.ReplayedEval(gsat, ds, BATCH, 5) if with_eval else None
        pin_seed_stream(dev, 0x5EED)
        for epoch, ids in enumerate(steps):
            rs.step(ids, epoch)
            if ev is not None:
                res = ev.run(np.asarray(EVAL_IDS), epoch)
                assert np.isfinite(res["loss"]) and gsat.training
        torch.cuda.synchronize()
        runs.append(_training_state(gsat, dev))
    (a, seed_a), (b, seed_b) = runs
    assert set(a) == set(b) and any(k.startswith("adam.") for k in a) and any("running_mean" in k for k in a)
    assert seed_a == seed_b and seed_a[1] > 0                              # (base, counter): the training steps drew, the evaluations did not
    for key in a:
        assert torch.equal(a[key], b[key]), key
    G.clear_cache()


def test_replayed_eval_refusals(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd.encoders import BatchNorm1d
    graphs = _labelled_graphs(**po.LAYOUT_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    gsat = _gsat(dev, "GIN", True, graphs)
    with pytest.raises(ValueError, match="multi-label"):
        G.ReplayedEval(G.GSAT(gsat.clf, gsat.extractor, G.Criterion(2, True), None, learn_edge_att=True), ds, 5, 5)
    bns = [m for m in gsat.modules() if isinstance(m, BatchNorm1d)]
    assert bns
    bns[0].sync_group = True
    with pytest.raises(ValueError, match="sync_group"):
        G.ReplayedEval(gsat, ds, 5, 5)
    del bns[0].sync_group
    shared = {"learn_edge_att": False, "extractor_dropout_p": 0.5}
    mcfg = dict(pred_loss_coef=1, info_loss_coef=1, fix_r=False, decay_interval=10, decay_r=0.1, final_r=0.5)
    dual = G.DualGSAT(gsat.clf, G.ExtractorMLP(H, shared, "primal").to(dev), None, gsat.clf, G.ExtractorMLP(H, shared, "dual").to(dev), None,
                      mcfg, mcfg, False, False)
    with pytest.raises(ValueError, match="DualGSAT"):
        G.ReplayedEval(dual, ds, 5, 5)
    ev = G.ReplayedEval(gsat, ds, 5, 5)                                       # and the plain model is taken
    with pytest.raises(ValueError, match="captured for 5"):
        ev.step([0, 1, 2], 0)
    ev.check_epoch(list(range(ds.num_graphs)))                                # inherited: the default capacity takes any batch
    G.clear_cache()
