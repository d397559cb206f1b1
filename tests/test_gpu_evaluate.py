"""gpu: dp_gsat_amd.evaluate against the CPU oracle of tests/evaluate_oracle.py -- per-task AUROC counts and attention histograms
bit-exact at the sizes the kernels branch on, the ogb mean, accuracies, the PR curve, the epoch meter, capture."""
import math

import numpy as np
import pytest
import torch

from tests import evaluate_oracle as eo
from tests import explain_oracle as xo
from tests.util import assert_no_memset_nodes, capture_with_dump

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 2, 63, 64, 65, 257, 5000]
TASKS = [1, 2, 12, 27]


def _task_data(R, T, seed, special=True):
    """Scores on a 0.01 grid in [-0.5, 0.5] (ties everywhere) with -0.0 and +0.0 both present, ~30 % positives, ~20 % NaN labels.
    With ``special`` and enough tasks: task 1 all NaN, task 2 one class only, task 3 constant score."""
    rng = np.random.RandomState(seed)
    s = (np.round(rng.rand(R, T) * 100) / 100 - 0.5).astype(np.float32)
    zero = s == 0
    s[zero & (rng.rand(R, T) < 0.5)] = np.float32(-0.0)
    if R >= 2:
        s[0, 0], s[1, 0] = np.float32(-0.0), np.float32(0.0)
    y = (rng.rand(R, T) < 0.3).astype(np.float32)
    y[rng.rand(R, T) < 0.2] = np.nan
    if special:
        if T > 1:
            y[:, 1] = np.nan
        if T > 2:
            y[~np.isnan(y[:, 2]), 2] = 1.0
        if T > 3:
            s[:, 3] = np.float32(0.25)
    return s, y


@pytest.fixture(scope="module")
def task_cases():
    """(scores, labels, oracle counts) per (R, T): computed once, shared, never modified."""
    cases = {}
    for R in ROWS:
        for T in TASKS:
            s, y = _task_data(R, T, seed=1000 * T + R)
            cases[R, T] = (s, y, eo.task_counts_oracle(s, y))
    return cases


@pytest.mark.parametrize("T", TASKS)
@pytest.mark.parametrize("R", ROWS)
def test_task_auroc_counts_equal_the_oracle(dev, task_cases, R, T):
    import dp_gsat_amd as G
    s, y, ref = task_cases[R, T]
    sd, yd = torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)
    got = G.task_auroc_counts(sd, yd)
    assert got.dtype == torch.int64 and tuple(got.shape) == (T, 3) and got.is_cuda
    got = got.cpu().numpy()
    print(f"R={R} T={T} counts {got.tolist()[:4]}")
    assert np.array_equal(got, ref), (R, T)
    if T > 1:
        assert tuple(got[1]) == (0, 0, 0)                                   # the all-NaN task
    if T > 2:
        assert got[2, 2] == 0 and got[2, 0] == 0                            # one class only: counted, not scorable
    if T > 3:
        assert got[3, 0] == got[3, 1] * got[3, 2]                           # constant score: every pair is a tie, AUROC 1/2
    auc = G.classifier_rocauc(sd, yd)
    assert auc.dtype == torch.float64 and auc.dim() == 0 and auc.is_cuda
    want = eo.rocauc_oracle(s, y)
    print(f"R={R} T={T} rocauc {auc.item()!r} oracle {want!r}")
    if math.isnan(want):
        assert math.isnan(auc.item())
    else:
        # one fp64 division per task and a mean of <= 27 terms on either side: 1e-12 is orders above their rounding and four orders
        # below 1 / (2 * 5000^2) = 2e-8, the smallest change one miscounted pair can cause at these sizes
        assert abs(auc.item() - want) <= 1e-12
    assert torch.equal(G.task_auroc_counts(sd, yd), torch.from_numpy(ref).to(dev))          # second call: same integers


def test_every_task_unlabelled_gives_nan_and_vectors_are_one_task(dev):
    import dp_gsat_amd as G
    s, y = _task_data(257, 12, seed=5, special=False)
    nan = np.full_like(y, np.nan)
    res = G.classifier_rocauc(torch.from_numpy(s).to(dev), torch.from_numpy(nan).to(dev))
    assert math.isnan(res.item())
    assert not G.task_auroc_counts(torch.from_numpy(s).to(dev), torch.from_numpy(nan).to(dev)).any().item()
    # one class everywhere: nothing scorable either
    ones = np.ones_like(y)
    assert math.isnan(G.classifier_rocauc(torch.from_numpy(s).to(dev), torch.from_numpy(ones).to(dev)).item())
    for R in (0, 1, 65, 5000):
        s1, y1 = _task_data(R, 1, seed=40 + R)
        a = G.task_auroc_counts(torch.from_numpy(s1[:, 0].copy()).to(dev), torch.from_numpy(y1[:, 0].copy()).to(dev))
        b = G.task_auroc_counts(torch.from_numpy(s1).to(dev), torch.from_numpy(y1).to(dev))
        assert tuple(a.shape) == (1, 3) and torch.equal(a, b)
        assert np.array_equal(a.cpu().numpy(), eo.task_counts_oracle(s1, y1))
    assert tuple(G.task_auroc_counts(torch.zeros((5, 0), device=dev), torch.zeros((5, 0), device=dev)).shape) == (0, 3)
    with pytest.raises(ValueError):
        G.task_auroc_counts(torch.zeros((5, 2), device=dev), torch.zeros((5, 3), device=dev))
    with pytest.raises(ValueError):
        G.task_auroc_counts(torch.zeros((5, 2, 1), device=dev), torch.zeros((5, 2, 1), device=dev))
    # integer and bool labels are accepted (no NaN possible)
    yi = (np.random.RandomState(3).rand(257, 12) < 0.4)
    ref = eo.task_counts_oracle(s, yi.astype(np.float64))
    for t in (torch.from_numpy(yi), torch.from_numpy(yi.astype(np.int64))):
        assert np.array_equal(G.task_auroc_counts(torch.from_numpy(s).to(dev), t.to(dev)).cpu().numpy(), ref)


@pytest.mark.parametrize("R", [1, 2, 64, 65, 257, 5000])
def test_one_task_without_nan_equals_attention_auroc_counts(dev, R):
    """The one consistency check between two of the package's own kernels; both are also compared with their oracles."""
    import dp_gsat_amd as G
    from dp_gsat_amd import explain as X
    s, _ = _task_data(R, 1, seed=70 + R)
    lab = (np.random.RandomState(R).rand(R) < 0.3).astype(np.uint8)
    sd, ld = torch.from_numpy(s[:, 0].copy()).to(dev), torch.from_numpy(lab).to(dev)
    mine = G.task_auroc_counts(sd, ld.float())
    assert torch.equal(mine[0], X.attention_auroc_counts(sd, ld))
    assert tuple(mine[0].tolist()) == xo.auroc_counts_oracle(s[:, 0], lab)


# ---- histogram -------------------------------------------------------------------------------------------------------------------------
EDGES = [0, 1, 63, 64, 65, 1000, 100003]
BINS = [1, 2, 127, 256, 4096]
RANGES = [(0.0, 1.0), (-0.25, 1.5)]


def _hist_input(E, B, lo, hi, seed):
    """fp32 attention with, besides uniform values a little wider than [lo, hi] and values piled into three bins (the sigmoid's
    shape): the ends lo and hi, the nearest fp32 outside either end, interior edges lo + j (hi - lo) / B, -0.0 and NaN."""
    rng = np.random.RandomState(seed)
    w = hi - lo
    a = (lo - 0.05 * w + rng.rand(E) * 1.1 * w).astype(np.float32)
    pile = rng.rand(E) < 0.5
    a[pile] = (lo + w * rng.choice([0.031, 0.5, 0.97], size=int(pile.sum())) + rng.rand(int(pile.sum())) * 1e-4 * w).astype(np.float32)
    f = np.float32
    special = [f(lo), f(hi), np.nextafter(f(lo), f(-np.inf)), np.nextafter(f(hi), f(np.inf)), f(-0.0), f(0.0), f(np.nan)]
    special += [f(lo + j * w / B) for j in sorted({1, B // 2, B - 1}) if 0 < j < B]          # exact in fp32 for power-of-two B
    if E >= 4 * len(special):
        pos = rng.permutation(E)[:4 * len(special)]
        a[pos] = np.tile(np.array(special, dtype=np.float32), 4)
    elif E:
        a[0] = special[(seed + B) % len(special)]
    return a


@pytest.fixture(scope="module")
def hist_cases():
    cases = {}
    for E in EDGES:
        for B in BINS:
            for r, (lo, hi) in enumerate(RANGES):
                a = _hist_input(E, B, lo, hi, seed=E + 7 * B + r)
                lab = (np.random.RandomState(E + B + r).rand(E) < 0.35).astype(np.uint8)
                cases[E, B, r] = (a, lab, eo.histogram_oracle(a, lab, B, lo, hi))
    return cases


@pytest.mark.parametrize("r", [0, 1])
@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("E", EDGES)
def test_histogram_counts_equal_the_oracle(dev, hist_cases, E, B, r):
    import dp_gsat_amd as G
    lo, hi = RANGES[r]
    a, lab, (counts, outside) = hist_cases[E, B, r]
    h = G.attention_histogram(torch.from_numpy(a).to(dev), torch.from_numpy(lab).to(dev), bins=B, range=(lo, hi))
    assert isinstance(h, G.AttentionHistogram) and (h.lo, h.hi) == (lo, hi)
    assert h.counts.dtype == torch.int64 and tuple(h.counts.shape) == (2, B) and tuple(h.outside.shape) == (2,)
    print(f"E={E} B={B} range=({lo},{hi}) binned {int(h.counts.sum())} outside {h.outside.tolist()}")
    assert np.array_equal(h.counts.cpu().numpy(), counts), (E, B, r)
    assert np.array_equal(h.outside.cpu().numpy(), outside), (E, B, r)
    assert int(h.counts.sum()) + int(h.outside.sum()) == E


def test_histogram_of_one_value_everywhere(dev):
    """100003 equal values: every lane of every wavefront wants the same counter (the contention case).  Counts only."""
    import dp_gsat_amd as G
    E = 100003
    lab = (np.arange(E) % 3 == 0).astype(np.uint8)
    for value, B in ((0.7310586, 64), (1.0, 4096), (2.0, 1)):
        a = np.full(E, value, dtype=np.float32)
        counts, outside = eo.histogram_oracle(a, lab, B, 0.0, 1.0)
        h = G.attention_histogram(torch.from_numpy(a).to(dev), torch.from_numpy(lab).to(dev), bins=B)
        assert np.array_equal(h.counts.cpu().numpy(), counts) and np.array_equal(h.outside.cpu().numpy(), outside)
        assert int((h.counts != 0).sum()) + int((h.outside != 0).sum()) == 2


def test_histogram_label_kinds_and_accumulation(dev):
    import dp_gsat_amd as G
    E, B = 1000, 127
    a0, a1 = _hist_input(E, B, 0.0, 1.0, seed=1), _hist_input(E + 65, B, 0.0, 1.0, seed=2)
    l0, l1 = (np.random.RandomState(s).rand(n) < 0.35 for s, n in ((3, E), (4, E + 65)))
    ref = eo.histogram_oracle(a0, l0, B, 0.0, 1.0)
    ad = torch.from_numpy(a0).to(dev)
    for lab in (torch.from_numpy(l0), torch.from_numpy(l0.astype(np.uint8) * 7), torch.from_numpy(l0.astype(np.int64) * -3),
                torch.from_numpy(l0.astype(np.float32))):
        h = G.attention_histogram(ad, lab.to(dev), bins=B)
        assert np.array_equal(h.counts.cpu().numpy(), ref[0]) and np.array_equal(h.outside.cpu().numpy(), ref[1]), lab.dtype
    none = G.attention_histogram(ad.view(-1, 1), None, bins=B)              # [E, 1] input, no labels: everything is background
    c0, o0 = eo.histogram_oracle(a0, None, B, 0.0, 1.0)
    assert np.array_equal(none.counts.cpu().numpy(), c0) and np.array_equal(none.outside.cpu().numpy(), o0)
    assert int(none.counts[1].sum()) == 0 and int(none.outside[1]) == 0
    # two updates into one `out` = the oracle on the concatenation
    out = G.attention_histogram(ad, torch.from_numpy(l0).to(dev), bins=B)
    again = G.attention_histogram(torch.from_numpy(a1).to(dev), torch.from_numpy(l1).to(dev), out=out)
    assert again is out
    both = eo.histogram_oracle(np.concatenate([a0, a1]), np.concatenate([l0, l1]), B, 0.0, 1.0)
    assert np.array_equal(out.counts.cpu().numpy(), both[0]) and np.array_equal(out.outside.cpu().numpy(), both[1])
    empty = G.attention_histogram(torch.zeros(0, device=dev), None, out=out)               # E = 0 adds nothing
    assert np.array_equal(empty.counts.cpu().numpy(), both[0])
    for bad in (dict(bins=0), dict(bins=4097), dict(range=(1.0, 1.0)), dict(range=(1.0, 0.0))):
        with pytest.raises(ValueError):
            G.attention_histogram(ad, None, **bad)
    with pytest.raises(ValueError):
        G.attention_histogram(ad, torch.zeros(E + 1, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        G.attention_histogram(ad, None, out=G.AttentionHistogram(torch.zeros((2, B), dtype=torch.int32, device=dev),
                                                                 torch.zeros(2, dtype=torch.int64, device=dev), 0.0, 1.0))


def test_pr_curve_equals_the_oracle(dev):
    import dp_gsat_amd as G
    rng = np.random.RandomState(0)
    a = rng.beta(0.5, 0.5, size=5000).astype(np.float32)
    lab = rng.rand(5000) < (0.1 + 0.8 * a)
    for B in (1, 2, 127):
        h = G.attention_histogram(torch.from_numpy(a).to(dev), torch.from_numpy(lab).to(dev), bins=B)
        ref = eo.pr_curve_oracle(eo.histogram_oracle(a, lab, B, 0.0, 1.0)[0])
        for got in (G.pr_curve(h), G.pr_curve(h.counts)):
            assert set(got) == set(ref)
            for name in ("tp", "fp", "tn", "fn"):
                assert got[name].dtype == torch.int64 and got[name].is_cuda and np.array_equal(got[name].cpu().numpy(), ref[name]), (B, name)
            for name in ("precision", "recall"):                            # one correctly rounded fp64 division on either side
                assert got[name].dtype == torch.float64 and np.array_equal(got[name].cpu().numpy(), ref[name]), (B, name)
    zero = G.pr_curve(torch.zeros((2, 4), dtype=torch.int64, device=dev))
    assert not zero["precision"].any().item() and not zero["recall"].any().item()
    with pytest.raises(ValueError):
        G.pr_curve(torch.zeros((3, 4), dtype=torch.int64, device=dev))


def _logits(shape, seed):
    """Random logits kept away from 0, where the fp32 sigmoid of get_preds rounds to 0.5."""
    z = np.random.RandomState(seed).randn(*shape).astype(np.float32)
    z[np.abs(z) < 1e-3] = np.float32(0.5)
    return z


def test_classifier_accuracy_equals_the_oracle(dev):
    import dp_gsat_amd as G
    R = 257
    z, (_, y) = _logits((R, 12), 1), _task_data(R, 12, seed=2)
    got = G.classifier_accuracy(torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev), multi_label=True)
    assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
    assert got.item() == eo.accuracy_oracle(z, y, True)
    assert np.isnan(y).any() and got.item() < 1.0
    y1 = (np.random.RandomState(3).rand(R, 1) < 0.5).astype(np.float32)
    assert G.classifier_accuracy(torch.from_numpy(z[:, :1].copy()).to(dev), torch.from_numpy(y1).to(dev), False).item() == \
        eo.accuracy_oracle(z[:, :1], y1, False)
    y3 = np.random.RandomState(4).randint(0, 3, size=R)
    assert G.classifier_accuracy(torch.from_numpy(z[:, :3].copy()).to(dev), torch.from_numpy(y3).to(dev), False).item() == \
        eo.accuracy_oracle(z[:, :3], y3, False)
    with pytest.raises(ValueError):
        G.classifier_accuracy(torch.from_numpy(z).to(dev), torch.from_numpy(y1).to(dev), True)


# ---- meter --------------------------------------------------------------------------------------------------------------------------------
def test_meter_over_three_batches_equals_the_oracle_on_the_concatenation(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    k, bins = 5, 32
    meter, inner = G.EvaluationMeter(k, bins=bins), G.ExplanationMeter(k)
    atts, labs, zs, ys = [], [], [], []
    for i in range(3):
        b = synth.ba2motifs_batch(num_graphs=8, seed=20 + i)
        rng = np.random.RandomState(30 + i)
        att = (np.round(rng.rand(b.num_edges) * 100) / 100).astype(np.float32)
        lab = (rng.rand(b.num_edges) < 0.3).astype(np.uint8)
        z = _logits((8, 1), 40 + i)
        b.edge_label = torch.from_numpy(lab)
        d = b.to(dev)
        meter.update(torch.from_numpy(att).view(-1, 1).to(dev), d, torch.from_numpy(z).to(dev))
        inner.update(torch.from_numpy(att).to(dev), d)
        atts.append(att); labs.append(lab); zs.append(z); ys.append(b.y.numpy())
    res, plain = meter.compute(), inner.compute()
    att, lab, z, y = (np.concatenate(v) for v in (atts, labs, zs, ys))
    for key, val in plain.items():                                          # the inner keys: a plain ExplanationMeter on the same batches
        assert res[key] == val, key
    assert abs(res["att_auroc"] - xo.auroc_oracle(att, lab)) <= 1e-12
    assert set(res) == set(plain) | {"clf_acc", "clf_roc", "bkg_att_hist", "signal_att_hist", "att_outside", "pr_curve"}
    assert res["clf_acc"] == eo.accuracy_oracle(z, y, False)
    assert abs(res["clf_roc"] - eo.rocauc_oracle(z, y)) <= 1e-12
    counts, outside = eo.histogram_oracle(att, lab, bins, 0.0, 1.0)
    for key, want in (("bkg_att_hist", counts[0]), ("signal_att_hist", counts[1]), ("att_outside", outside)):
        assert isinstance(res[key], np.ndarray) and res[key].dtype == np.int64 and np.array_equal(res[key], want), key
    ref = eo.pr_curve_oracle(counts)
    assert set(res["pr_curve"]) == set(ref)
    for name, want in ref.items():
        assert res["pr_curve"][name].dtype == want.dtype and np.array_equal(res["pr_curve"][name], want), name
    with pytest.raises(ValueError):
        G.EvaluationMeter(k).compute()


def test_multi_label_meter(dev):
    """12 tasks with NaN labels through the meter: the multi-label accuracy and the ogb mean."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    meter = G.EvaluationMeter(5, bins=16, multi_label=True)
    zs, ys = [], []
    for i in range(2):
        b = synth.ba2motifs_batch(num_graphs=8, seed=50 + i)
        b.edge_label = torch.from_numpy((np.arange(b.num_edges) % 4 == 0).astype(np.uint8))
        z, (_, y) = _logits((8, 12), 60 + i), _task_data(8, 12, seed=70 + i, special=False)
        b.y = torch.from_numpy(y)
        meter.update(torch.rand(b.num_edges, device=dev), b.to(dev), torch.from_numpy(z).to(dev))
        zs.append(z); ys.append(y)
    res = meter.compute()
    z, y = np.concatenate(zs), np.concatenate(ys)
    assert res["clf_acc"] == eo.accuracy_oracle(z, y, True)
    want = eo.rocauc_oracle(z, y)
    assert not math.isnan(want) and abs(res["clf_roc"] - want) <= 1e-12


# ---- capture ------------------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_on_refilled_inputs(dev):
    """attention_histogram(out=...) then task_auroc_counts captured into one graph on one stream; two replays on refilled static
    inputs equal the oracle for each fill (the histogram accumulates over the replays, as an epoch's does)."""
    import dp_gsat_amd as G
    E, B, R, T = 1000, 127, 257, 12
    fills = [(_hist_input(E, B, 0.0, 1.0, seed=80 + i), (np.random.RandomState(90 + i).rand(E) < 0.35).astype(np.uint8),
              *_task_data(R, T, seed=100 + i)) for i in range(3)]
    a, l = torch.from_numpy(fills[0][0]).to(dev), torch.from_numpy(fills[0][1]).to(dev)
    s, y = torch.from_numpy(fills[0][2]).to(dev), torch.from_numpy(fills[0][3]).to(dev)
    hist = G.attention_histogram(a[:0], None, bins=B)                       # zeros
    out = {}

    def step():
        G.attention_histogram(a, l, out=hist)
        out["counts"] = G.task_auroc_counts(s, y)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    hist.counts.zero_(); hist.outside.zero_()
    graph, dot = capture_with_dump(step)
    assert_no_memset_nodes(dot, "evaluate")
    torch.cuda.synchronize()
    assert int(hist.counts.sum()) == 0                                      # capturing ran nothing
    seen_a, seen_l = [], []
    for fill in fills[1:]:
        for dst, src in zip((a, l, s, y), fill):
            dst.copy_(torch.from_numpy(src).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        seen_a.append(fill[0]); seen_l.append(fill[1])
        assert np.array_equal(out["counts"].cpu().numpy(), eo.task_counts_oracle(fill[2], fill[3]))
        counts, outside = eo.histogram_oracle(np.concatenate(seen_a), np.concatenate(seen_l), B, 0.0, 1.0)
        assert np.array_equal(hist.counts.cpu().numpy(), counts) and np.array_equal(hist.outside.cpu().numpy(), outside)
