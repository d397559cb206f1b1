"""not gpu: public surface of dp_gsat_amd.evaluate, its error convention, and the CPU oracle the GPU tests compare against."""
import numpy as np
import pytest
import torch

from tests import evaluate_oracle as eo

NAMES = ["task_auroc_counts", "classifier_rocauc", "classifier_accuracy", "attention_histogram", "pr_curve", "EvaluationMeter",
         "AttentionHistogram"]


def test_evaluate_names_are_public():
    import dp_gsat_amd as G
    for name in NAMES:
        assert name in G.__all__ and hasattr(G, name), name


def test_evaluate_symbols_are_bound():
    import __graft_entry__ as ge
    ge.build()
    from dp_gsat_amd import _lib
    for sym in ("gsat_auroc_tasks", "gsat_auroc_tasks_workspace_bytes", "gsat_att_histogram"):
        assert sym in _lib.SIGNATURES, sym
        assert hasattr(_lib.load(), sym), sym
    assert _lib.load().gsat_auroc_tasks_workspace_bytes(7831, 12) > 7831 * 12 * (8 + 8 + 1 + 1 + 4)


def test_cpu_tensors_raise():
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import GsatHipError
    from dp_gsat_amd.synth import Batch
    logits, y = torch.randn(4, 3), torch.tensor([[1.0, 0.0, float("nan")]] * 4)
    att, lab = torch.rand(3), torch.tensor([1, 0, 1])
    with pytest.raises(GsatHipError):
        G.task_auroc_counts(logits, y)
    with pytest.raises(GsatHipError):
        G.classifier_rocauc(logits, y)
    with pytest.raises(GsatHipError):
        G.classifier_accuracy(logits, y, True)
    with pytest.raises(GsatHipError):
        G.attention_histogram(att, lab)
    with pytest.raises(GsatHipError):
        G.attention_histogram(att)
    with pytest.raises(GsatHipError):
        G.pr_curve(torch.zeros(2, 8, dtype=torch.int64))
    with pytest.raises(GsatHipError):
        G.pr_curve(G.AttentionHistogram(torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 0.0, 1.0))
    with pytest.raises(GsatHipError):
        ei = torch.tensor([[0, 1, 2], [1, 0, 0]])
        data = Batch(edge_index=ei, batch=torch.zeros(3, dtype=torch.int64), edge_label=lab, y=torch.ones(1, 1), num_graphs=1)
        G.EvaluationMeter(5).update(att, data, torch.randn(1, 1))
    with pytest.raises(ValueError):
        G.EvaluationMeter(5, bins=0)
    with pytest.raises(ValueError):
        G.EvaluationMeter(0)


def test_oracle_task_auroc_equals_sklearn_on_the_labelled_rows():
    from sklearn.metrics import roc_auc_score
    rng = np.random.RandomState(0)
    R, T = 3000, 5
    s = (np.round(rng.rand(R, T) * 100) / 100).astype(np.float32)          # quantised to 0.01: ties everywhere
    y = (rng.rand(R, T) < 0.3).astype(np.float64)
    y[rng.rand(R, T) < 0.2] = np.nan                                        # ~20 % unlabelled
    c = eo.task_counts_oracle(s, y)
    per = []
    for t in range(T):
        have = ~np.isnan(y[:, t])
        U2, P, Nn = (int(v) for v in c[t])
        assert P == int((y[have, t] != 0).sum()) and Nn == int(have.sum()) - P
        ref = roc_auc_score(y[have, t], s[have, t])
        assert abs(U2 / (2 * P * Nn) - ref) <= 1e-12
        per.append(ref)
    assert abs(eo.rocauc_oracle(s, y) - np.mean(per)) <= 1e-12
    # the ogb rule: a task with one class, or without labels, is left out of the mean; no task left -> NaN
    y2 = y.copy()
    y2[:, 1] = np.nan
    y2[~np.isnan(y2[:, 3]), 3] = 1.0
    c2 = eo.task_counts_oracle(s, y2)
    assert tuple(c2[1]) == (0, 0, 0) and c2[3, 2] == 0 and c2[3, 1] > 0
    assert abs(eo.rocauc_oracle(s, y2) - np.mean([per[0], per[2], per[4]])) <= 1e-12
    assert np.isnan(eo.rocauc_oracle(s[:, :1], np.full((R, 1), np.nan)))
    # [R] inputs are one task; a brute-force pair count agrees
    a, l = s[:400, 0], y[:400, 0]
    have = ~np.isnan(l)
    neg, pos = a[have][l[have] == 0], a[have][l[have] != 0]
    brute = sum(2 * int((neg < v).sum()) + int((neg == v).sum()) for v in pos)
    assert tuple(eo.task_counts_oracle(a, l)[0]) == (brute, len(pos), len(neg))


@pytest.mark.parametrize("bins,lo,hi", [(1, 0.0, 1.0), (7, 0.0, 1.0), (64, 0.0, 1.0), (127, 0.0, 1.0), (100, -0.25, 1.5), (4096, -0.25, 1.5)])
def test_oracle_histogram_equals_numpy_away_from_interior_edges(bins, lo, hi):
    """Values at bin centres shifted by less than a quarter bin (numpy's edge arithmetic differs from the contract's only AT interior
    edges), plus values exactly at lo and hi, plus out-of-range values and NaN."""
    rng = np.random.RandomState(bins)
    n = 5000
    centre = (rng.randint(0, bins, size=n) + 0.5 + rng.uniform(-0.25, 0.25, size=n)) / bins
    a = (lo + centre * (hi - lo)).astype(np.float32)
    a[:20], a[20:40] = np.float32(lo), np.float32(hi)
    a[40:50], a[50:60], a[60:65] = np.float32(lo - 0.5), np.float32(hi + 0.5), np.nan
    lab = (rng.rand(n) < 0.4).astype(np.int64)
    counts, outside = eo.histogram_oracle(a, lab, bins, lo, hi)
    a64 = a.astype(np.float64)
    ok = (a64 >= lo) & (a64 <= hi)
    for c in (0, 1):
        ref, _ = np.histogram(a64[ok & (lab == c)], bins=bins, range=(lo, hi))
        assert np.array_equal(counts[c], ref), c
        assert outside[c] == int((~ok & (lab == c)).sum())
    assert counts.sum() + outside.sum() == n and outside.sum() == 25
    c0, o0 = eo.histogram_oracle(a, None, bins, lo, hi)
    assert np.array_equal(c0[0], counts.sum(0)) and c0[1].sum() == 0 and o0.tolist() == [25, 0]


def test_oracle_pr_curve_and_accuracy():
    counts = np.array([[5, 0, 2, 1], [0, 1, 3, 4]])
    pr = eo.pr_curve_oracle(counts)
    assert pr["tp"].tolist() == [8, 8, 7, 4] and pr["fp"].tolist() == [8, 3, 3, 1]
    assert pr["fn"].tolist() == [0, 0, 1, 4] and pr["tn"].tolist() == [0, 5, 5, 7]
    assert np.allclose(pr["precision"], [0.5, 8 / 11, 0.7, 0.8]) and np.allclose(pr["recall"], [1.0, 1.0, 7 / 8, 0.5])
    zero = eo.pr_curve_oracle(np.zeros((2, 3), dtype=np.int64))
    assert zero["precision"].tolist() == [0.0] * 3 and zero["recall"].tolist() == [0.0] * 3
    z = np.array([[2.0, -1.0], [-3.0, 0.5], [1.0, 1.0]], dtype=np.float32)
    y = np.array([[1.0, np.nan], [0.0, 0.0], [0.0, 1.0]])
    assert eo.accuracy_oracle(z, y, True) == 3 / 6                          # NaN never matches
    assert eo.accuracy_oracle(z[:, :1], y[:, :1], False) == 2 / 3
    assert eo.accuracy_oracle(z, np.array([0, 1, 1]), False) == 2 / 3       # argmax head; a tie takes the first column
