"""not gpu: public surface of dp_gsat_amd.explain, its error convention, and the CPU oracle the GPU tests compare against."""
import numpy as np
import pytest
import torch

from tests import explain_oracle as xo

NAMES = ["rank_edges", "topk_edge_mask", "precision_at_k", "attention_auroc", "delta_kl", "ExplanationMeter", "EdgeRanking"]


def test_explain_names_are_public():
    import dp_gsat_amd as G
    for name in NAMES:
        assert name in G.__all__ and hasattr(G, name), name


def test_explain_symbols_are_bound():
    from dp_gsat_amd import _lib
    for sym in ("gsat_rank_edges", "gsat_rank_edges_lds_cap", "gsat_rank_edges_workspace_bytes", "gsat_auroc", "gsat_auroc_workspace_bytes",
                "gsat_delta_kl", "gsat_delta_kl_workspace_bytes"):
        assert sym in _lib.SIGNATURES, sym


def test_cpu_tensors_raise():
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import GsatHipError
    ei = torch.tensor([[0, 1, 2], [1, 0, 0]])
    batch = torch.zeros(3, dtype=torch.int64)
    att, lab = torch.rand(3), torch.tensor([1, 0, 1])
    with pytest.raises(GsatHipError):
        G.rank_edges(att, ei, batch, 1)
    with pytest.raises(GsatHipError):
        G.topk_edge_mask(att, ei, batch, k=1, num_graphs=1)
    with pytest.raises(GsatHipError):
        G.precision_at_k(att, lab, 2, batch, ei)
    with pytest.raises(GsatHipError):
        G.attention_auroc(att, lab)
    with pytest.raises(GsatHipError):
        G.delta_kl(att, lab)
    with pytest.raises(GsatHipError):
        from dp_gsat_amd.synth import Batch
        G.ExplanationMeter(5).update(att, Batch(edge_index=ei, batch=batch, edge_label=lab, num_graphs=1))


def test_midrank_auroc_equals_sklearn_on_tied_data():
    from sklearn.metrics import roc_auc_score
    rng = np.random.RandomState(0)
    a = (np.round(rng.rand(5000) * 100) / 100).astype(np.float32)          # quantised to 0.01: ties everywhere
    y = (rng.rand(5000) < 0.3).astype(np.int64)
    assert abs(xo.auroc_oracle(a, y) - roc_auc_score(y, a)) <= 1e-12
    U2, P, Nn = xo.auroc_counts_oracle(a, y)
    brute = sum(2 * int((a[~y.astype(bool)] < v).sum()) + int((a[~y.astype(bool)] == v).sum()) for v in a[y.astype(bool)])
    assert U2 == brute and P == int(y.sum()) and Nn == 5000 - P
    assert xo.auroc_oracle(a, np.ones_like(y)) == 0.0


def test_rank_oracle_is_the_stable_order():
    b = xo.custom_batch([3, 0, 4], seed=1)
    att = np.array([0.5, 0.5, -0.0, 0.0, 0.5, 0.25, 0.25], dtype=np.float32)
    lab = np.array([1, 0, 1, 0, 0, 1, 1])
    order, rank, topk, hits, ptr = xo.rank_oracle(att, b.edge_index.numpy(), b.batch.numpy(), 3, 2, lab)
    eg = b.batch.numpy()[b.edge_index.numpy()[0]]
    for g in range(3):
        o = order[ptr[g]:ptr[g + 1]]
        assert sorted(o.tolist()) == np.flatnonzero(eg == g).tolist()
        keys = [(-float(att[e]) + 0.0, int(e)) for e in o]
        assert keys == sorted(keys)                                         # descending attention, ties by ascending edge id
        assert hits[g] == int(lab[o[:2]].sum())
    assert np.array_equal(rank[order], np.concatenate([np.arange(ptr[g + 1] - ptr[g]) for g in range(3)]))
    assert np.array_equal(topk, (rank < 2).astype(np.uint8))
    prec = xo.precision_at_k_reference_loop(att, lab, 2, b.batch.numpy(), b.edge_index.numpy())
    assert np.array_equal(prec, hits.astype(np.float32) / np.float32(2))
