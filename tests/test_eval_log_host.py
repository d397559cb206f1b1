"""not gpu: the epoch-log oracle against the existing oracles on the concatenation, and the declarations of the new entry points."""
import os
import re

import numpy as np
import pytest

from tests import eval_log_oracle as lo
from tests import evaluate_oracle as eo
from tests import explain_oracle as xo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsat_eval_log_append", "gsat_delta_kl_segments", "gsat_delta_kl_segments_workspace_bytes", "gsat_delta_kl_segments_chunk")


def _batches():
    """Four batches with interleaved edge ids; quantised attention, so ties are common; one batch has a graph without edges."""
    out = []
    for i, counts in enumerate(([7, 0, 12, 3], [1], [64, 65, 2, 9, 30], [5, 5])):
        b = xo.custom_batch(counts, seed=10 + i)
        rng = np.random.RandomState(20 + i)
        E = b.edge_index.shape[1]
        att = (np.round(rng.rand(E) * 20) / 20).astype(np.float32)
        lab = (rng.rand(E) < 0.3).astype(np.uint8)
        z = rng.randn(len(counts), 1).astype(np.float32)
        y = (rng.rand(len(counts), 1) < 0.5).astype(np.float32)
        out.append((b, att, lab, z, y, rng.rand(3).astype(np.float32)))
    return out


def test_log_oracle_equals_the_existing_oracles_on_the_concatenation():
    k, bins = 5, 32
    batches = _batches()
    G = sum(b.num_graphs for b, *_ in batches)
    E = sum(b.edge_index.shape[1] for b, *_ in batches)
    log = lo.LogOracle(k, G + 3, E + 11, len(batches) + 2, 1, 1, bins)
    hits, dkl, atts, labs, seen_e, seen_g = [], [], [], [], 0, 0
    for n, (b, att, lab, z, y, losses) in enumerate(batches):
        ei, bt = b.edge_index.numpy(), b.batch.numpy()
        log.append(att, lab, ei, bt, b.num_graphs, z, y, losses)
        order, _, _, h, ptr = xo.rank_oracle(att, ei, bt, b.num_graphs, k, lab)
        grouped = np.argsort(bt[ei[0]], kind="stable")
        # the layout: the batch's edges graph by graph, ascending edge id inside a graph; pointers shifted by the running offset
        assert np.array_equal(log.att[seen_e:seen_e + len(att)], att[grouped]) and np.array_equal(log.label[seen_e:seen_e + len(att)], lab[grouped])
        assert np.array_equal(log.graph_edge_ptr[seen_g:seen_g + b.num_graphs + 1], seen_e + ptr)
        assert all(np.array_equal(np.sort(order[ptr[g]:ptr[g + 1]]), grouped[ptr[g]:ptr[g + 1]]) for g in range(b.num_graphs))
        seen_e, seen_g = seen_e + len(att), seen_g + b.num_graphs
        assert log.state.tolist() == [seen_e, seen_g, n + 1, 0] and log.batch_edge_ptr[n + 1] == seen_e
        hits.append(h); dkl.append(xo.delta_kl_oracle(att, lab)[0]); atts.append(att); labs.append(lab)
    att, lab = np.concatenate(atts), np.concatenate(labs)
    # beyond the prefix: the sentinel
    assert (log.label[seen_e:] == lo.LogOracle.SENTINEL).all() and (log.att[seen_e:].view(np.uint8) == lo.LogOracle.SENTINEL).all()
    assert (log.graph_edge_ptr[seen_g + 1:].view(np.uint8) == lo.LogOracle.SENTINEL).all()
    assert np.array_equal(log.hits(), np.concatenate(hits))                               # per-graph hits, integers
    assert log.auroc_counts() == xo.auroc_counts_oracle(att, lab)                         # (U2, P, Nn), integers
    counts, outside = eo.histogram_oracle(att, lab, bins, 0.0, 1.0)
    got = log.histogram()
    assert np.array_equal(got[0], counts) and np.array_equal(got[1], outside)
    assert abs(log.delta_kl_per_batch().mean() - np.mean(dkl)) <= 1e-12
    res = log.compute()
    assert abs(res["precision@5"] - np.concatenate(hits).mean() / k) <= 1e-15
    want = np.stack([l for *_, l in batches]).astype(np.float64).sum(0) / len(batches)
    assert np.allclose([res["loss"], res["pred"], res["info"]], want, rtol=0, atol=1e-15)
    assert res["clf_acc"] == eo.accuracy_oracle(np.concatenate([z for _, _, _, z, _, _ in batches]), np.concatenate([y for *_, y, _ in batches]), False)


def test_log_oracle_flags_and_padded_counts():
    b, att, lab, z, y, _ = _batches()[0]
    ei, bt = b.edge_index.numpy(), b.batch.numpy()
    E, G = ei.shape[1], b.num_graphs
    for caps, bit in (((G, E - 1, 1), 2), ((G - 1, E, 1), 2), ((G, E, 0), 2)):
        log = lo.LogOracle(5, caps[0], caps[1], caps[2], 1)
        before = {n: a.copy() for n, a in log.arrays().items()}
        log.append(att, lab, ei, bt, G, z, y)
        assert log.state.tolist() == [0, 0, 0, bit]
        assert all(np.array_equal(a.view(np.uint8), before[n].view(np.uint8)) for n, a in log.arrays().items())
    log = lo.LogOracle(5, G, E, 1, 1)
    log.append(att, lab, ei, bt, G, z, y, overflow=True)
    assert log.state.tolist() == [0, 0, 0, 1]
    # a padded batch logs its first real_graphs graphs and their edges only; no losses: the sums turn NaN
    log.append(att, lab, ei, bt, G, z, y, real_graphs=G - 1)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(bt[ei[0]], minlength=G))])
    assert log.state.tolist() == [ptr[G - 1], G - 1, 1, 1] and np.isnan(log.loss_sums).all()


def test_header_and_signatures_list_the_new_entry_points():
    from dp_gsat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsat_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gsat_[a-z0-9_]+)\s*\(", txt))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/gsat_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
    assert re.search(r"#define\s+GSAT_ABI_VERSION\s+4\b", txt)
    res, args = _lib.SIGNATURES["gsat_eval_log_append"]
    assert res is _lib.INT and args[-1] is _lib.P and len(args) == 24          # an int status, the stream last
    res, args = _lib.SIGNATURES["gsat_delta_kl_segments"]
    assert res is _lib.INT and args[-1] is _lib.P
    import dp_gsat_amd as G
    assert G.EpochLog.__module__ == "dp_gsat_amd.eval_log" and G.ReplayedEval.__module__ == "dp_gsat_amd.replay"


def test_epoch_log_rejects_capacities_beyond_int32():
    import dp_gsat_amd as G
    with pytest.raises(ValueError, match="2\\*\\*31"):
        G.EpochLog(5, 10, 2 ** 31, 1, 1)
    with pytest.raises(ValueError, match="k must be positive"):
        G.EpochLog(0, 10, 10, 1, 1)
