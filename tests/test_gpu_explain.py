"""gpu: dp_gsat_amd.explain against the CPU oracle of tests/explain_oracle.py -- ranking bit-exact under the tie rule, both kernel
paths, precision@k against the restated reference loop, integer AUROC, delta-KL, repeatability, capture, end to end."""
import os

import numpy as np
import pytest
import torch

from tests import explain_oracle as xo
from tests.util import TOL, assert_no_memset_nodes, capture_with_dump, close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 5, 64, 100)


def _labels(E, seed, p=0.25):
    return (np.random.RandomState(seed).rand(E) < p).astype(np.int64)


def _att(E, seed, kind="random"):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.rand(E).astype(np.float32)
    if kind == "quantised":                                   # multiples of 1/16: mass ties
        return (rng.randint(0, 17, size=E) / 16.0).astype(np.float32)
    if kind == "constant":
        return np.full(E, 0.5, dtype=np.float32)
    if kind == "signed":                                      # negative values and both zeros
        a = (rng.randint(-4, 5, size=E) / 4.0).astype(np.float32)
        a[rng.rand(E) < 0.2] = -0.0
        return a
    raise ValueError(kind)


def _symmetrised(b, seed):
    """One value per undirected edge: every edge is tied with its reverse (edge-attention mode after the symmetrised mask)."""
    ei = b.edge_index.numpy()
    N = b.num_nodes
    key = np.minimum(ei[0], ei[1]) * N + np.maximum(ei[0], ei[1])
    _, inv = np.unique(key, return_inverse=True)
    return np.random.RandomState(seed).rand(inv.max() + 1).astype(np.float32)[inv]


def _check_ranking(dev, b, att, lab, ks=KS, paths=("auto", "general"), expect_general=False):
    """order / rank / topk / hits of every path in `paths` equal the oracle exactly (and therefore each other)."""
    import dp_gsat_amd as G
    from dp_gsat_amd import explain as X
    G.clear_cache()
    ei_np, batch_np, Gn = b.edge_index.numpy(), b.batch.numpy(), b.num_graphs
    d = b.to(dev)
    a, l = torch.from_numpy(att).to(dev), torch.from_numpy(lab).to(dev)
    seg = G.get_index(d.edge_index, d.num_nodes).graphs(d.batch, Gn)
    fits = 0 <= seg.max_edges_per_graph <= X.rank_edges_lds_cap()
    assert fits != expect_general
    for k in ks:
        order, rank, topk, hits, ptr = xo.rank_oracle(att, ei_np, batch_np, Gn, k, lab)
        for path in paths:
            if path == "fused" and not fits:
                continue
            out, _ = X._rank(a, d.edge_index, d.batch, Gn, path, k=k, label=l, want=("order", "rank", "topk", "hits"))
            what = f"k={k} path={path}"
            assert np.array_equal(out["order"].cpu().numpy(), order), what
            assert np.array_equal(out["rank"].cpu().numpy(), rank), what
            assert np.array_equal(out["topk"].cpu().numpy(), topk), what
            assert np.array_equal(out["hits"].cpu().numpy(), hits), what
            assert np.array_equal(seg.edge_segments[0].cpu().numpy(), ptr), what
    r = G.rank_edges(a.view(-1, 1), d.edge_index, d.batch, Gn)                   # the public call, [E, 1] input
    order, rank, topk, _, _ = xo.rank_oracle(att, ei_np, batch_np, Gn, 5)
    assert np.array_equal(r.order.cpu().numpy(), order) and np.array_equal(r.rank.cpu().numpy(), rank)
    assert np.array_equal(G.topk_edge_mask(a, d.edge_index, d.batch, k=5, num_graphs=Gn).cpu().numpy(), topk.astype(bool))


def test_ranking_molhiv_wave_and_workgroup_tiers(dev):
    from dp_gsat_amd import synth
    b = synth.molhiv_batch(2048, seed=0)
    counts = np.bincount(b.batch.numpy()[b.edge_index.numpy()[0]], minlength=2048)
    assert counts.min() <= 64 < counts.max()                                     # both tiers of the fused kernel
    _check_ranking(dev, b, _att(b.num_edges, 1), _labels(b.num_edges, 2), paths=("auto", "fused", "general"))
    _check_ranking(dev, b, _att(b.num_edges, 3, "quantised"), _labels(b.num_edges, 4), paths=("fused", "general"))


def test_ranking_ba2motifs_symmetrised_ties(dev):
    from dp_gsat_amd import synth
    b = synth.ba2motifs_batch(num_graphs=256, seed=3)
    _check_ranking(dev, b, _symmetrised(b, 5), _labels(b.num_edges, 6), paths=("auto", "fused", "general"))


@pytest.mark.parametrize("kind", ["random", "quantised", "constant", "signed"])
def test_ranking_spmotif_and_mutag(dev, kind):
    from dp_gsat_amd import synth
    b = synth.spmotif_batch(num_graphs=300, seed=1)                              # directed
    _check_ranking(dev, b, _att(b.num_edges, 7, kind), _labels(b.num_edges, 8), paths=("fused", "general"))
    m = synth.mutag_batch(os.path.join(ROOT, "tests", "golden", "mutag128.npz"))
    _check_ranking(dev, m, _att(m.num_edges, 9, kind), _labels(m.num_edges, 10), paths=("fused", "general"))


def test_ranking_edge_cases_and_tier_boundaries(dev):
    from dp_gsat_amd import explain as X
    cap = X.rank_edges_lds_cap()
    assert cap >= 128
    for counts in ([5, 0, 0, 7, 0, 3], [0, 0, 9], [11], [0], [0, 0, 0]):           # empty graphs in the middle, G = 1, E = 0
        b = xo.custom_batch(counts, seed=len(counts))
        _check_ranking(dev, b, _att(b.num_edges, 11, "quantised"), _labels(b.num_edges, 12), paths=("auto", "fused", "general"))
    for counts in ([64, 65, 1, 63, 128, 129, 2], [3, 64], [65]):
        b = xo.custom_batch(counts, nodes_per_graph=12, seed=13)
        for kind in ("random", "quantised"):
            _check_ranking(dev, b, _att(b.num_edges, 14, kind), _labels(b.num_edges, 15), paths=("auto", "fused", "general"))
    b = xo.custom_batch([7, cap, 70], nodes_per_graph=40, seed=16)
    _check_ranking(dev, b, _att(b.num_edges, 17, "quantised"), _labels(b.num_edges, 18), paths=("auto", "fused", "general"))
    b = xo.custom_batch([7, cap + 1, 70], nodes_per_graph=40, seed=19)
    _check_ranking(dev, b, _att(b.num_edges, 20, "quantised"), _labels(b.num_edges, 21), paths=("auto",), expect_general=True)


def test_powerlaw_takes_the_general_path_and_forced_fused_raises(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    from dp_gsat_amd._lib import GsatHipError
    b = synth.powerlaw_batch(num_nodes=40_000, num_edges=400_000, num_graphs=4)
    att, lab = _att(b.num_edges, 22, "quantised"), _labels(b.num_edges, 23)
    _check_ranking(dev, b, att, lab, paths=("auto",), expect_general=True)
    d = b.to(dev)
    with pytest.raises(GsatHipError):
        G.rank_edges(torch.from_numpy(att).to(dev), d.edge_index, d.batch, 4, path="fused")


def test_precision_at_k_equals_the_reference_loop(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    for b, seed in ((synth.molhiv_batch(256, seed=4), 30), (synth.ba2motifs_batch(num_graphs=64, seed=5), 31)):
        G.clear_cache()
        att = _symmetrised(b, seed)
        lab = _labels(b.num_edges, seed + 1).astype(np.float32)               # float labels, as edge_label comes
        d = b.to(dev)
        for k in KS:                                                          # 64 and 100 exceed most graphs' edge counts
            ref = xo.precision_at_k_reference_loop(att, lab, k, b.batch.numpy(), b.edge_index.numpy())
            for path in ("auto", "general"):
                got = G.precision_at_k(torch.from_numpy(att).to(dev), torch.from_numpy(lab).to(dev), k, d.batch, d.edge_index, path=path)
                assert got.dtype == torch.float32 and got.is_cuda
                assert np.array_equal(got.cpu().numpy(), ref), (k, path)


def test_auroc_integers_and_float(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import explain as X
    from sklearn.metrics import roc_auc_score
    for E, kind, seed in ((111_310, "random", 40), (111_310, "quantised", 41), (5000, "signed", 42), (777, "constant", 43), (1, "random", 44)):
        att, lab = _att(E, seed, kind), _labels(E, seed + 100, 0.1)
        if E == 1:
            lab[:] = 1
        a, l = torch.from_numpy(att).to(dev), torch.from_numpy(lab).to(dev)
        counts = X.attention_auroc_counts(a, l)
        assert counts.dtype == torch.int64 and tuple(counts.tolist()) == xo.auroc_counts_oracle(att, lab), (E, kind)
        got = G.attention_auroc(a, l)
        assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
        if 0 < lab.sum() < E:
            assert abs(got.item() - roc_auc_score(lab, xo.canon(att))) <= 1e-12, (E, kind)
        else:
            assert got.item() == 0.0
    a = torch.rand(1000, device=dev)
    assert G.attention_auroc(a, torch.zeros(1000, device=dev)).item() == 0.0            # one class only
    assert G.attention_auroc(a, torch.ones(1000, device=dev)).item() == 0.0
    assert G.attention_auroc(a[:0], torch.ones(0, device=dev)).item() == 0.0


def test_delta_kl_and_means(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import explain as X
    for E, seed in ((111_310, 50), (4097, 51), (3, 52)):
        rng = np.random.RandomState(seed)
        att = rng.rand(E).astype(np.float32)
        att[rng.rand(E) < 0.05] = 0.0                                         # values the clamp acts on
        att[rng.rand(E) < 0.05] = 1.0
        lab = _labels(E, seed + 1, 0.3)
        lab[0] = 1
        ref = torch.from_numpy(xo.delta_kl_oracle(att, lab))
        got = X.delta_kl_stats(torch.from_numpy(att).to(dev), torch.from_numpy(lab).to(dev))
        for i, name in enumerate(("delta_kl", "avg_signal_att_weights", "avg_bkg_att_weights")):
            close(got[i:i + 1], ref[i:i + 1], TOL, what=f"{name} E={E}")
        one = G.delta_kl(torch.from_numpy(att).to(dev).view(-1, 1), torch.from_numpy(lab).to(dev))
        assert one.dim() == 0 and one.dtype == torch.float32 and one.item() == got[0].item()


def test_repeatability_is_bitwise(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import explain as X
    from dp_gsat_amd import synth
    b = synth.molhiv_batch(512, seed=6)
    d = b.to(dev)
    a = torch.from_numpy(_att(b.num_edges, 60, "quantised")).to(dev)
    l = torch.from_numpy(_labels(b.num_edges, 61)).to(dev)

    def run(path):
        out, _ = X._rank(a, d.edge_index, d.batch, b.num_graphs, path, k=5, label=l, want=("order", "rank", "topk", "hits"))
        return [out[n] for n in ("order", "rank", "topk", "hits")] + [X.attention_auroc_counts(a, l), X.delta_kl_stats(a, l)]

    for path in ("fused", "general"):
        first, second = run(path), run(path)
        for x, y in zip(first, second):
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.float32 else x, y.view(torch.uint8) if y.dtype == torch.float32 else y)


def _assert_single_chain(dot_text, what):
    """Every node of the dumped graph has at most one successor and one predecessor: one stream, no parallel branches.  Returns False
    when this build produced no dump (the recorded stream handles are the check that always runs)."""
    import re
    if dot_text is None:
        return False
    edges = re.findall(r'^\s*"?([\w.]+)"?(?::\w+)?\s*->\s*"?([\w.]+)"?', dot_text, flags=re.M)
    succ, pred = {}, {}
    for a, b in edges:
        succ.setdefault(a, set()).add(b)
        pred.setdefault(b, set()).add(a)
    fan = {n: sorted(v) for n, v in list(succ.items()) + list(pred.items()) if len(v) > 1}
    assert not fan, f"{what}: the captured graph branches at {fan}\n{dot_text[:3000]}"
    return True


@pytest.mark.parametrize("mode", ["sync_free_general", "fused"])
def test_capture_and_replay_on_refilled_attention(dev, mode, monkeypatch):
    """Ranking, precision@k, AUROC and delta-KL captured into ONE graph; the attention buffer is then refilled and the replay must match
    the oracle for the new values.  Every library call of the capture goes to the one capturing stream (recorded handles), and the
    dumped graph, where the build can dump it, is a single chain without memset nodes.  sync_free_general: sync-free mode, the largest
    graph is unknown inside the step, so the general path is captured.  fused: the warm-up runs cached the bound, the fused kernel is
    captured, with one graph large enough to need more than 48 KiB of dynamic LDS."""
    import dp_gsat_amd as G
    from dp_gsat_amd import explain as X
    from dp_gsat_amd import graph_index, synth
    fused = mode == "fused"
    b = xo.custom_batch([30, 7000, 0, 64, 65, 200], nodes_per_graph=30, seed=70) if fused else synth.molhiv_batch(256, seed=7)
    d = b.to(dev)
    E, Gn = b.num_edges, b.num_graphs
    att0, att1 = _att(E, 70, "quantised"), _att(E, 71, "quantised")
    lab = _labels(E, 72)
    a, l = torch.from_numpy(att0).to(dev), torch.from_numpy(lab).to(dev)
    out, used = {}, []
    path = "fused" if fused else "auto"

    def recording_stream():
        h = _real_stream()
        used.append(h)
        return h

    from dp_gsat_amd import _lib
    _real_stream = _lib.stream
    monkeypatch.setattr(X, "stream", recording_stream)
    monkeypatch.setattr(graph_index, "stream", recording_stream)

    def step():
        out["rank"] = G.rank_edges(a, d.edge_index, d.batch, Gn, path=path)
        out["prec"] = G.precision_at_k(a, l, 5, d.batch, d.edge_index, Gn, path=path)
        out["auc"] = G.attention_auroc(a, l)
        out["counts"] = X.attention_auroc_counts(a, l)
        out["dkl"] = X.delta_kl_stats(a, l)

    G.clear_cache()
    G.set_sync_free(not fused)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        del used[:]
        capture_stream = []

        def captured_step():
            capture_stream.append(_real_stream())
            step()

        graph, dot = capture_with_dump(captured_step)
        assert len(used) >= 5 and set(used) == set(capture_stream), "library calls left the capturing stream"
        assert_no_memset_nodes(dot, "explain metrics")
        _assert_single_chain(dot, "explain metrics")
        a.copy_(torch.from_numpy(att1).to(dev))
        graph.replay()
        torch.cuda.synchronize()
    finally:
        G.set_sync_free(False)
        G.clear_cache()
    order, rank, _, hits, _ = xo.rank_oracle(att1, b.edge_index.numpy(), b.batch.numpy(), Gn, 5, lab)
    assert np.array_equal(out["rank"].order.cpu().numpy(), order) and np.array_equal(out["rank"].rank.cpu().numpy(), rank)
    assert np.array_equal(out["prec"].cpu().numpy(), hits.astype(np.float32) / np.float32(5))
    assert tuple(out["counts"].tolist()) == xo.auroc_counts_oracle(att1, lab)
    assert abs(out["auc"].item() - xo.auroc_oracle(att1, lab)) <= 1e-12
    close(out["dkl"], torch.from_numpy(xo.delta_kl_oracle(att1, lab)), TOL, what="replayed delta_kl")


@pytest.mark.parametrize("ratio", [0.1, 0.3, 0.5, 1.0])
def test_topk_edge_mask_by_ratio(dev, ratio):
    """ceil(ratio * E_g) best edges per graph, with ratios that have no exact binary value, empty graphs and both paths."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    for b in (xo.custom_batch([10, 0, 20, 3, 0, 30, 1, 100, 70], nodes_per_graph=9, seed=3), synth.molhiv_batch(128, seed=13),
              xo.custom_batch([0, 0], seed=1)):
        G.clear_cache()
        att = _att(b.num_edges, 33, "quantised")
        ref = xo.topk_ratio_oracle(att, b.edge_index.numpy(), b.batch.numpy(), b.num_graphs, ratio)
        d = b.to(dev)
        for path in ("auto", "general"):
            got = G.topk_edge_mask(torch.from_numpy(att).to(dev), d.edge_index, d.batch, ratio=ratio, num_graphs=b.num_graphs, path=path)
            assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), ref), (ratio, path)
    with pytest.raises(ValueError):
        G.topk_edge_mask(torch.rand(3, device=dev), d.edge_index, d.batch, k=1, ratio=0.5)


def test_meter_over_three_batches_equals_oracle_on_the_concatenation(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    meter = G.ExplanationMeter(5)
    atts, labs, precs, dkls = [], [], [], []
    for i, b in enumerate((synth.ba2motifs_batch(num_graphs=40, seed=8), synth.molhiv_batch(64, seed=9), synth.spmotif_batch(num_graphs=50, seed=10))):
        att, lab = _att(b.num_edges, 80 + i, "quantised"), _labels(b.num_edges, 90 + i)
        b.edge_label = torch.from_numpy(lab.astype(np.float32))
        meter.update(torch.from_numpy(att).view(-1, 1).to(dev), b.to(dev))
        atts.append(att); labs.append(lab)
        precs.append(xo.precision_at_k_reference_loop(att, lab, 5, b.batch.numpy(), b.edge_index.numpy()))
        dkls.append(xo.delta_kl_oracle(att, lab)[0])
    res = meter.compute()
    att, lab = np.concatenate(atts), np.concatenate(labs)
    assert abs(res["att_auroc"] - xo.auroc_oracle(att, lab)) <= 1e-12
    assert abs(res["precision@5"] - float(np.concatenate(precs).astype(np.float64).mean())) <= 1e-12
    ref = xo.delta_kl_oracle(att, lab)
    assert abs(res["delta_kl"] - np.mean(dkls)) <= TOL * max(1.0, abs(np.mean(dkls)))
    assert abs(res["avg_signal_att_weights"] - ref[1]) <= TOL and abs(res["avg_bkg_att_weights"] - ref[2]) <= TOL


@pytest.mark.parametrize("backbone,edge_mode", [("GIN", True), ("PNA", False)])
def test_forward_pass_feeds_the_meter(dev, backbone, edge_mode):
    """GSAT.forward_pass(training=False) -> ExplanationMeter without a conversion: the [E, 1] tensor of edge mode (ba2motifs) and the
    LiftedAttention view of node mode (molhiv)."""
    import dp_gsat_amd as G
    from dp_gsat_amd import ops, synth
    b = synth.ba2motifs_batch(num_graphs=32, seed=11) if edge_mode else synth.molhiv_batch(32, seed=12, categorical=False)
    H = 32
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=0.0, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=synth.in_degree_histogram(b))
    clf = G.get_model(b.x.shape[1], 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(H, edge_mode).to(dev)
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), None, learn_edge_att=edge_mode).eval()
    lab = _labels(b.num_edges, 95)
    b.edge_label = torch.from_numpy(lab)
    d = b.to(dev)
    with torch.no_grad():
        att, _, _, _ = gsat.forward_pass(d, 0, False)
    assert isinstance(att, ops.LiftedAttention) != edge_mode
    meter = G.ExplanationMeter(5)
    meter.update(att, d)
    res = meter.compute()
    att_np = ops.edge_tensor(att).detach().view(-1).cpu().numpy()
    assert abs(res["att_auroc"] - xo.auroc_oracle(att_np, lab)) <= 1e-12
    prec = xo.precision_at_k_reference_loop(att_np, lab, 5, b.batch.numpy(), b.edge_index.numpy())
    assert abs(res["precision@5"] - float(prec.astype(np.float64).mean())) <= 1e-12
    ref = xo.delta_kl_oracle(att_np, lab)
    assert abs(res["delta_kl"] - ref[0]) <= TOL * max(1.0, abs(ref[0]))
