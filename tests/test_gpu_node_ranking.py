"""gpu: node ranking, top-k node masks, node levels and node precision@k (dp_gsat_amd.rank_nodes / topk_node_mask / node_levels /
node_precision_at_k) against tests/node_stack_oracle.py -- graphs of 1, 2, 63, 64, 65 and ~300 nodes (the wave path, its boundary, the
LDS path), scores quantised to five values so that ties dominate, signed zeros, k = 1 and k > N_g, ratio 1.0 -- and the rows of an
unranked padding graph, which must stay unwritten."""
import numpy as np
import pytest
import torch

from tests import node_stack_oracle as nso

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 63, 64, 65, 301, 5]


def _case(seed=0):
    rng = np.random.RandomState(seed)
    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    att = (rng.randint(0, 5, size=len(batch)) / 4).astype(np.float32)                   # five values: ties are the rule
    zeros = np.nonzero(att == 0)[0]
    att[zeros[::2]] = -0.0                                                             # -0.0 counts as +0.0
    assert np.signbit(att).any() and (att == 0).sum() > np.signbit(att).sum()
    label = (rng.rand(len(batch)) < 0.4).astype(np.uint8)
    return att, batch, label


@pytest.fixture(scope="module")
def case(dev):
    att, batch, label = _case()
    return att, batch, label, torch.from_numpy(att).to(dev), torch.from_numpy(batch).to(dev), torch.from_numpy(label).to(dev)


@pytest.mark.parametrize("path", ["auto", "fused", "general"])
def test_rank_nodes_equals_the_stable_sort(dev, case, path):
    import dp_gsat_amd as G
    att, batch, _, a, b, _ = case
    G_ = len(SIZES)
    order, rank, ptr = nso.rank_nodes_oracle(att, batch, G_)
    for shaped in (a, a.view(-1, 1)):
        got = G.rank_nodes(shaped, b, num_graphs=G_, path=path)
        assert isinstance(got, G.NodeRanking) and got.order.dtype == torch.int32
        assert np.array_equal(got.order.cpu().numpy(), order) and np.array_equal(got.rank.cpu().numpy(), rank)
        assert np.array_equal(got.node_ptr.cpu().numpy(), ptr)
    got = G.rank_nodes(a, b)                                                           # the graph count read back from the batch vector
    assert np.array_equal(got.order.cpu().numpy(), order)


def test_masks_levels_and_their_bitwise_agreement(dev, case):
    import dp_gsat_amd as G
    att, batch, _, a, b, _ = case
    G_ = len(SIZES)
    for kw in (dict(ks=[1, 2, 64, 400]), dict(ratios=[0.1, 0.5, 1.0])):
        by_ratio = "ratios" in kw
        levels = next(iter(kw.values()))
        want_lv = nso.node_levels_oracle(att, batch, G_, **kw)
        for bound in (dict(), dict(max_seg_nodes=max(SIZES))):
            lv = G.node_levels(a, b, num_graphs=G_, **kw, **bound)
            assert lv.dtype == torch.uint8 and np.array_equal(lv.cpu().numpy(), want_lv), (kw, bound)
            for s, l in enumerate(levels):
                one = dict(ratio=l) if by_ratio else dict(k=l)
                mask = G.topk_node_mask(a, b, num_graphs=G_, **one, **bound)
                assert mask.dtype == torch.bool and torch.equal(lv <= s, mask), (kw, bound, s)
                assert np.array_equal(mask.cpu().numpy(), nso.topk_node_mask_oracle(att, batch, G_, **one)), (kw, bound, s)
        if by_ratio:
            assert int(lv.max()) < len(levels)                                         # ratio 1.0 keeps every node
    assert G.topk_node_mask(a, b, k=400, num_graphs=G_).all()                          # k above every N_g
    assert int(G.topk_node_mask(a, b, k=1, num_graphs=G_).sum()) == G_


def test_node_precision_and_auroc(dev, case):
    import dp_gsat_amd as G
    from tests import explain_oracle as xo
    att, batch, label, a, b, lab = case
    G_ = len(SIZES)
    for k in (1, 3, 64, 400):
        got = G.node_precision_at_k(a, lab, k, b, num_graphs=G_)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), nso.node_precision_oracle(att, label, k, batch, G_)), k
    got = float(G.attention_auroc(a, lab))                                             # any vector against labels of its length: here nodes
    pos, neg = att[label != 0].astype(np.float64), att[label == 0].astype(np.float64)
    u2 = (2 * (pos[:, None] > neg[None, :]).sum() + (pos[:, None] == neg[None, :]).sum())
    assert got == u2 / (2 * len(pos) * len(neg))


def test_lifted_attention_is_ranked_by_its_node_scores(dev, case):
    import dp_gsat_amd as G
    att, batch, _, a, b, _ = case
    N = len(batch)
    ei = torch.stack([torch.arange(N - 1), torch.arange(1, N)]).to(dev)
    lifted = G.lift_node_att_to_edge_att(a.view(-1, 1), ei)
    G.clear_cache()
    assert torch.equal(G.rank_nodes(lifted, b, num_graphs=len(SIZES)).order, G.rank_nodes(a, b, num_graphs=len(SIZES)).order)
    G.clear_cache()


def test_declared_bounds_and_what_is_refused(dev, case):
    import dp_gsat_amd as G
    from dp_gsat_amd.explain import rank_edges_lds_cap
    att, batch, _, a, b, _ = case
    with pytest.raises(ValueError, match="max_seg_nodes"):
        G.topk_node_mask(a, b, k=1, num_graphs=len(SIZES), max_seg_nodes=rank_edges_lds_cap() + 1)
    with pytest.raises(ValueError, match="max_seg_nodes"):
        G.topk_node_mask(a, b, k=1, num_graphs=len(SIZES), ranked_graphs=2)
    with pytest.raises(ValueError, match="general"):
        G.topk_node_mask(a, b, k=1, num_graphs=len(SIZES), max_seg_nodes=400, path="general")
    with pytest.raises(ValueError):
        G.topk_node_mask(a, b, num_graphs=len(SIZES))
    with pytest.raises(ValueError):
        G.rank_nodes(a[:-1], b, num_graphs=len(SIZES))
    with pytest.raises(ValueError):
        G.node_precision_at_k(a, a, 0, b)


def test_ranked_graphs_leaves_the_padding_graph_unwritten(dev, case):
    """The last graph plays the padding graph: with ``ranked_graphs = G - 1`` its nodes are in no mask and no level, and the ranking
    kernel writes none of their bytes (pre-filled pattern intact)."""
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import call, ptr, stream
    att, batch, _, a, b, _ = case
    G_, N = len(SIZES), len(batch)
    real, pad = G_ - 1, batch == G_ - 1
    bound = dict(num_graphs=G_, max_seg_nodes=max(SIZES), ranked_graphs=real)
    lv = G.node_levels(a, b, ks=[1, 3, 70], **bound)
    assert np.array_equal(lv.cpu().numpy(), nso.node_levels_oracle(att, batch, real, ks=[1, 3, 70])) and (lv.cpu().numpy()[pad] == 3).all()
    for one in (dict(k=3), dict(ratio=0.5)):
        mask = G.topk_node_mask(a, b, **one, **bound).cpu().numpy()
        assert np.array_equal(mask[~pad], nso.topk_node_mask_oracle(att, batch, real, **one)[~pad]), one
    ranking = G.rank_nodes(a, b, num_graphs=G_)
    order = torch.arange(N, dtype=torch.int32, device=dev)
    out = {n: torch.full((N,), 0x5A, dtype=dt, device=dev) for n, dt in (("order", torch.int32), ("rank", torch.int32), ("topk", torch.uint8))}
    call("gsat_rank_edges", ptr(a), ptr(ranking.node_ptr), ptr(order), None, N, real, 3, max(SIZES), 1, ptr(out["order"]), ptr(out["rank"]),
         ptr(out["topk"]), None, None, 0, stream())
    torch.cuda.synchronize()
    pad_t = torch.from_numpy(pad).to(dev)
    for n, t in out.items():
        assert (t[pad_t] == 0x5A).all(), n
    assert torch.equal(out["rank"][~pad_t], ranking.rank[~pad_t]) and torch.equal(out["topk"][~pad_t].bool(), (ranking.rank < 3)[~pad_t])
