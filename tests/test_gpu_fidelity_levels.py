"""gpu: ``explanation_levels`` -- every sparsity level of a fidelity curve from one ranking -- against ``topk_edge_mask`` level by level
(bit for bit) and against tests/fidelity_stack_oracle.py, on graphs whose edge counts reach both branches of the fused ranking."""
import numpy as np
import pytest
import torch

from tests import explain_oracle as xo
from tests import fidelity_stack_oracle as fso

pytestmark = pytest.mark.gpu
EDGE_COUNTS = [0, 1, 2, 63, 64, 65, 300, 0, 7]           # wavefront-sized and workgroup-sized graphs, empty ones in between and last
LEVELS = [dict(ks=[1]), dict(ks=[2, 64]), dict(ks=[1, 2, 3, 5, 8, 13, 21, 34, 55, 63, 64, 65, 89, 144, 299, 400]),       # k > E_g
          dict(ratios=[1.0]), dict(ratios=[0.3, 1.0]), dict(ratios=[(i + 1) / 16 for i in range(16)])]


def _att(kind, E):
    if kind == "equal":
        return torch.full((E,), 0.25)                                                  # every edge ties: lower edge id first
    a = torch.rand(E, generator=torch.Generator().manual_seed(E))
    a[::4] = 0.5                                                                       # a block of ties inside every graph
    return a


@pytest.mark.parametrize("kind", ["random", "equal"])
@pytest.mark.parametrize("levels", LEVELS, ids=lambda kw: f"{next(iter(kw))}{len(next(iter(kw.values())))}")
def test_levels_equal_topk_edge_mask_for_every_level(dev, kind, levels):
    import dp_gsat_amd as G
    G.clear_cache()
    b = xo.custom_batch(EDGE_COUNTS, nodes_per_graph=9, seed=2)
    d = b.to(dev)
    att = _att(kind, b.num_edges).to(dev)
    values = next(iter(levels.values()))
    S = len(values)
    cap = int(G.explain.rank_edges_lds_cap())
    assert cap >= max(EDGE_COUNTS)
    for bound in (None, max(EDGE_COUNTS)):                                             # the path the batch picks, and the declared fused path
        lv = G.explanation_levels(att, d.edge_index, d.batch, num_graphs=b.num_graphs, max_seg_edges=bound, **levels)
        assert lv.dtype == torch.uint8 and lv.shape == (b.num_edges,) and int(lv.max()) <= S
        for s, l in enumerate(values):
            one = dict(k=l) if "ks" in levels else dict(ratio=l)
            want = G.topk_edge_mask(att, d.edge_index, d.batch, num_graphs=b.num_graphs, max_seg_edges=bound, **one)
            assert torch.equal(lv <= s, want), (kind, levels, s, bound)
        want = fso.levels_oracle(att.cpu().numpy(), b.edge_index.numpy(), b.batch.numpy(), b.num_graphs, **levels)
        assert np.array_equal(lv.cpu().numpy(), want), (kind, levels, bound)
    if "ratios" in levels and values[-1] == 1.0:
        assert int(lv.max()) < S                                                       # ratio 1.0 keeps every edge
    G.clear_cache()


def test_unranked_graphs_get_no_level_and_bad_levels_are_refused(dev):
    import dp_gsat_amd as G
    G.clear_cache()
    b = xo.custom_batch([5, 9, 4], nodes_per_graph=5, seed=1)
    d = b.to(dev)
    att = torch.rand(b.num_edges, generator=torch.Generator().manual_seed(0)).to(dev)
    lv = G.explanation_levels(att, d.edge_index, d.batch, ks=[2, 4], num_graphs=3, max_seg_edges=9, ranked_graphs=2)
    graph_of_edge = b.batch[b.edge_index[0]]
    assert (lv.cpu()[graph_of_edge == 2] == 2).all()                                   # the last graph is not ranked: no level keeps its edges
    want = G.explanation_levels(att, d.edge_index, d.batch, ks=[2, 4], num_graphs=3)
    assert torch.equal(lv.cpu()[graph_of_edge < 2], want.cpu()[graph_of_edge < 2])
    for kw in (dict(), dict(ks=[1], ratios=[0.5]), dict(ks=[2, 2]), dict(ratios=[0.5, 0.2]), dict(ks=list(range(1, 18)))):
        with pytest.raises(ValueError):
            G.explanation_levels(att, d.edge_index, d.batch, num_graphs=3, **kw)
    G.clear_cache()
