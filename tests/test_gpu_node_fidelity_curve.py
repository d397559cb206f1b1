"""gpu: the eager front ends of node explanations -- ``explanation_node_subgraph`` and ``explanation_node_fidelity_curve`` (the node stack,
one backbone forward, the scores as device tensors) -- against the log oracle on the returned logits, against the single-level path built
from the unchanged ``node_subgraph_padded`` level by level, and against the CPU oracle backbone on the numpy-extracted subgraphs."""
import numpy as np
import pytest
import torch

from tests import fidelity_curve_oracle as fco
from tests import node_stack_oracle as nso
from tests import subgraph_oracle as so
from tests.test_gpu_subgraph import _models
from tests.util import TOL

pytestmark = pytest.mark.gpu


def _probs(full, other):
    """The probability, under ``other``, of the class ``full`` predicts: the rule of explanation_fidelity."""
    if full.dim() == 2 and full.shape[1] > 1:
        cls = full.argmax(dim=1, keepdim=True)
        return torch.softmax(other.double(), dim=1).gather(1, cls).view(-1)
    sign = torch.where(full >= 0, 1.0, -1.0).double()
    return torch.sigmoid(sign * other.double()).view(-1)


@pytest.mark.parametrize("backbone", ["GIN", "PNA"])
@pytest.mark.parametrize("levels", [dict(ks=[2, 6, 11]), dict(ratios=[0.25, 0.6])], ids=["ks", "ratios"])
def test_eager_node_curve_equals_the_oracles_and_the_single_level_path(dev, backbone, levels):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    data = synth.ba2motifs_batch(num_graphs=14, seed=6)
    data.edge_attr = None
    oclf, clf = _models(dev, data, backbone)
    clf.train()
    d = data.to(dev)
    B, N, E = data.num_graphs, data.num_nodes, data.num_edges
    att_host = (torch.randint(0, 9, (N,), generator=torch.Generator().manual_seed(3)).float() / 8)          # ties: lower node id first
    att = att_host.to(dev)
    values = next(iter(levels.values()))
    S, V = len(values), 2 * len(values) + 1
    res = G.explanation_node_fidelity_curve(clf, d, att.view(-1, 1), **levels)
    assert clf.training and res["levels"] == tuple(values) and res["logits"].shape[:2] == (V, B + 1) and int(res["n"]) == B
    logits = res["logits"]
    cls, p = fco.rows(logits.reshape(V * (B + 1), -1).cpu().numpy(), B + 1, S, B)
    level = nso.node_levels_oracle(att_host.numpy(), data.batch.numpy(), B, **levels)
    assert np.array_equal(G.node_levels(att, d.batch, num_graphs=B, **levels).cpu().numpy(), level)
    ei = data.edge_index.numpy()
    kept_e = [int(((level <= s)[ei[0]] & (level <= s)[ei[1]]).sum()) for s in range(S)]
    kept_n = [int((level <= s).sum()) for s in range(S)]
    want = fco.compute(cls, p, S, kept_e, E, values)
    want["kept_node_fraction"] = [k / N for k in kept_n]
    for key in ("flip_plus", "flip_minus", "kept_fraction", "kept_node_fraction"):
        assert res[key].dtype == torch.float64 and res[key].is_cuda and res[key].tolist() == want[key], (key, res[key], want[key])
    assert all(a < b for a, b in zip(want["kept_node_fraction"], want["kept_node_fraction"][1:]))
    for key in fco.PROB_KEYS:                  # torch's fp64 softmax / sigmoid and a mean of 14 terms against numpy's: fp64 rounding
        assert np.allclose(np.atleast_1d(res[key].cpu().numpy()), np.atleast_1d(want[key]), rtol=0, atol=1e-12), (key, res[key], want[key])

    # level by level against the single-level path: two node_subgraph_padded extractions and three padded forwards
    bound = TOL * max(1.0, float(logits[:, :B].abs().max()))
    clf.eval()
    lv_dev = torch.from_numpy(level).to(dev)
    with torch.no_grad():
        full = clf(d.x, d.edge_index, d.batch, None)
        for s, l in enumerate(values):
            mask = G.topk_node_mask(att, d.batch, num_graphs=B, **(dict(k=l) if "ks" in levels else dict(ratio=l)))
            assert torch.equal(mask, lv_dev <= s)
            single = []
            for m in (mask, ~mask):
                sub = G.node_subgraph_padded(d, m, (N + 2, E))
                G.get_index(sub.edge_index, int(sub.x.shape[0])).graphs(sub.batch, int(sub.num_graphs))
                with G.padded(sub.valid, sub.capacity):
                    single.append(clf(sub.x, sub.edge_index, sub.batch, None)[:B])
            p_full, p_keep, p_drop = _probs(full, full), _probs(full, single[0]), _probs(full, single[1])
            for key, ref in (("fidelity_plus", (p_full - p_drop).mean()), ("fidelity_minus", (p_full - p_keep).mean())):
                assert abs(float(res[key][s]) - float(ref)) <= 2 * bound, (l, key, float(res[key][s]), float(ref))
    clf.train()

    # every variant against the CPU oracle backbone on the numpy-extracted subgraph; these levels empty no graph
    masks = nso.variant_masks(level, S)
    with torch.no_grad():
        for v, mask in enumerate(masks):
            ob, o = so.extract_batch(data, mask, "node", False)
            assert np.bincount(o["batch"], minlength=B).min() > 0, "the levels of this test must empty no graph"
            ref = oclf(ob.x, ob.edge_index, ob.batch, None)
            got = logits[v, :B].cpu().double()
            assert (got - ref.double()).abs().max().item() <= TOL * max(1.0, ref.abs().max().item()), (backbone, v)
    G.clear_cache()


def test_explanation_node_subgraph_is_node_subgraph_on_the_topk_mask(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    data = synth.ba2motifs_batch(num_graphs=6, seed=2)
    d = data.to(dev)
    att_host = torch.randint(0, 5, (data.num_nodes,), generator=torch.Generator().manual_seed(1)).float() / 4
    att = att_host.to(dev)
    for kw in (dict(k=4), dict(ratio=0.3)):
        top = nso.topk_node_mask_oracle(att_host.numpy(), data.batch.numpy(), data.num_graphs, **kw)
        for complement in (False, True):
            sub = G.explanation_node_subgraph(att, d, complement=complement, **kw)
            ob, o = so.extract_batch(data, ~top if complement else top, "node", False)
            assert np.array_equal(sub.node_id.cpu().numpy(), o["node_id"]) and np.array_equal(sub.edge_id.cpu().numpy(), o["edge_id"])
            assert torch.equal(sub.edge_index.cpu(), ob.edge_index) and torch.equal(sub.x.cpu(), ob.x) and torch.equal(sub.batch.cpu(), ob.batch)
            assert torch.equal(sub.node_att.cpu(), att_host[torch.from_numpy(o["node_id"])]) and sub.num_graphs == data.num_graphs
    with pytest.raises(ValueError):
        G.explanation_node_subgraph(att, d)
    with pytest.raises(ValueError):
        G.explanation_node_subgraph(att[:-1], d, k=1)
    G.clear_cache()
