"""gpu: the eager front end ``explanation_fidelity_curve`` -- the stack, one backbone forward, the scores as device tensors -- against the log
oracle on the logits it returns and against the single-level ``explanation_fidelity`` (unchanged code) level by level."""
import numpy as np
import pytest
import torch

from tests import fidelity_curve_oracle as fco
from tests.test_gpu_subgraph import _models
from tests.util import TOL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("backbone", ["GIN", "PNA"])
@pytest.mark.parametrize("levels", [dict(ks=[2, 6, 11]), dict(ratios=[0.25, 0.6])], ids=["ks", "ratios"])
def test_eager_curve_equals_the_oracle_and_the_single_level_fidelity(dev, backbone, levels):
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    G.clear_cache()
    data = synth.ba2motifs_batch(num_graphs=14, seed=6)
    data.edge_attr = None
    _, clf = _models(dev, data, backbone)
    clf.train()
    d = data.to(dev)
    B, E = data.num_graphs, data.num_edges
    att = torch.rand(E, generator=torch.Generator().manual_seed(3)).to(dev)
    values = next(iter(levels.values()))
    S, V = len(values), 2 * len(values) + 1
    res = G.explanation_fidelity_curve(clf, d, att, **levels)
    assert clf.training and res["levels"] == tuple(values) and res["logits"].shape[:2] == (V, B + 1) and int(res["n"]) == B
    logits = res["logits"]
    cls, p = fco.rows(logits.reshape(V * (B + 1), -1).cpu().numpy(), B + 1, S, B)
    level = G.explanation_levels(att, d.edge_index, d.batch, num_graphs=B, **levels)
    kept = [int((level <= s).sum()) for s in range(S)]
    want = fco.compute(cls, p, S, kept, E, values)
    for key in ("flip_plus", "flip_minus", "kept_fraction"):
        assert res[key].dtype == torch.float64 and res[key].is_cuda and res[key].tolist() == want[key], (key, res[key], want[key])
    for key in fco.PROB_KEYS:                  # torch's fp64 softmax / sigmoid and a mean of 14 terms against numpy's: fp64 rounding
        assert np.allclose(np.atleast_1d(res[key].cpu().numpy()), np.atleast_1d(want[key]), rtol=0, atol=1e-12), (key, res[key], want[key])
    bound = TOL * max(1.0, float(logits[:, :B].abs().max()))
    for s, l in enumerate(values):             # the path as it was; softmax and sigmoid are 1-Lipschitz in the logits
        single = G.explanation_fidelity(clf, d, att, **(dict(k=l) if "ks" in levels else dict(ratio=l)))
        for key in ("fidelity_plus", "fidelity_minus"):
            assert abs(float(res[key][s]) - float(single[key])) <= 2 * bound, (l, key, float(res[key][s]), float(single[key]))
    G.clear_cache()
