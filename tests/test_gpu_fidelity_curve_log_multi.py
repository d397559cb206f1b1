"""gpu: ``FidelityCurveLog(..., rankings=R)`` -- the unchanged gsat_fidelity_curve_append / _reduce with ``R S`` flat levels -- on synthetic
logits of a multi-ranking stack, against tests/fidelity_curve_oracle.py called per ranking: the ``[R][S]`` reshaping, exact integers, and
the probabilities within the existing bound of tests/test_gpu_fidelity_curve_log.py (the fp64 reduction is unchanged)."""
import numpy as np
import pytest
import torch

from tests import fidelity_curve_oracle as fco
from tests import fidelity_multi_oracle as fmo
from tests.test_gpu_fidelity_curve_log import P_RTOL, _logits

pytestmark = pytest.mark.gpu


def _stack_valid(R, S, g, rng):
    """int32[V, 4] of a multi-ranking stack: (nodes, kept edges, g, 0), nested kept counts per ranking."""
    V = 1 + 2 * R * S
    E = int(rng.randint(50, 500))
    v = np.zeros((V, 4), np.int32)
    v[:, 0], v[:, 2], v[0, 1] = 33, g, E
    for r in range(R):
        keep = np.sort(rng.randint(0, E + 1, size=S))
        for s in range(S):
            v[fmo.variant_index(R, S, r, s, True), 1] = keep[s]
            v[fmo.variant_index(R, S, r, s, False), 1] = E - keep[s]
    return v


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("R,S", [(2, 3), (2, 8), (3, 5), (1, 4)])
def test_two_rankings_reshape_to_the_per_ranking_oracle(dev, C, R, S):
    import dp_gsat_amd as G
    Gp, V = 65, 1 + 2 * R * S
    ks = list(range(1, S + 1))
    log = G.FidelityCurveLog(2 * Gp, C, ks=ks, device=dev, rankings=R)
    assert log.rankings == R and log.variants == V and log.levels == tuple(ks)
    rng = np.random.RandomState(100 * C + 10 * R + S)
    batches = []
    for i, g in enumerate((Gp, Gp - 3)):
        z = _logits(V * Gp, C, 7 * i + C + R + S).view(V, Gp, C)
        z[:, g:] = float("nan")                            # rows beyond the graph count are never loaded
        sv = _stack_valid(R, S, g, rng)
        valid = torch.tensor([5, int(sv[0, 1]), g, 0], dtype=torch.int32, device=dev)
        log.append(z.reshape(V * Gp, C).to(dev), torch.from_numpy(sv).to(dev), valid)
        batches.append((z.numpy(), sv, g))
    res = log.compute()
    n = sum(g for _, _, g in batches)
    edges = sum(int(sv[0, 1]) for _, sv, _ in batches)
    assert res["n"] == n and res["levels"] == ks
    p_full = None
    for r in range(R):
        place = [0] + [fmo.variant_index(R, S, r, s, True) for s in range(S)] + [fmo.variant_index(R, S, r, s, False) for s in range(S)]
        rows = [fco.rows(z[place].reshape((2 * S + 1) * Gp, C), Gp, S, g) for z, _, g in batches]
        cls, p = np.concatenate([c for c, _ in rows]), np.concatenate([q for _, q in rows])
        kept = sum(sv[place[1:1 + S], 1].astype(np.int64) for _, sv, _ in batches)
        want = fco.compute(cls, p, S, kept, edges, ks)
        for key in ("flip_plus", "flip_minus", "kept_fraction"):
            got = res[key][r] if R > 1 else res[key]
            assert got == want[key], (r, key, got, want[key])
        for key in ("fidelity_plus", "fidelity_minus", "p_keep", "p_drop"):
            got, ref = np.asarray(res[key][r] if R > 1 else res[key]), np.asarray(want[key])
            assert got.shape == ref.shape == (S,) and np.max(np.abs(got - ref)) <= 2 * (P_RTOL + n * 2.0 ** -53), (r, key, got, ref)
        assert abs(res["p_full"] - want["p_full"]) <= 2 * (P_RTOL + n * 2.0 ** -53)
        p_full = want["p_full"] if p_full is None else p_full
        assert want["p_full"] == p_full                    # one full variant, shared by the rankings
    if R > 1:
        assert all(len(res[key]) == R and all(len(row) == S for row in res[key]) for key in ("fidelity_plus", "flip_minus", "kept_fraction"))
    assert log.compute() == res                            # bitwise repeatable


def test_one_ranking_is_the_log_as_it_was_and_the_product_is_bounded(dev):
    import dp_gsat_amd as G
    C, Gp, S = 2, 33, 3
    V = 2 * S + 1
    rng = np.random.RandomState(4)
    z = _logits(V * Gp, C, 3).to(dev)
    sv = torch.from_numpy(_stack_valid(1, S, Gp, rng)).to(dev)
    a, b = G.FidelityCurveLog(Gp, C, ratios=[0.2, 0.5, 0.8], device=dev), G.FidelityCurveLog(Gp, C, ratios=[0.2, 0.5, 0.8], device=dev, rankings=1)
    a.append(z, sv)
    b.append(z, sv)
    assert a.compute() == b.compute() and torch.equal(a.state, b.state) and torch.equal(a.cls, b.cls)
    assert G.FidelityCurveLog(4, C, ks=list(range(1, 9)), device=dev, rankings=2).variants == 33         # R S = 16
    for kw in (dict(ks=list(range(1, 10)), rankings=2), dict(ks=[1], rankings=17), dict(ks=[1, 2], rankings=0)):
        with pytest.raises(ValueError):
            G.FidelityCurveLog(4, C, device=dev, **kw)
