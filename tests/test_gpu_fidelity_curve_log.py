"""gpu: the level-aware fidelity log (gsat_fidelity_curve_append / _reduce / _reset, dp_gsat_amd.FidelityCurveLog) against the fp64 oracle
of tests/fidelity_curve_oracle.py: classes, flip counts, kept-edge sums and n exactly, probabilities within the measured fp64 gap, the
state words and their flags."""
import numpy as np
import pytest
import torch

from tests import fidelity_curve_oracle as fco

pytestmark = pytest.mark.gpu

# Worst relative gap of a logged probability to the numpy fp64 oracle.  The device exp is not the host's, so the bound is measured, not
# derived: an MI355X run printed the worst gap over all cases of this file, 6.734e-16 (C = 10; k_fid_rows, whose fid_prob the rows
# kernel reuses, measured 5.65e-16 on its own cases); the bound is 4 x that.
P_RTOL = 4 * 6.734e-16


def _logits(rows, C, seed):
    """fp32 [rows, C] with every |z| >= 1e-3, so that no class decision sits on a rounding edge."""
    z = torch.randn(rows, C, generator=torch.Generator().manual_seed(seed)) * 4
    return torch.where(z.abs() < 1e-3, torch.where(z < 0, -1e-3, 1e-3), z).to(torch.float32)


def _stack_valid(S, g, rng, over=None):
    """int32[V, 4]: (nodes, kept edges, g, 0) with nested edge counts; ``over``: the variant whose overflow word is set."""
    V = 2 * S + 1
    E = int(rng.randint(50, 500))
    keep = np.sort(rng.randint(0, E + 1, size=S))
    v = np.zeros((V, 4), np.int32)
    v[:, 0], v[:, 2] = 33, g
    v[0, 1], v[1:1 + S, 1], v[1 + S:, 1] = E, keep, E - keep
    if over is not None:
        v[over] = [0, 0, 0, 1]
    return v


def _gap(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want))) if want.size else 0.0


@pytest.mark.parametrize("C", [1, 2, 3, 10])
@pytest.mark.parametrize("Gp", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("S", [1, 3, 16])
def test_append_and_compute_equal_the_oracle(dev, C, Gp, S):
    """Two appends -- one without the input's valid word (the stack's own graph count), one of a ragged padded batch whose rows beyond
    valid[2] are NaN in every block -- then compute()."""
    import dp_gsat_amd as G
    V = 2 * S + 1
    ratios = [(s + 1) / (S + 1) for s in range(S)]
    log = G.FidelityCurveLog(2 * Gp, C, ratios=ratios, device=dev)
    rng = np.random.RandomState(1000 * C + 10 * Gp + S)
    z1 = _logits(V * Gp, C, 100 * C + Gp + S)
    sv1 = _stack_valid(S, Gp, rng)
    log.append(z1.to(dev), torch.from_numpy(sv1).to(dev))
    real = max(Gp - 3, 0)
    z2 = _logits(V * Gp, C, 7 + 100 * C + Gp + S).view(V, Gp, C)
    z2[:, real:] = float("nan")
    z2 = z2.reshape(V * Gp, C)
    sv2 = _stack_valid(S, real, rng)
    valid = torch.tensor([5, int(sv2[0, 1]), real, 0], dtype=torch.int32, device=dev)
    log.append(z2.to(dev), torch.from_numpy(sv2).to(dev), valid)
    c1, p1 = fco.rows(z1.numpy(), Gp, S, Gp)
    c2, p2 = fco.rows(z2.numpy(), Gp, S, real)
    cls, p = np.concatenate([c1, c2]), np.concatenate([p1, p2])
    n = Gp + real
    kept = sv1[1:1 + S, 1].astype(np.int64) + sv2[1:1 + S, 1]
    edges = int(sv1[0, 1]) + int(sv2[0, 1])
    assert log.state.tolist() == [n, 2, 0, edges] + kept.tolist() + [0] * (16 - S)
    assert np.array_equal(log.cls[:n].cpu().numpy(), cls)                              # classes are exact
    got_p = log.p[:n].cpu().numpy()
    gap = _gap(got_p, p)
    print(f"fidelity curve log C={C} Gp={Gp} S={S}: worst relative gap of a probability {gap:.3e}")
    assert gap <= P_RTOL
    res, want = log.compute(), fco.compute(cls, p, S, kept, edges, ratios)
    for key in fco.EXACT_KEYS:                                                         # exact integers and their quotients
        assert res[key] == want[key], (key, res[key], want[key])
    for key in fco.PROB_KEYS:
        # a mean of n probabilities <= 1, each within P_RTOL of the oracle's, moves by at most P_RTOL; adding n such terms in another
        # order moves the sum by at most n * 2^-53 of its size, and the mean (<= 1) by no more; a fidelity is a difference of two such
        got, ref = np.atleast_1d(res[key]), np.atleast_1d(want[key])
        assert got.shape == ref.shape and np.max(np.abs(got - ref)) <= 2 * (P_RTOL + n * 2.0 ** -53), (key, res[key], want[key])
    assert torch.isfinite(log.p[:n]).all()                                             # the NaN rows were never loaded
    assert log.compute() == res                                                        # bitwise repeatable


def test_state_flags_reset_and_what_a_refused_append_leaves_alone(dev):
    import dp_gsat_amd as G
    C, Gp, S = 3, 65, 3
    V = 2 * S + 1
    rng = np.random.RandomState(0)
    log = G.FidelityCurveLog(3 * Gp, C, ks=[1, 4, 9], device=dev)
    assert log.levels == (1, 4, 9) and not log.by_ratio and log.variants == V
    batches = [(_logits(V * Gp, C, s).to(dev), torch.from_numpy(_stack_valid(S, Gp, rng)).to(dev)) for s in range(4)]
    with pytest.raises(ValueError, match="before any append"):
        log.compute()

    def epoch():
        log.reset()
        for b in batches[:3]:
            log.append(*b)
        return log.compute(), log.cls.clone(), log.p.clone(), log.state.clone()

    r1, c1, p1, s1 = epoch()
    r2, c2, p2, s2 = epoch()
    assert r1 == r2 and torch.equal(c1, c2) and torch.equal(p1.view(torch.int64), p2.view(torch.int64)) and torch.equal(s1, s2)     # bitwise
    assert r1["n"] == 3 * Gp and r1["levels"] == [1, 4, 9] and s1.tolist()[:3] == [3 * Gp, 3, 0]
    unchanged = lambda: torch.equal(log.cls, c1) and torch.equal(log.p.view(torch.int64), p1.view(torch.int64))
    # the log is full: flag bit 1, nothing else written
    log.append(*batches[3])
    assert log.state.tolist() == s1.tolist()[:2] + [2] + s1.tolist()[3:] and unchanged()
    with pytest.raises(ValueError, match="bit 1"):
        log.compute()
    # an input that had overflowed, and a stack one of whose variants had: flag bit 0, nothing else written, nothing counted
    for valid, over in ((torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=dev), None), (None, 0), (None, S), (None, 2 * S)):
        log.reset()
        assert log.state.tolist() == [0] * 20
        log.append(*batches[0])
        before = (log.cls.clone(), log.p.clone(), log.state.clone())
        sv = torch.from_numpy(_stack_valid(S, Gp, rng, over)).to(dev)
        log.append(batches[1][0], sv, valid)
        assert log.state.tolist() == before[2].tolist()[:2] + [1] + before[2].tolist()[3:]
        assert torch.equal(log.cls, before[0]) and torch.equal(log.p.view(torch.int64), before[1].view(torch.int64))
        with pytest.raises(ValueError, match="bit 0"):
            log.compute()
    # valid[2] outside [0, Gp] is clamped
    log.reset()
    log.append(*batches[0], torch.tensor([0, 0, Gp + 9, 0], dtype=torch.int32, device=dev))
    log.append(*batches[1], torch.tensor([0, 0, -4, 0], dtype=torch.int32, device=dev))
    assert log.state.tolist()[:3] == [Gp, 2, 0]
    with pytest.raises(ValueError):
        log.append(batches[0][0][:, :2], batches[0][1])
    with pytest.raises(ValueError):
        log.append(batches[0][0][:-1], batches[0][1])
    for kw in (dict(), dict(ks=[1], ratios=[0.5]), dict(ks=[2, 1]), dict(ratios=[0.1] * 2), dict(ks=list(range(1, 18)))):
        with pytest.raises(ValueError):
            G.FidelityCurveLog(10, C, device=dev, **kw)
