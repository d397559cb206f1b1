"""gpu: the fidelity log (gsat_fidelity_append / gsat_fidelity_reduce / dp_gsat_amd.FidelityLog) against the fp64 oracle of
tests/fidelity_oracle.py: classes and flip counts exactly, probabilities within fp64 rounding, the state word and its flags."""
import numpy as np
import pytest
import torch

from tests import fidelity_oracle as fo

pytestmark = pytest.mark.gpu

# Worst relative gap of a logged probability to the numpy fp64 oracle.  The device exp is not the host's, so the bound is measured, not
# derived: the first MI355X run printed the worst gap over all cases of this file; the bound is 4 x that.
P_RTOL = 4 * 5.65e-16


def _logits(G_rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    full, keep, drop = (torch.randn(G_rows, C, generator=g) * 4 for _ in range(3))
    full[0] = 0.0                                                                      # z = 0 (C = 1) / a tie over every class
    if G_rows > 2 and C > 2:
        full[2, 0], full[2, 1:] = -9.0, 3.0                                            # a tie that does not include class 0
    keep[0] = 0.0
    return full, keep, drop


def _gap(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want))) if len(want) else 0.0


@pytest.mark.parametrize("C", [1, 2, 3, 10])
@pytest.mark.parametrize("G_rows", [1, 63, 64, 65, 257])
def test_append_and_compute_equal_the_oracle(dev, C, G_rows):
    """Two appends -- all rows, then a padded batch whose rows beyond valid[2] are NaN -- then compute()."""
    import dp_gsat_amd as G
    log = G.FidelityLog(2 * G_rows, C, dev)
    full, keep, drop = _logits(G_rows, C, 100 * C + G_rows)
    log.append(full.to(dev), keep.to(dev), drop.to(dev))
    real = max(G_rows - 3, 0)
    f2, k2, d2 = _logits(G_rows, C, 7 + 100 * C + G_rows)
    nan = lambda t: torch.cat([t[:real], torch.full((G_rows - real, C), float("nan"))])
    valid = torch.tensor([5, 6, real, 0], dtype=torch.int32, device=dev)
    log.append(nan(f2).to(dev), nan(k2).to(dev), nan(d2).to(dev), valid)
    c1, p1 = fo.rows(full.numpy(), keep.numpy(), drop.numpy())
    c2, p2 = fo.rows(f2[:real].numpy(), k2[:real].numpy(), d2[:real].numpy()) if real else (np.zeros((0, 3), np.int32), np.zeros((0, 3)))
    cls, p = np.concatenate([c1, c2]), np.concatenate([p1, p2])
    n = G_rows + real
    assert log.state.tolist() == [n, 2, 0, 0]
    assert np.array_equal(log.cls[:n].cpu().numpy(), cls)                              # classes are exact, ties included
    assert cls[0, 0] == (1 if C == 1 else 0) and (C < 3 or G_rows < 3 or cls[2, 0] == 1)
    got_p = log.p[:n].cpu().numpy()
    gap = _gap(got_p, p)
    print(f"fidelity log C={C} G_rows={G_rows}: worst relative gap of a probability {gap:.3e}")
    assert gap <= P_RTOL
    res, want = log.compute(), fo.compute(cls, p)
    assert res["n"] == n and res["flip_plus"] == want["flip_plus"] and res["flip_minus"] == want["flip_minus"]       # exact integers
    for key in ("fidelity_plus", "fidelity_minus", "p_full", "p_keep", "p_drop"):
        # a mean of n probabilities <= 1, each within P_RTOL of the oracle's, moves by at most P_RTOL; adding n such terms in another
        # order moves the sum by at most n * 2^-53 of its size, and the mean (<= 1) by no more
        assert abs(res[key] - want[key]) <= P_RTOL + n * 2.0 ** -53, (key, res[key], want[key])
    assert torch.isfinite(log.p[:n]).all()                                             # the NaN rows were never loaded


def test_state_flags_reset_and_repeatability(dev):
    import dp_gsat_amd as G
    C, rows = 3, 65
    log = G.FidelityLog(3 * rows, C, dev)
    batches = [tuple(t.to(dev) for t in _logits(rows, C, s)) for s in range(4)]
    with pytest.raises(ValueError, match="before any append"):
        log.compute()

    def epoch():
        log.reset()
        for b in batches[:3]:
            log.append(*b)
        return log.compute(), log.cls.clone(), log.p.clone()

    r1, c1, p1 = epoch()
    r2, c2, p2 = epoch()
    assert r1 == r2 and torch.equal(c1, c2) and torch.equal(p1.view(torch.int64), p2.view(torch.int64))             # bitwise
    assert r1["n"] == 3 * rows and log.state.tolist() == [3 * rows, 3, 0, 0]
    # the log is full: flag bit 1, nothing written
    log.append(*batches[3])
    assert log.state.tolist() == [3 * rows, 3, 2, 0]
    assert torch.equal(log.cls, c1) and torch.equal(log.p.view(torch.int64), p1.view(torch.int64))
    with pytest.raises(ValueError, match="bit 1"):
        log.compute()
    # a batch that had overflowed: flag bit 0, nothing written, not counted
    log.reset()
    assert log.state.tolist() == [0, 0, 0, 0]
    log.append(*batches[0])
    before = (log.cls.clone(), log.p.clone())
    log.append(*batches[1], torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=dev))
    assert log.state.tolist() == [rows, 1, 1, 0]
    assert torch.equal(log.cls, before[0]) and torch.equal(log.p.view(torch.int64), before[1].view(torch.int64))
    with pytest.raises(ValueError, match="bit 0"):
        log.compute()
    # valid[2] outside [0, rows] is clamped
    log.reset()
    log.append(*batches[0], torch.tensor([0, 0, rows + 9, 0], dtype=torch.int32, device=dev))
    log.append(*batches[1], torch.tensor([0, 0, -4, 0], dtype=torch.int32, device=dev))
    assert log.state.tolist() == [rows, 2, 0, 0]
    with pytest.raises(ValueError):
        log.append(batches[0][0], batches[0][1][:, :2], batches[0][2])
