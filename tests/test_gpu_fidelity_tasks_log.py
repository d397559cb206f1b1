"""gpu: the fidelity-curve log with a task axis (gsat_fidelity_curve_append_tasks / _reduce_tasks, FidelityCurveLog(tasks=T)) against the
fp64 oracle of tests/fidelity_tasks_oracle.py: classes, flip counts, kept-edge sums and n exactly, probabilities within the bound of
tests/test_gpu_fidelity_curve_log.py (the rows go through the same fid_prob), every reduced sum against numpy's sum of the logged doubles,
the log without a task axis at T = 1 bit for bit, the guard entries, the flags."""
import numpy as np
import pytest
import torch

from tests import fidelity_tasks_oracle as fto
from tests.test_gpu_fidelity_curve_log import P_RTOL, _gap, _logits, _stack_valid

pytestmark = pytest.mark.gpu
PAD = 3                                    # guard graphs in front of and behind the log arrays
SENT = 0x5A
# G_rows in {1, 63, 64, 65, 257}, T in {1, 2, 12, 27}, S in {1, 3, 16}: every value once or more, the large ones together once
CASES = [(1, 1, 1), (63, 2, 3), (64, 12, 1), (65, 27, 3), (257, 12, 16), (257, 1, 3), (65, 2, 16), (64, 27, 1)]


def _guarded(log):
    """Move ``cls`` and ``p`` into the middle of larger buffers filled with a sentinel byte; returns the buffers."""
    bufs = []
    for name in ("cls", "p"):
        t = getattr(log, name)
        big = torch.empty((t.shape[0] + 2 * PAD,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        big.view(torch.uint8).fill_(SENT)
        setattr(log, name, big[PAD:PAD + t.shape[0]])
        assert getattr(log, name).is_contiguous()
        bufs.append(big)
    return bufs


def _guards_intact(bufs):
    for big in bufs:
        raw = big.cpu().contiguous().view(torch.uint8).numpy().reshape(big.shape[0], -1)
        if not ((raw[:PAD] == SENT).all() and (raw[-PAD:] == SENT).all()):
            return False
    return True


def _two_appends(dev, Gp, T, S, tasks=True, beyond=float("nan")):
    """A log of capacity 2 Gp after two appends -- one without the input's valid word, one of a ragged padded batch whose rows at and
    beyond valid[2] hold ``beyond`` in every block -- with what the oracle needs."""
    import dp_gsat_amd as G
    V = 2 * S + 1
    ratios = [(s + 1) / (S + 1) for s in range(S)]
    log = G.FidelityCurveLog(2 * Gp, T, ratios=ratios, device=dev, **(dict(tasks=T) if tasks else {}))
    bufs = _guarded(log)
    rng = np.random.RandomState(1000 * T + 10 * Gp + S)
    z1 = _logits(V * Gp, T, 100 * T + Gp + S)
    sv1 = _stack_valid(S, Gp, rng)
    log.append(z1.to(dev), torch.from_numpy(sv1).to(dev))
    real = max(Gp - 3, 0)
    z2 = _logits(V * Gp, T, 7 + 100 * T + Gp + S).view(V, Gp, T)
    z2[:, real:] = beyond
    z2 = z2.reshape(V * Gp, T)
    sv2 = _stack_valid(S, real, rng)
    valid = torch.tensor([5, int(sv2[0, 1]), real, 0], dtype=torch.int32, device=dev)
    log.append(z2.to(dev), torch.from_numpy(sv2).to(dev), valid)
    kept = sv1[1:1 + S, 1].astype(np.int64) + sv2[1:1 + S, 1]
    return log, bufs, (z1.numpy(), z2.numpy(), real, kept, int(sv1[0, 1]) + int(sv2[0, 1]), ratios)


def _bits(log, n):
    return log.cls[:n].cpu().numpy().copy(), log.p[:n].cpu().numpy().view(np.int64).copy()


@pytest.mark.parametrize("Gp,T,S", CASES)
def test_task_log_equals_the_oracle(dev, Gp, T, S):
    log, bufs, (z1, z2, real, kept, edges, ratios) = _two_appends(dev, Gp, T, S)
    V = 2 * S + 1
    assert log.cls.shape == (2 * Gp, T, V) and log.p.shape == (2 * Gp, T, V) and log.tasks == T
    c1, p1 = fto.rows(z1, Gp, S, Gp, T)
    c2, p2 = fto.rows(z2, Gp, S, real, T)
    cls, p = np.concatenate([c1, c2]), np.concatenate([p1, p2])
    n = Gp + real
    assert log.state.tolist() == [n, 2, 0, edges] + kept.tolist() + [0] * (16 - S)           # state[0] counts graphs, not (graph, task)
    assert np.array_equal(log.cls[:n].cpu().numpy(), cls)                                  # classes are exact
    got_p = log.p[:n].cpu().numpy()
    gap = _gap(got_p, p)
    print(f"fidelity task log Gp={Gp} T={T} S={S}: worst relative gap of a probability {gap:.3e}")
    assert gap <= P_RTOL
    assert torch.isfinite(log.p[:n]).all()                                                 # the NaN rows were never loaded
    res, want = log.compute(), fto.compute(cls, p, S, kept, edges, ratios)
    assert set(res) == set(want)
    for key in fto.EXACT_KEYS + ("flip_plus", "flip_minus"):                               # exact integers, their quotients, means of those
        assert res[key] == want[key], (key, res[key], want[key])
    for key in fto.PROB_KEYS:                                                              # the argument of the curve-log test, per task
        got, ref = np.asarray(res[key], np.float64), np.asarray(want[key], np.float64)
        assert got.shape == ref.shape and np.max(np.abs(got - ref)) <= 2 * (P_RTOL + n * 2.0 ** -53), (key, res[key], want[key])
    # every reduced sum against numpy's sum of the doubles the log holds, in the layout include/gsat_hip.h gives for `out`
    out = log._out.cpu().numpy()
    A = 4 + S
    D = A + 2 * T * S
    assert out.size == 4 + S + T * (1 + 6 * S)
    assert out[:4].tolist() == [n, 2, 0, edges] and out[4:A].tolist() == kept.tolist()
    flips = out[A:D].reshape(2, T, S)
    assert np.array_equal(flips[0], (cls[:, :, 1 + S:] != cls[:, :, :1]).sum(axis=0)) and np.array_equal(
        flips[1], (cls[:, :, 1:1 + S] != cls[:, :, :1]).sum(axis=0))
    sums = out[D:].view(np.float64)
    full, per = sums[:T], sums[T:].reshape(4, T, S)
    terms = {"full": got_p[:, :, 0], 0: got_p[:, :, 1:1 + S], 1: got_p[:, :, 1 + S:], 2: got_p[:, :, :1] - got_p[:, :, 1 + S:],
             3: got_p[:, :, :1] - got_p[:, :, 1:1 + S]}
    bound = lambda x: n * 2.0 ** -52 * np.abs(x).sum(axis=0)
    assert (np.abs(full - terms["full"].sum(axis=0)) <= bound(terms["full"])).all()
    for k in range(4):
        assert (np.abs(per[k] - terms[k].sum(axis=0)) <= bound(terms[k])).all(), k
    # the per-level keys are the numpy mean of the returned per-task means
    for key in fto.TASK_KEYS:
        for s in range(S):
            assert res[key][s] == float(np.mean(np.array(res[key + "_tasks"][s], dtype=np.float64))), (key, s)
    assert res["p_full"] == float(np.mean(np.array(res["p_full_tasks"], dtype=np.float64)))
    assert log.compute() == res and _guards_intact(bufs)                                   # bitwise repeatable; nothing written outside
    # a second run, with other values behind valid[2]: not a bit differs
    log2, bufs2, _ = _two_appends(dev, Gp, T, S, beyond=123.0)
    a, b = _bits(log, n), _bits(log2, n)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and log2.compute() == res and _guards_intact(bufs2)


@pytest.mark.parametrize("Gp,S", [(1, 1), (65, 3), (257, 16)])
def test_one_task_is_the_log_without_a_task_axis_bit_for_bit(dev, Gp, S):
    with_tasks, _, _ = _two_appends(dev, Gp, 1, S)
    plain, _, _ = _two_appends(dev, Gp, 1, S, tasks=False)
    n = int(plain.state[0])
    assert n == 2 * Gp - min(Gp, 3) and with_tasks.state.tolist() == plain.state.tolist()
    a, b = _bits(with_tasks, n), _bits(plain, n)
    assert np.array_equal(a[0][:, 0], b[0]) and np.array_equal(a[1][:, 0], b[1])
    got, want = with_tasks.compute(), plain.compute()
    for key, v in want.items():
        assert got[key] == v, key
    for key in fto.TASK_KEYS:
        assert [row[0] for row in got[key + "_tasks"]] == want[key], key
    assert got["p_full_tasks"] == [want["p_full"]]


def test_flags_and_what_a_refused_append_leaves_alone(dev):
    import dp_gsat_amd as G
    T, Gp, S = 12, 65, 3
    V = 2 * S + 1
    rng = np.random.RandomState(0)
    log = G.FidelityCurveLog(3 * Gp, T, ks=[1, 4, 9], device=dev, tasks=T)
    bufs = _guarded(log)
    batches = [(_logits(V * Gp, T, s).to(dev), torch.from_numpy(_stack_valid(S, Gp, rng)).to(dev)) for s in range(4)]
    with pytest.raises(ValueError, match="before any append"):
        log.compute()
    for b in batches[:3]:
        log.append(*b)
    res = log.compute()
    c1, p1, s1 = log.cls.clone(), log.p.clone(), log.state.clone()
    assert res["n"] == 3 * Gp and s1.tolist()[:3] == [3 * Gp, 3, 0]
    unchanged = lambda: torch.equal(log.cls, c1) and torch.equal(log.p.view(torch.int64), p1.view(torch.int64)) and _guards_intact(bufs)
    log.append(*batches[3])                                                    # the log is full: flag bit 1, nothing else written
    assert log.state.tolist() == s1.tolist()[:2] + [2] + s1.tolist()[3:] and unchanged()
    with pytest.raises(ValueError, match="bit 1"):
        log.compute()
    for valid, over in ((torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=dev), None), (None, 0), (None, S), (None, 2 * S)):
        log.reset()
        assert log.state.tolist() == [0] * 20
        log.append(*batches[0])
        before = (log.cls.clone(), log.p.clone(), log.state.clone())
        log.append(batches[1][0], torch.from_numpy(_stack_valid(S, Gp, rng, over)).to(dev), valid)
        assert log.state.tolist() == before[2].tolist()[:2] + [1] + before[2].tolist()[3:]           # overflow: flag bit 0, nothing counted
        assert torch.equal(log.cls, before[0]) and torch.equal(log.p.view(torch.int64), before[1].view(torch.int64)) and _guards_intact(bufs)
        with pytest.raises(ValueError, match="bit 0"):
            log.compute()
    with pytest.raises(ValueError):
        log.append(batches[0][0][:, :2], batches[0][1])
    for kw in (dict(tasks=T + 1), dict(tasks=0), dict(tasks=1025), dict(tasks=T, rankings=2), dict(tasks=True)):
        with pytest.raises(ValueError):
            G.FidelityCurveLog(10, T, ks=[1, 2], device=dev, **kw)
    from dp_gsat_amd import _lib
    with pytest.raises(_lib.GsatHipError):                                      # the entry point's own limits
        _lib.call("gsat_fidelity_curve_append_tasks", None, 0, 1025, 1, None, _lib.ptr(batches[0][1]), None, None, _lib.ptr(log.state), 0,
                  _lib.stream())
