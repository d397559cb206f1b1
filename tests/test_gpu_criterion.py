"""-m gpu: gsat_criterion_fwd / _bwd (dp_gsat_amd.criterion_valid) against the fp64 oracle of tests/ragged_oracle.py: the three modes over
the first b rows with b read on the device, at the row counts where the kernels' loops branch.  Comparisons follow tests.util.close
(TOL = 1e-4, the fp64 evaluation as ref64).  The gradient is taken with gout = the divisor, so that its entries are O(1) (sigmoid - y,
softmax - onehot) and the tolerance bites at every size."""
import pytest
import torch

from tests import ragged_oracle as ro
from tests.util import TOL, assert_no_memset_nodes, capture_with_dump, close

pytestmark = pytest.mark.gpu

GRID = [1, 63, 64, 65, 257, 5000]
NAN = float("nan")


def _edges(C, mode):
    """Row counts at and one either side of the first-stage block size and of the size at which every block is in use."""
    from dp_gsat_amd._lib import load
    items, blocks = int(load().gsat_criterion_block_items(C, mode)), int(load().gsat_criterion_max_blocks())
    per_row = 1 if mode == 1 else C
    out = set()
    for total in (items, items * blocks):
        rows = -(-total // per_row)
        out.update(r for r in (rows - 1, rows, rows + 1) if r >= 1)
    return sorted(out)


def _counts(G):
    return sorted({0, 1, max(G // 2, 1) | 1 if G > 2 else 1, G - 1, G} & set(range(G + 1))) + [None]


def _divisor(y, mode, C, b):
    if mode == 2:
        return max(int((y[:b] == y[:b]).sum()), 1)
    return max(b * (1 if mode == 1 else C), 1)


def _check(dev, G, C, mode, b, z, y):
    """One (G, b): rows >= b hold NaN on the device, the oracle never sees them."""
    import dp_gsat_amd as A
    rows = G if b is None else b
    gout = float(_divisor(y, mode, C, rows))
    a64 = z.double().requires_grad_(True)
    ref = ro.criterion64(a64, y, mode, rows)
    (ref * gout).backward()
    zd, yd = z.clone(), y.clone()
    zd[rows:], yd[rows:] = NAN, NAN
    zd = zd.to(dev).requires_grad_(True)
    yd = yd.to(dev)
    gv = None if b is None else torch.tensor([b], dtype=torch.int32, device=dev)
    if mode == 1 and C == 2:           # Criterion's rule sends two classes to the binary mode: the two-column cross entropy has no public name
        run = lambda t: A.ops.CriterionLoss.apply(t, yd, 1, gv)
    else:
        num_class, multi = {0: (2, False), 1: (C, False), 2: (C, True)}[mode]
        run = lambda t: A.criterion_valid(t, yd, num_class, multi, gv)
    out = run(zd)
    (out * gout).backward()
    again = run(zd.detach())
    what = f"mode {mode} G={G} C={C} b={b}: "
    assert out.dtype == torch.float32 and out.shape == () and torch.isfinite(out), what + "loss"
    assert torch.equal(out.detach(), again), what + "two calls give equal bits"
    ref = ref.detach()
    close(out, ref.float(), TOL, ref64=ref, what=what + "loss")
    close(zd.grad[:rows], a64.grad[:rows].float(), TOL, ref64=a64.grad[:rows], what=what + "dlogits")
    assert torch.equal(zd.grad[rows:], torch.zeros_like(zd.grad[rows:])), what + "dlogits of rows >= b must be exactly 0"
    if rows == 0 or (mode == 2 and not (y[:rows] == y[:rows]).any()):
        assert float(out.detach()) == 0.0 and not zd.grad.any(), what + "an empty selection gives 0 and zero gradients"


def _sweep(dev, C, mode, sizes, counts=_counts):
    for G in sizes:
        z, y = ro.criterion_case(G, C, mode, 100 * G + C)
        assert float(z.max()) == 100.0
        for b in counts(G):
            _check(dev, G, C, mode, b, z, y)


def _some(G):
    return [max(G // 2, 1) | 1, G - 1, None]


def test_binary_criterion(dev):
    _sweep(dev, 1, 0, GRID)
    _sweep(dev, 1, 0, _edges(1, 0), _some)


@pytest.mark.parametrize("C", [2, 3, 7, 130])
def test_cross_entropy_criterion(dev, C):
    _sweep(dev, C, 1, GRID)
    _sweep(dev, C, 1, _edges(C, 1), _some)


@pytest.mark.parametrize("C", [1, 12])
def test_multi_label_criterion(dev, C):
    _sweep(dev, C, 2, GRID)
    _sweep(dev, C, 2, _edges(C, 2), _some)


def test_criterion_is_stable_at_large_logits(dev):
    """z = +-100: log(1 + exp(z)) overflows in fp32, the max-subtracted forms do not."""
    import dp_gsat_amd as A
    z = torch.tensor([[100.0], [-100.0], [100.0], [-100.0], [88.8], [0.0]])
    y = torch.tensor([[1.0], [0.0], [0.0], [1.0], [0.0], [1.0]])
    for mode, (zz, yy, nc) in enumerate([(z, y, 2), (torch.cat([z, -z, z * 0], 1), torch.tensor([0.0, 1, 2, 0, 1, 2]), 3), (z, y, 1)]):
        zd = zz.to(dev).requires_grad_(True)
        out = A.criterion_valid(zd, yy.to(dev), nc, mode == 2)
        out.backward()
        ref = ro.criterion64(zz, yy, mode)
        assert torch.isfinite(out) and torch.isfinite(zd.grad).all(), mode
        assert float(ref) > 30.0
        close(out, ref.float(), TOL, ref64=ref, what=f"mode {mode} at +-100")


def test_cross_entropy_bad_label_gives_nan(dev):
    """A label of C, -1 or NaN makes the loss NaN; the label is never used as an offset (a good row next to it keeps its gradient)."""
    import dp_gsat_amd as A
    for C in (3, 130):
        for bad in (float(C), -1.0, NAN, 1e9):
            z, y = ro.criterion_case(70, C, 1, C)
            y[5] = bad
            zd = z.to(dev).requires_grad_(True)
            out = A.criterion_valid(zd, y.to(dev), C)
            out.backward()
            torch.cuda.synchronize()
            assert torch.isnan(out), (C, bad)
            assert torch.isfinite(zd.grad[:5]).all() and torch.isfinite(zd.grad[6:]).all()
            gv = torch.tensor([5], dtype=torch.int32, device=dev)          # the bad row is not counted: finite again
            assert torch.isfinite(A.criterion_valid(zd.detach(), y.to(dev), C, False, gv))


def test_criterion_sizes_and_arguments(dev):
    import dp_gsat_amd as A
    from dp_gsat_amd._lib import GsatHipError, call, ptr, stream
    z = torch.zeros(4, 2, device=dev)
    buf = lambda n: torch.empty(n, device=dev)
    for G, C in (((1 << 20) + 1, 1), (1, 1025)):          # refused before any launch: the extents are never used
        with pytest.raises(GsatHipError, match="code -4"):
            call("gsat_criterion_fwd", ptr(z), ptr(z), G, C, 0, None, ptr(buf(512)), ptr(buf(1)), ptr(buf(4)), stream())
        with pytest.raises(GsatHipError, match="code -4"):
            call("gsat_criterion_bwd", ptr(z), ptr(z), ptr(buf(4)), ptr(buf(1)), G, C, 0, None, ptr(z), stream())
    with pytest.raises(GsatHipError, match="code -2"):
        call("gsat_criterion_fwd", ptr(z), ptr(z), 4, 2, 3, None, ptr(buf(512)), ptr(buf(1)), ptr(buf(4)), stream())
    with pytest.raises(ValueError, match="g_valid"):
        A.criterion_valid(z, z, 2, True, torch.tensor([1], device=dev))
    with pytest.raises(ValueError, match="target"):
        A.criterion_valid(z, z, 3)
    G = 1 << 20                                             # the largest supported row count, a count past it is clamped
    zl, yl = ro.criterion_case(G, 1, 0, 9)
    gv = torch.tensor([G + 5], dtype=torch.int32, device=dev)
    out = A.criterion_valid(zl.to(dev), yl.to(dev), 2, False, gv)
    ref = ro.criterion64(zl, yl, 0)
    close(out, ref.float(), TOL, ref64=ref, what="G = 2^20")
    wide, yw = ro.criterion_case(3, 1024, 1, 4)
    ref = ro.criterion64(wide, yw, 1)
    close(A.criterion_valid(wide.to(dev), yw.to(dev), 1024), ref.float(), TOL, ref64=ref, what="C = 1024")
    # Criterion.forward: g_valid picks the kernel, None keeps torch's arithmetic
    crit = A.Criterion(2, False)
    zs, ys = ro.criterion_case(9, 1, 0, 2)
    three = torch.tensor([3], dtype=torch.int32, device=dev)
    close(crit(zs.to(dev), ys.to(dev), g_valid=three), crit(zs[:3].to(dev), ys[:3].to(dev)), TOL, what="Criterion(g_valid)")


def test_captured_criterion_reads_the_count_on_replay(dev):
    """Forward and backward captured once: no memset node, and a replay follows the count and the logits written before it."""
    from dp_gsat_amd._lib import call, ptr, stream
    G, C = 300, 7
    z, y = ro.criterion_case(G, C, 1, 11)
    zd, yd = z.to(dev), y.to(dev)
    gv = torch.tensor([G], dtype=torch.int32, device=dev)
    partial, loss, stats = torch.empty(512, device=dev), torch.empty((), device=dev), torch.empty(4, device=dev)
    gout, dz = torch.ones((), device=dev), torch.empty(G, C, device=dev)

    def fn():
        call("gsat_criterion_fwd", ptr(zd), ptr(yd), G, C, 1, ptr(gv), ptr(partial), ptr(loss), ptr(stats), stream())
        call("gsat_criterion_bwd", ptr(zd), ptr(yd), ptr(stats), ptr(gout), G, C, 1, ptr(gv), ptr(dz), stream())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph, text = capture_with_dump(fn)
    assert_no_memset_nodes(text, "gsat_criterion")
    assert text is None or "memcpy" not in text.lower(), "the captured criterion contains a memcpy node"
    for b in (G, 41, 0):
        gv.fill_(b)
        graph.replay()
        torch.cuda.synchronize()
        a64 = z.double().requires_grad_(True)
        ref = ro.criterion64(a64, y, 1, b)
        ref.backward()
        close(loss, ref.detach().float(), TOL, ref64=ref.detach(), what=f"replay b={b}: loss")
        close(dz * max(b, 1), (a64.grad * max(b, 1)).float(), TOL, ref64=a64.grad * max(b, 1), what=f"replay b={b}: dlogits")
        assert not dz[b:].any()
