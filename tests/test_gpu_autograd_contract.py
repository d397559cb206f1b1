"""-m gpu: the contract of the autograd wrappers of dp_gsat_amd/ops.py under the ways users call them -- frozen inputs, unused outputs,
views, re-runs, a partial backward before the full one, in-place edits of saved inputs, no-grad forwards -- over the table of
tests/autograd_cases.py.  Every comparison with a reference is ``|actual - ref64| <= TOL * scale + 4 |ref32 - ref64|`` (tests/util.close;
the PNA entries per entry through test_gpu_pna's conditioning weights), and tests/test_autograd_cases_host.py keeps the slack term at or
below TOL * scale.  Everything goes through the wrappers, which allocate every output and gradient themselves: no test here hands the C
ABI a buffer of its own.  Comparisons between two device runs are bitwise."""
import pytest
import torch

from tests import autograd_cases as ac
from tests.test_gpu_pna import close_weighted
from tests.util import TOL, close

pytestmark = pytest.mark.gpu

_CASES = ac.pattern_cases()


def _ids(pattern):
    return [pytest.param(n, d, id=n + ("-" + d if d else "")) for p, n, d in _CASES if p == pattern]


def _names(pattern):
    return [n for p, n, _ in _CASES if p == pattern]


def _setup(case, monkeypatch):
    """The environment a case names, and a process that has seen no hub yet (else an earlier test's hub rows route a batch whose status
    has not landed to the chunked path)."""
    monkeypatch.setattr("dp_gsat_amd.graph_index._HUBS_SEEN", [False])
    for k in ("GSAT_PNA_COMPACT", "GSAT_PNA_TILED", "GSAT_NODE_ATT_LIFT", "GSAT_NODE_ATT_SHARED_GRAD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if case.own_gemm_flops is not None:
        monkeypatch.setattr("dp_gsat_amd.ops._OWN_GEMM_FLOPS", case.own_gemm_flops)


def _leaves(case, dev, need=None):
    return {k: v.to(dev).clone().requires_grad_(need is None or k in need) for k, v in case.inputs.items()}


def _gouts(case, dev):
    return [g.to(dev) for g in case.gouts()]


def _backward(outs, gouts, used=None, retain=False):
    pick = [i for i in range(len(outs)) if (used is None or used[i]) and outs[i].requires_grad]
    torch.autograd.backward([outs[i] for i in pick], [gouts[i].reshape(outs[i].shape) for i in pick], retain_graph=retain)


def _grads(t):
    return {k: (None if v.grad is None else v.grad.clone()) for k, v in t.items()}


def _step(case, dev, need=None, used=None):
    t = _leaves(case, dev, need)
    outs = case.device(dev, t)
    _backward(outs, _gouts(case, dev), used)
    return tuple(o.detach() for o in outs), _grads(t)


_BASELINE = {}


def _baseline(case, dev):
    """The all-require-grad, contiguous, dense-gradient run of a case: computed once and left unchanged."""
    if case.name not in _BASELINE:
        _BASELINE[case.name] = _step(case, dev)
    return _BASELINE[case.name]


def _against_reference(case, outs, grads, need=None, used=None):
    (o32, g32), (o64, g64) = ac.reference(case, torch.float32, need, used), ac.reference(case, torch.float64, need, used)
    assert len(outs) == len(o64)
    for i, (a, r32, r64) in enumerate(zip(outs, o32, o64)):
        assert not torch.isnan(a).any(), f"{case.name}: out{i} has NaN entries"
        close(a.reshape(r32.shape), r32, TOL, ref64=r64, what=f"{case.name}: out{i}")
    for k in case.diff:
        if g64[k] is None:
            assert grads[k] is None, f"{case.name}: d{k} must be absent (no path / frozen), got a tensor"
            continue
        assert grads[k] is not None, f"{case.name}: d{k} is missing"
        assert not torch.isnan(grads[k]).any(), f"{case.name}: d{k} has NaN entries"
        a = grads[k].reshape(g32[k].shape)
        if k in case.weights:
            close_weighted(a, g32[k], g64[k], case.weights[k], f"{case.name}: d{k}")
        else:
            close(a, g32[k], TOL, ref64=g64[k], what=f"{case.name}: d{k}")


def _bitwise(a, b, what):
    assert (a is None) == (b is None), f"{what}: one of the two is absent"
    if a is not None:
        assert a.shape == b.shape and torch.equal(a, b), f"{what}: not bitwise equal (max diff {(a - b).abs().max().item():.3e})"


# ---- 1. baseline ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("baseline"))
def test_baseline_matches_fp64(dev, monkeypatch, name):
    case = ac.get(name)
    _setup(case, monkeypatch)
    outs, grads = _baseline(case, dev)
    _against_reference(case, outs, grads)


# ---- 2. frozen subsets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,subset", _ids("frozen"))
def test_frozen_inputs_get_no_gradient_and_change_no_other(dev, monkeypatch, name, subset):
    """Only ``subset`` requires grad: the frozen inputs end with .grad None, the others match fp64 and are bit for bit the baseline's (the
    same launch writes them; an entry's ``other_launch`` names the exceptions and why)."""
    case = ac.get(name)
    _setup(case, monkeypatch)
    need = frozenset(subset.split("+"))
    base_outs, base_grads = _baseline(case, dev)
    outs, grads = _step(case, dev, need)
    _against_reference(case, outs, grads, need)
    for a, b in zip(outs, base_outs):
        _bitwise(a, b, f"{name}: output")
    for k in case.diff:
        if k not in need:
            assert grads[k] is None
        elif k not in case.other_launch:
            _bitwise(grads[k], base_grads[k], f"{name}: d{k} with only {sorted(need)} requiring grad")


# ---- 3. unused outputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mask", _ids("unused"))
def test_unused_output_contributes_nothing(dev, monkeypatch, name, mask):
    """The backward runs through one output only.  Where the reference has no gradient (only the pass-through output used: no path to the
    attention or the weights) the wrapper's must be absent too -- None, not a zero-filled tensor."""
    case = ac.get(name)
    _setup(case, monkeypatch)
    used = tuple(c == "1" for c in mask)
    outs, grads = _step(case, dev, used=used)
    _against_reference(case, outs, grads, used=used)
    if name.endswith("_passthrough") and used == (False, True):
        _bitwise(grads["x"], _gouts(case, dev)[1], f"{name}: dx is the pass-through gradient itself")


# ---- 4. layouts --------------------------------------------------------------------------------------------------------------------------
def _as_view(v, kind):
    """(leaf, the view of it that is fed to the wrapper, leaf.grad -> gradient in v's shape) for a contiguous device tensor ``v``."""
    if kind == "colslice":
        wide = torch.zeros(v.shape[0], v.shape[1] + 8, device=v.device)
        wide[:, 4:4 + v.shape[1]] = v
        leaf = wide.requires_grad_(True)

        def back(g):
            assert float(g[:, :4].abs().max()) == 0.0 and float(g[:, 4 + v.shape[1]:].abs().max()) == 0.0
            return g[:, 4:4 + v.shape[1]]
        return leaf, leaf[:, 4:4 + v.shape[1]], back
    if kind == "transposed":
        leaf = v.t().contiguous().t().detach().requires_grad_(True)
        return leaf, leaf, lambda g: g
    if kind == "flat":
        leaf = v.reshape(-1).clone().requires_grad_(True)
        return leaf, leaf, lambda g: g.reshape(v.shape)
    if kind == "column":
        leaf = v.reshape(-1, 1).clone().requires_grad_(True)
        return leaf, leaf, lambda g: g.reshape(v.shape)
    raise ValueError(kind)


@pytest.mark.parametrize("name", _names("layouts"))
def test_views_and_strided_gradients_equal_the_contiguous_call(dev, monkeypatch, name):
    """Inputs as a column slice of a wider tensor, with transposed storage, attention as [E] / [E, 1] / an expanded scalar; upstream
    gradients with stride 0 (what out.sum().backward() produces) and with transposed storage: bitwise the contiguous call.  Every view here
    is non-contiguous or a whole allocation, so the wrapper's own copy (or the allocation) is what the kernel reads: no misaligned pointer."""
    case = ac.get(name)
    _setup(case, monkeypatch)
    base_outs, base_grads = _baseline(case, dev)
    gouts = _gouts(case, dev)
    for k, kinds in case.layouts.items():
        for kind in kinds:
            t = _leaves(case, dev)
            if kind == "expanded":
                # all entries equal: compared with the contiguous call on the same values.  The scalar's gradient is autograd's sum of the
                # wrapper's gradient -- another launch than the baseline's, compared at TOL instead of bit for bit
                s = t[k].detach().flatten()[0].reshape([1] * t[k].dim()).clone().requires_grad_(True)
                full = s.detach().expand(t[k].shape).contiguous().requires_grad_(True)
                res = []
                for fed in (s.expand(t[k].shape), full):
                    tt = _leaves(case, dev)
                    tt[k] = fed
                    outs = case.device(dev, tt)
                    _backward(outs, gouts)
                    res.append((outs, {n: v.grad for n, v in tt.items() if n != k}))
                assert t[k].numel() == 1 or not s.expand(t[k].shape).is_contiguous()
                for a, b in zip(res[0][0], res[1][0]):
                    _bitwise(a.detach(), b.detach(), f"{name}: output with {k} expanded")
                for n in res[0][1]:
                    _bitwise(res[0][1][n], res[1][1][n], f"{name}: d{n} with {k} expanded")
                close(s.grad.reshape(()), full.grad.sum(), TOL, what=f"{name}: d{k} of the expanded scalar")
                continue
            leaf, view, back = _as_view(t[k].detach(), kind)
            assert kind in ("flat", "column") or not view.is_contiguous()
            t[k] = view
            outs = case.device(dev, t)
            _backward(outs, gouts)
            for a, b in zip(outs, base_outs):
                _bitwise(a.detach().reshape(b.shape), b, f"{name}: output with {k} as {kind}")
            for n in case.diff:
                g = back(leaf.grad) if n == k else t[n].grad
                _bitwise(g, base_grads[n], f"{name}: d{n} with {k} as {kind}")
    # upstream gradients: transposed storage
    t = _leaves(case, dev)
    outs = case.device(dev, t)
    strided = [g.t().contiguous().t() if g.dim() == 2 and min(g.shape) > 1 else g for g in gouts]
    _backward(outs, strided)
    for n in case.diff:
        _bitwise(t[n].grad, base_grads[n], f"{name}: d{n} under a transposed-storage upstream gradient")
    # upstream gradients: the stride-0 ones of sum().backward() against dense ones
    res = []
    for dense in (False, True):
        t = _leaves(case, dev)
        outs = case.device(dev, t)
        if dense:
            _backward(outs, [torch.ones_like(o) for o in outs])
        else:
            sum(o.sum() for o in outs).backward()
        res.append(_grads(t))
    for n in case.diff:
        _bitwise(res[0][n], res[1][n], f"{name}: d{n} under sum().backward()")


# ---- 5. re-runs --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("rerun"))
def test_backward_twice_through_a_retained_graph(dev, monkeypatch, name):
    """Second backward: bitwise the first; a third, into the existing .grad: exactly twice the value.  The in-kernel-Philox extractor and
    the BatchNorm dropout draw the same masks again (fixed seed); the hub entries share index.partial(H) between the calls."""
    case = ac.get(name)
    _setup(case, monkeypatch)
    _, base_grads = _baseline(case, dev)
    gouts = _gouts(case, dev)
    t = _leaves(case, dev)
    outs = case.device(dev, t)
    _backward(outs, gouts, retain=True)
    first = _grads(t)
    for v in t.values():
        v.grad = None
    _backward(outs, gouts, retain=True)
    for k in case.diff:
        _bitwise(first[k], base_grads[k], f"{name}: d{k}, first backward")
        _bitwise(t[k].grad, first[k], f"{name}: d{k}, second backward")
    _backward(outs, gouts)
    for k in case.diff:
        _bitwise(t[k].grad, 2 * first[k], f"{name}: d{k} accumulated into an existing .grad")


# ---- 6. partial, then full ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("partial_full"))
def test_full_backward_after_a_partial_one(dev, monkeypatch, name):
    """torch.autograd.grad on the first input group alone (saliency, a gradient penalty) prunes nodes from that pass; the full backward
    through the same graph afterwards must be bit for bit the full backward of a fresh graph.  On the three-layer stacks the pruned node
    is the one that used to clear the shared d node_att buffer."""
    case = ac.get(name)
    _setup(case, monkeypatch)
    _, base_grads = _baseline(case, dev)
    gouts = _gouts(case, dev)
    t = _leaves(case, dev)
    outs = case.device(dev, t)
    part = torch.autograd.grad(outs, [t[k] for k in case.groups[0]], gouts, retain_graph=True)
    for k, g in zip(case.groups[0], part):
        _bitwise(g, base_grads[k], f"{name}: d{k} of the partial backward")
    _backward(outs, gouts)
    grads = _grads(t)
    for k in case.diff:
        _bitwise(grads[k], base_grads[k], f"{name}: d{k} of the full backward after a partial one")
    _against_reference(case, tuple(o.detach() for o in outs), grads)


@pytest.mark.parametrize("name", ["pna_stack3_lifted", "pna_conv_stack3_lifted"])
def test_full_backward_after_an_interrupted_one(dev, monkeypatch, name):
    """A hook on the middle layer's output raises once: the backward stops after the last layer has handed out the shared buffer.  The
    next full backward must still be right."""
    case = ac.get(name)
    _setup(case, monkeypatch)
    _, base_grads = _baseline(case, dev)
    gouts = _gouts(case, dev)
    t = _leaves(case, dev)
    outs = case.device(dev, t)
    state = {"raise": True}

    class Interrupted(RuntimeError):
        pass

    def hook(g):
        if state["raise"]:
            state["raise"] = False
            raise Interrupted("interrupted on purpose")
        return g

    outs[1].register_hook(hook)
    with pytest.raises(Interrupted):
        _backward(outs, gouts, retain=True)
    for v in t.values():
        v.grad = None
    _backward(outs, gouts)
    grads = _grads(t)
    for k in case.diff:
        _bitwise(grads[k], base_grads[k], f"{name}: d{k} after an interrupted backward")
    _against_reference(case, tuple(o.detach() for o in outs), grads)


# ---- 7. stale forward state ----------------------------------------------------------------------------------------------------------------
# autograd's refusals of a backward through data that was edited in place: a saved tensor's version moved on; a view made inside
# Function.forward (the flattened attention) whose base was edited; an identity output (pass-through) whose base was edited
_VERSION_ERRORS = ("modified by an inplace operation", "has been modified inplace")


@pytest.mark.parametrize("name", _names("stale"))
def test_inplace_edit_of_an_input_before_backward(dev, monkeypatch, name):
    """An input edited in place between forward and backward: autograd's version error, or the gradients of the forward's values -- never
    those of the edited data."""
    case = ac.get(name)
    _setup(case, monkeypatch)
    _, base_grads = _baseline(case, dev)
    gouts = _gouts(case, dev)
    for k in case.diff:
        t = _leaves(case, dev)
        outs = case.device(dev, t)
        try:
            with torch.no_grad():
                t[k].mul_(0.5).add_(0.25)
            _backward(outs, gouts)
        except RuntimeError as e:
            assert any(m in str(e) for m in _VERSION_ERRORS), e
            continue
        for n in case.diff:
            _bitwise(t[n].grad, base_grads[n], f"{name}: d{n} after {k} was edited in place (no version error raised)")


def test_embedding_sum_index_edited_before_backward(dev):
    """The categorical features are saved through save_for_backward: an in-place edit before the backward raises instead of building the
    one-hot matrix -- and dW -- from indices the forward never saw."""
    from dp_gsat_amd.ops import EmbeddingSum
    case = ac.get("embedding_sum")
    _, base_grads = _baseline(case, dev)
    x_idx = ac.embedding_idx().to(dev)
    W = case.inputs["W"].to(dev).requires_grad_(True)
    cache = {}
    out = EmbeddingSum.apply(x_idx, W, list(ac.EMB_DIMS), cache)
    x_idx[:, 0] = (x_idx[:, 0] + 1) % ac.EMB_DIMS[0]
    try:
        out.backward(_gouts(case, dev)[0])
    except RuntimeError as e:
        assert any(m in str(e) for m in _VERSION_ERRORS), e
    else:
        _bitwise(W.grad, base_grads["W"], "dW after x_idx was edited in place (no version error raised)")


def test_device_counts_and_seeds_stay_live_between_forward_and_backward(dev):
    """m_valid, g_valid, r_dev and seed_dev are read again by the backward ON PURPOSE: a replayed step rewrites those words between
    replays, and forward and backward of one replay see the same value.  Pinned as it is: editing the word between forward and backward
    changes the backward -- the gradient follows the new count (zero beyond it, 1 / count inside), the new r, the new seed."""
    from dp_gsat_amd.dual_gsat import f1_sparsity_loss_valid
    from dp_gsat_amd.get_model import criterion_valid
    from dp_gsat_amd.ops import BatchNormFn, InfoLoss
    from oracle import ops as oops
    g = torch.Generator().manual_seed(5)
    M, m0, m1 = 500, 500, 320
    a0 = torch.rand(M, 1, generator=g) * 0.9 + 0.05

    def info(edit):
        a = a0.to(dev).requires_grad_(True)
        mv = torch.tensor([m0], dtype=torch.int32, device=dev)
        rd = torch.tensor([0.7], dtype=torch.float32, device=dev)
        loss = InfoLoss.apply(a, 0.7, mv, rd)
        if edit == "count":
            mv.fill_(m1)
        if edit == "r":
            rd.fill_(0.5)
        loss.backward()
        return a.grad

    plain, count, r = info(None), info("count"), info("r")
    for m, r_, got in ((m0, 0.7, plain), (m1, 0.7, count), (m0, 0.5, r)):
        ref = {}
        for dt in (torch.float32, torch.float64):
            a = a0.detach().to(dt).clone().requires_grad_(True)
            oops.info_loss(a[:m], r_).backward()
            ref[dt] = a.grad
        close(got, ref[torch.float32], TOL, ref64=ref[torch.float64], what=f"info loss gradient under count {m}, r {r_}")
    assert float(count[m1:].abs().max()) == 0.0 and float(plain[m1:].abs().max()) > 0.0 and not torch.equal(r, plain)

    p0, y0 = torch.rand(M, generator=g), (torch.rand(M, generator=g) > 0.6).float()
    z0, t0 = torch.randn(40, 3, generator=g), torch.randint(0, 3, (40,), generator=g).float()
    for what, fn, x0, cnt0, cnt1 in (("f1 sparsity", lambda x, c: f1_sparsity_loss_valid(x, y0.to(dev), c), p0, M, 320),
                                     ("criterion", lambda x, c: criterion_valid(x, t0.to(dev), 3, False, c), z0, 40, 25)):
        res = []
        for edit in (False, True):
            x = x0.to(dev).requires_grad_(True)
            c = torch.tensor([cnt0], dtype=torch.int32, device=dev)
            loss = fn(x, c)
            if edit:
                c.fill_(cnt1)
            loss.backward()
            res.append(x.grad)
        # the entries beyond the edited count lose their gradient; inside it the sums the forward saved still scale the gradient
        assert float(res[1][cnt1:].abs().max()) == 0.0 and float(res[0][cnt1:].abs().max()) > 0.0, what

    case = ac.get("bn_train_relu_residual_dropout")
    res = []
    for edit in (False, True):
        t = _leaves(case, dev)
        sd = torch.tensor([ac.BN_SEED], dtype=torch.int64, device=dev)
        C = t["x"].shape[1]
        y = BatchNormFn.apply(t["x"], t["weight"], t["bias"], torch.zeros(C, device=dev), torch.ones(C, device=dev), True, ac.BN_MOMENTUM,
                              ac.BN_EPS, True, t["residual"], ac.BN_P, 0, sd, None)
        if edit:
            sd.add_(1)
        y.backward(_gouts(case, dev)[0])
        res.append((y.detach(), t["residual"].grad))
    _bitwise(res[0][0], _baseline(case, dev)[0][0], "BatchNorm tail: device seed word vs host seed")
    _bitwise(res[0][1], _baseline(case, dev)[1]["residual"], "BatchNorm tail: d residual under the device seed word")
    _bitwise(res[1][0], res[0][0], "BatchNorm tail: the forward ran before the seed word was edited")
    assert not torch.equal(res[0][1] != 0, res[1][1] != 0), "the backward did not follow the edited seed word"


# ---- 8. grad mode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("grad_mode"))
def test_forward_without_grad_equals_the_grad_mode_forward(dev, monkeypatch, name):
    case = ac.get(name)
    _setup(case, monkeypatch)
    base_outs, _ = _baseline(case, dev)
    for mode in (torch.no_grad, torch.inference_mode):
        t = _leaves(case, dev)
        with mode():
            outs = case.device(dev, t)
        assert all(not o.requires_grad for o in outs)
        for a, b in zip(outs, base_outs):
            assert torch.equal(a, b), f"{name}: forward under {mode.__name__}"


def test_relu_dropout_with_p_one_is_zero(dev):
    """F.dropout(relu(x), 1.0) of the reference: zeros, and a zero gradient (the library's 1 / (1 - p) has no such case)."""
    from dp_gsat_amd.ops import relu_dropout
    x = torch.randn(300, 16, device=dev).requires_grad_(True)
    y = relu_dropout(x, 1.0, True)
    assert y.shape == x.shape and y.dtype == x.dtype and float(y.detach().abs().max()) == 0.0
    y.backward(torch.randn_like(y))
    assert x.grad is not None and float(x.grad.abs().max()) == 0.0
    ref = torch.nn.functional.dropout(torch.relu(x.detach()), 1.0, training=True)
    assert torch.equal(y.detach(), ref)
    assert torch.equal(relu_dropout(x.detach(), 1.0, False), torch.relu(x.detach()))          # eval: p plays no part


# ---- wrong dtypes and CPU tensors ----------------------------------------------------------------------------------------------------------
_REFUSED = ["sum_att", "pna_edge_twopass", "pna_node_lifted", "pna_conv_edge", "extractor_node", "extractor_edge_streamed",
            "concrete_sample_train", "gumbel_sigmoid_seed", "lift", "symmetrise_host_flag", "info_loss_scalar_prior", "f1_sparsity_all",
            "criterion_ce", "instance_norm", "embedding_sum", "bn_train_relu_residual", "relu_dropout_seeded", "linear_own_gemm",
            "segment_pool_mean"]
# linear(), relu_dropout() and pna_conv() document another path for anything that is not a 2-D fp32 ROCm tensor (torch; the two-op layer):
# linear's Function is called directly, the relu_dropout entry already does, and pna_conv is not fed a CPU tensor


@pytest.mark.parametrize("name", _REFUSED)
def test_wrong_dtype_and_cpu_tensors_raise_before_any_launch(dev, monkeypatch, name):
    from dp_gsat_amd import _lib
    from dp_gsat_amd import ops
    case = ac.get(name)
    _setup(case, monkeypatch)
    _baseline(case, dev)                                      # index caches, workspaces: nothing below needs a launch to get started
    first = case.diff[0]
    for what, convert, error in (("fp64", lambda v: v.double(), TypeError), ("bf16", lambda v: v.bfloat16(), TypeError),
                                 ("cpu", lambda v: v.cpu(), (_lib.GsatHipError, TypeError))):
        if what == "cpu" and name.startswith("pna_conv"):
            continue
        t = {k: v.detach() for k, v in _leaves(case, dev).items()}
        t[first] = convert(t[first])
        if name == "linear_own_gemm":
            run = lambda: ops.LinearFn.apply(t["x"], t["weight"], t["bias"])
        else:
            run = lambda: case.device(dev, t)
        launched, real = [], _lib.call
        with monkeypatch.context() as m:
            m.setattr("dp_gsat_amd.ops.call", lambda fn, *a: (launched.append(fn), real(fn, *a))[1])
            with pytest.raises(error):
                run()
        kernels = [fn for fn in launched if not fn.endswith(("_bytes", "_floats"))]
        assert not kernels, f"{name}: {what} input reached {kernels}"
