"""-m gpu: fixed-capacity batches -- the padded collation bit-exact against tests/padded_oracle.py, the count-aware BatchNorm and info
loss against fp64, one captured training step replayed on several real batches against the oracle on the UNPADDED batch, and the eager
padded step.  Floating-point comparisons follow tests.util.close (TOL = 1e-4, fp64 evaluation as ref64)."""
import copy
import math
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import modules as om
from oracle import ops as oops
from tests import padded_oracle as po
from tests.replay import SeedRecorder, philox_inputs, pin_seed_stream, seed_state
from tests.util import TOL, assert_no_memset_nodes, close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_BASE = 0x5EED


# ---- 1. layout ---------------------------------------------------------------------------------------------------------------------------
def _layout_dataset(dev):
    import dp_gsat_amd as G
    graphs = po.mutag_graphs(**po.LAYOUT_GRAPHS)
    gen = torch.Generator().manual_seed(3)
    for g in graphs:                                   # edge features and labels that are nowhere zero: padding slots must be
        e = g.edge_index.shape[1]
        g.edge_attr = torch.rand(e, 2, generator=gen) + 1.0
        g.edge_label = torch.ones(e)
    return graphs, G.PackedDataset.from_data_list(graphs, dev)


@pytest.mark.parametrize("case", ["tight", "odd_self_loop", "duplicated", "wide"])
def test_collate_padded_layout_is_bit_exact(dev, case):
    graphs, ds = _layout_dataset(dev)
    cap = po.layout_cases()[case]
    ids = torch.tensor(po.LAYOUT_IDS, device=dev)
    want = po.collate_padded(graphs, po.LAYOUT_IDS, cap)
    b = ds.collate_padded(ids, cap)
    u = ds.collate(ids)
    N, E = u.x.shape[0], u.edge_index.shape[1]
    assert b.valid.dtype == torch.int32 and b.valid.tolist() == want["valid"].tolist() == [N, E, 5, 0]
    assert b.num_graphs == 6 and b.capacity == cap
    assert b.x.shape == (cap[0], 14) and b.edge_index.shape == (2, cap[1]) and b.batch.shape == (cap[0],) and b.y.shape == (6, 1)
    assert b.edge_attr.shape == (cap[1], 2) and b.edge_label.shape == (cap[1],)
    for name in ("batch", "node_src_row", "edge_index", "edge_src_slot"):
        assert np.array_equal(getattr(b, name).cpu().numpy(), want[name]), name
    # the real part is collate's, bit for bit; the padding is zero
    assert torch.equal(b.x[:N], u.x) and torch.equal(b.edge_index[:, :E], u.edge_index) and torch.equal(b.batch[:N], u.batch)
    assert torch.equal(b.y[:5], u.y) and torch.equal(b.edge_attr[:E], u.edge_attr) and torch.equal(b.edge_label[:E], u.edge_label)
    assert not b.x[N:].any() and not b.edge_attr[E:].any() and not b.edge_label[E:].any() and not b.y[5:].any()
    po.check_invariants({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in vars(b).items()
                         if k in want}, cap)


def test_collate_padded_categorical_and_overflow(dev):
    import dp_gsat_amd as G
    graphs, ds = _layout_dataset(dev)
    ids = torch.tensor(po.LAYOUT_IDS, device=dev)
    N, E = po.totals(graphs, po.LAYOUT_IDS)
    cat = G.PackedDataset.from_data_list([NS(x=g.x.argmax(1, keepdim=True) + 1, edge_index=g.edge_index, y=g.y, edge_attr=None, edge_label=None)
                                          for g in graphs], dev)
    b = cat.collate_padded(ids, (N + 4, E + 3))
    assert b.x.dtype == torch.int64 and int(b.x[:N].min()) >= 1 and not b.x[N:].any() and b.edge_attr is None
    for cap in [(N + 1, E), (N + 2, E - 1)]:
        with pytest.raises(ValueError, match="does not fit"):
            ds.collate_padded(ids, cap)
        G.set_sync_free(True)
        try:
            b = ds.collate_padded(ids, cap)             # nothing is read back: the flag is set and the batch is all padding
        finally:
            G.set_sync_free(False)
        want = po.collate_padded(graphs, po.LAYOUT_IDS, cap)
        assert b.valid.tolist() == [0, 0, 5, 1]
        assert b.x.shape == (cap[0], 14) and b.edge_index.shape == (2, cap[1]) and b.edge_attr.shape == (cap[1], 2) and b.y.shape == (6, 1)
        for name in ("batch", "node_src_row", "edge_index", "edge_src_slot"):
            assert np.array_equal(getattr(b, name).cpu().numpy(), want[name]), name
        assert not b.x.any() and not b.edge_attr.any()


# ---- 2. BatchNorm over the first n_valid rows ----------------------------------------------------------------------------------------------
BN_ROWS = 200                                # row_blocks(200): 4 blocks of 50 rows
BN_COUNTS = [0, 2, 37, 50, 51, 199, 200]     # none (an overflow batch), inside the first block (the others empty), on a block edge,
                                             # one past it, the last row, all
BN_SEED, BN_P = 0x1234_5678_9ABC, 0.3


def _bn_case(dev, C, n, fused):
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.ops import BatchNormFn
    g = torch.Generator().manual_seed(1000 * C + n)
    N = BN_ROWS
    x = torch.randn(N, C, generator=g) * 2 + 0.5
    dy = torch.randn(N, C, generator=g)
    res = torch.randn(N, C, generator=g)
    x[n:], dy[n:] = 1e4, 1e4                  # a padding row that is counted cannot hide
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    momentum, eps = 0.1, 1e-5
    keep = torch.ones(N, C)
    if fused:
        kd = torch.empty(N, C, device=dev)
        call("gsat_philox_keep_mask", BN_SEED, 3, N, C, BN_P, ptr(kd), stream())
        keep = kd.cpu()
        assert 0.5 < float(keep.mean()) < 0.9
    if n == 0:
        _bn_empty(dev, x, dy, res, gamma, beta, rm0, rv0, fused)
        return
    # fp64 reference on the counted rows alone
    x64 = x[:n].double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    r64 = res[:n].double().requires_grad_(True)
    rm64, rv64 = rm0.double().clone(), rv0.double().clone()
    y64 = torch.nn.functional.batch_norm(x64, rm64, rv64, g64, b64, True, momentum, eps)
    if fused:
        y64 = (torch.relu(y64) + r64) * keep[:n].double() / (1 - BN_P)
    y64.backward(dy[:n].double())
    mean64 = x[:n].double().mean(0)
    rstd64 = 1.0 / torch.sqrt(x[:n].double().var(0, unbiased=False) + eps)

    xd = x.to(dev).requires_grad_(True)
    gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    rd = res.to(dev).requires_grad_(True) if fused else None
    rm, rv = rm0.to(dev), rv0.to(dev)
    nv = torch.tensor([n], dtype=torch.int32, device=dev)
    y = BatchNormFn.apply(xd, gd, bd, rm, rv, True, momentum, eps, fused, rd, BN_P if fused else 0.0, BN_SEED, None, nv)
    mean, rstd = y.grad_fn.saved_tensors[3:5]
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    what = f"C={C} n_valid={n} fused={fused}: "
    assert torch.isfinite(y).all(), what + "padding rows of y must stay finite"
    close(y[:n], y64, TOL, what=what + "y")
    close(mean, mean64, TOL, what=what + "mean")
    close(rstd, rstd64, TOL, what=what + "rstd")
    close(rm, rm64, TOL, what=what + "running_mean")
    close(rv, rv64, TOL, what=what + "running_var")
    close(xd.grad[:n], x64.grad, TOL, what=what + "dx")
    close(gd.grad, g64.grad, TOL, what=what + "dgamma")
    close(bd.grad, b64.grad, TOL, what=what + "dbeta")
    assert not xd.grad[n:].any(), what + "dx of padding rows must be exactly 0"
    if fused:
        close(rd.grad[:n], r64.grad, TOL, what=what + "dresidual")
        assert not rd.grad[n:].any(), what + "dresidual of padding rows must be exactly 0"


def _bn_empty(dev, x, dy, res, gamma, beta, rm0, rv0, fused):
    """A count of 0 (the all-padding batch of an overflow): the divisors are clamped to 1, so everything stays finite; no row is counted,
    so every gradient is exactly 0."""
    from dp_gsat_amd.ops import BatchNormFn
    xd = x.to(dev).requires_grad_(True)
    gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    rd = res.to(dev).requires_grad_(True) if fused else None
    rm, rv = rm0.to(dev), rv0.to(dev)
    nv = torch.zeros(1, dtype=torch.int32, device=dev)
    y = BatchNormFn.apply(xd, gd, bd, rm, rv, True, 0.1, 1e-5, fused, rd, BN_P if fused else 0.0, BN_SEED, None, nv)
    mean, rstd = y.grad_fn.saved_tensors[3:5]
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    for name, t in (("y", y), ("mean", mean), ("rstd", rstd), ("running_mean", rm), ("running_var", rv)):
        assert torch.isfinite(t).all(), f"n_valid=0 fused={fused}: {name} is not finite"
    assert not mean.any()
    close(rm, 0.9 * rm0, 1e-6, what="running_mean after an empty batch")
    close(rv, 0.9 * rv0, 1e-6, what="running_var after an empty batch")
    assert not xd.grad.any() and not gd.grad.any() and not bd.grad.any()
    if fused:
        assert not rd.grad.any()


def run_bn_plain_cases():
    """Every plain case; also the entry of the child process that takes the two-pass statistics path."""
    dev = torch.device("cuda:0")
    for C in (8, 68):
        for n in BN_COUNTS:
            _bn_case(dev, C, n, False)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "relu-residual-dropout"])
@pytest.mark.parametrize("C", [8, 68])
def test_batchnorm_counts_valid_rows_only(dev, C, fused):
    for n in BN_COUNTS:
        _bn_case(dev, C, n, fused)


def test_batchnorm_valid_rows_two_pass_statistics(dev):
    """GSAT_BN_ONE_PASS is read once per process: the two-pass path runs in one fresh child."""
    env = dict(os.environ, GSAT_BN_ONE_PASS="0")
    out = subprocess.run([sys.executable, "-c", "from tests.test_gpu_padded import run_bn_plain_cases; run_bn_plain_cases(); print('two-pass ok')"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0 and "two-pass ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ---- 3. info loss over the first m_valid entries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_mode", ["scalar", "r_dev", "tensor_prior"])
@pytest.mark.parametrize("m", [0, 1, 257, 1500])
def test_info_loss_counts_valid_entries_only(dev, m, r_mode):
    from dp_gsat_amd.ops import InfoLoss
    M = 1500
    g = torch.Generator().manual_seed(m)
    att = torch.rand(M, 1, generator=g) * 0.96 + 0.02
    edge = torch.tensor([0.5, 1e-7, 1.0 - 1e-7, 0.0, 1.0]).repeat(M // 5 + 1)[:M].view(M, 1)
    att[m:] = edge[m:]                                       # padding entries at 0.5 and next to (and at) 0 and 1
    gout = 1.7
    r32 = float(np.float32(0.6))
    prior = torch.rand(M, 1, generator=g) * 0.8 + 0.1
    a64 = att[:m].double().requires_grad_(True)
    if m:
        ref = oops.info_loss(a64, prior[:m].double() if r_mode == "tensor_prior" else r32)
        (ref * gout).backward()
    else:                                                    # an overflow batch: the divisor is clamped to 1, the empty sum is 0
        ref, a64.grad = torch.zeros((), dtype=torch.float64), torch.zeros_like(a64)
    ad = att.to(dev).requires_grad_(True)
    mv = torch.tensor([m], dtype=torch.int32, device=dev)
    if r_mode == "scalar":
        out = InfoLoss.apply(ad, r32, mv, None)
    elif r_mode == "r_dev":
        out = InfoLoss.apply(ad, 0.9, mv, torch.tensor([r32], device=dev))          # the device float overrides the scalar
    else:
        out = InfoLoss.apply(ad, prior.to(dev), mv, None)
    (out * gout).backward()
    torch.cuda.synchronize()
    assert m or float(out) == 0.0
    close(out, ref, TOL, what="info loss")
    close(ad.grad[:m], a64.grad, TOL, what="datt")
    assert not ad.grad[m:].any(), "datt of padding entries must be exactly 0"
    assert torch.isfinite(ad.grad).all()


# ---- 4. / 5. whole steps ---------------------------------------------------------------------------------------------------------------------
def _adam64(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=3e-6):
    """torch.optim.Adam's update (L2 weight decay, bias-corrected) in fp64, from the pre-step parameter and state."""
    p, g, m, v = (x.detach().cpu().double() for x in (p, g, m, v))
    g = g + wd * p
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    return p - lr / (1 - betas[0] ** t) * m / (v.sqrt() / math.sqrt(1 - betas[1] ** t) + eps)


H = 32


def _models(dev, backbone, edge, graphs):
    import dp_gsat_amd as G
    deg = torch.bincount(torch.cat([torch.bincount(g.edge_index[1], minlength=g.x.shape[0]) for g in graphs]), minlength=10)
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=0.0, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=deg)
    oclf = {"GIN": om.GIN, "PNA": om.PNA}[backbone](14, 0, 2, False, cfg)
    oext = om.ExtractorMLP(H, edge)
    clf = G.get_model(14, 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(H, edge).to(dev)
    return cfg, oclf, oext, clf, ext


def _oracle_step(oclf, oext, clf_sd, ext_sd, ub, edge, epoch, u, masks, decay_interval):
    """The oracle's GSAT step on the unpadded batch ``ub`` (CPU) from the given state, in fp32 and fp64:
    dt -> (edge_att, loss, clf_logits, gradients, the backbone's state_dict after the step's two forwards)."""
    runs = {}
    for dt in (torch.float32, torch.float64):
        oc, oe = copy.deepcopy(oclf), copy.deepcopy(oext)
        oc.load_state_dict(clf_sd)
        oe.load_state_dict(ext_sd)
        oc, oe = oc.to(dt), oe.to(dt)
        d = NS(x=ub.x.to(dt), edge_index=ub.edge_index, batch=ub.batch, edge_attr=None, y=ub.y.to(dt))
        og = om.GSAT(oc, oe, om.Criterion(2, False), learn_edge_att=edge, decay_interval=decay_interval).train()
        att, loss, _, logits, _ = og.forward_pass(d, epoch, True, u=u.to(dt), masks=[m.to(dt) for m in masks])
        loss.backward()
        runs[dt] = (att.detach(), loss.detach(), logits.detach(), [p.grad for p in list(oc.parameters()) + list(oe.parameters())],
                    {k: v.detach().clone() for k, v in oc.state_dict().items()})
    return runs[torch.float32], runs[torch.float64]


def _check_step(got_att, got_loss, got_logits, params, names, clf, r32, r64, E, B, what):
    (a32, l32, z32, g32, s32), (a64, l64, z64, g64, s64) = r32, r64
    close(got_loss.reshape(()), l32.reshape(()), TOL, ref64=l64.reshape(()), what=what + "loss")
    close(got_att[:E], a32, TOL, ref64=a64, what=what + "edge_att")
    close(got_logits[:B], z32, TOL, ref64=z64, what=what + "clf_logits")
    for n, p, q32, q64 in zip(names, params, g32, g64):
        if q32 is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        close(p.grad, q32, TOL, ref64=q64, what=what + "grad " + n)
    sd = clf.state_dict()
    stats = [k for k in sd if "running_" in k]
    assert stats
    for k in stats:                                          # statistics over the real rows only, updated by both forwards of the step
        close(sd[k], s32[k], TOL, ref64=s64[k], what=what + k)
    for k in sd:
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(s32[k]), k


@pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])
def test_one_captured_graph_replays_real_batches(dev, backbone, edge):
    """ReplayedStep's graph, captured once, replayed for three id sets of different (N_real, E_real) at epochs 0, 1, 2 (decay_interval 1:
    r changes between replays).  After each replay the Philox inputs are regenerated at capacity size from the recorded seed word and
    sliced to the real rows, and the oracle's step on the unpadded batch from the pre-step state gives the reference for loss, attention,
    every gradient and the BatchNorm running statistics; the parameters after the step against fp64 Adam."""
    import dp_gsat_amd as G
    graphs = po.mutag_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    cfg, oclf, oext, clf, ext = _models(dev, backbone, edge, graphs)
    params = list(clf.parameters()) + list(ext.parameters())
    names = [n for n, _ in clf.named_parameters()] + ["ext." + n for n, _ in ext.named_parameters()]
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-6, capturable=True, fused=True)
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), opt, learn_edge_att=edge, decay_interval=1).train()
    before = [p.detach().clone() for p in params]
    graph = torch.cuda.CUDAGraph()
    try:
        graph.enable_debug_mode()
    except Exception:
        pass
    with SeedRecorder() as rec:
        rs = G.ReplayedStep(gsat, ds, po.STEP_BATCH, keep_edge_att=True, graph=graph)
    assert not G.graph_index.sync_free() and gsat.sync_loss_dict
    for p, p0 in zip(params, before):                        # capturing (three warm-up steps) did not train
        assert torch.equal(p, p0)
    text = None
    try:
        path = os.path.join(tempfile.mkdtemp(), "graph.dot")
        graph.debug_dump(path)
        if os.path.exists(path) and os.path.getsize(path) > 0:
            text = open(path, errors="replace").read()
    except Exception:
        text = None
    assert_no_memset_nodes(text, "ReplayedStep")
    pin_seed_stream(dev, STREAM_BASE)
    N_cap, E_cap = cap = ds.capacity_for(po.STEP_BATCH)
    assert rs.capacity == cap
    B = po.STEP_BATCH
    M_cap = E_cap if edge else N_cap
    for epoch, ids in enumerate(po.STEP_IDS):
        N, E = po.totals(graphs, ids)
        clf_sd = {k: v.detach().clone().cpu() for k, v in clf.state_dict().items()}
        ext_sd = {k: v.detach().clone().cpu() for k, v in ext.state_dict().items()}
        pre = [p.detach().clone() for p in params]
        st = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), float(opt.state[p]["step"])) for p in params]
        assert st[0][2] == epoch
        base, counter = seed_state(dev)
        loss = rs.step(np.asarray(ids), epoch)
        torch.cuda.synchronize()
        (word,) = rec.check(base, counter)
        assert rs.batch.valid.tolist() == [N, E, B, 0]
        assert rs.edge_att.shape == (E_cap, 1) and rs.clf_logits.shape == (B + 1, 1) and rs.batch.x.shape == (N_cap, 14)
        assert abs(float(rs.r) - G.get_r(1, 0.1, epoch, final_r=0.7)) < 1e-6
        ub = ds.collate(torch.tensor(ids, device=dev)).to("cpu")
        assert ub.x.shape[0] == N and ub.edge_index.shape[1] == E
        M = E if edge else N
        masks, u = philox_inputs(word, M_cap, 4 * H if edge else 2 * H, H, 0.5, dev)
        r32, r64 = _oracle_step(oclf, oext, clf_sd, ext_sd, ub, edge, epoch, u[:M], [m[:M] for m in masks], 1)
        what = f"replay {epoch}: "
        _check_step(rs.edge_att, loss, rs.clf_logits, params, names, clf, r32, r64, E, B, what)
        for n, p, q32, p0, (m, v, t) in zip(names, params, r32[3], pre, st):
            if q32 is not None:
                close(p, _adam64(p0, p.grad, m, v, t + 1), 1e-6, what=what + "adam " + n)
    G.clear_cache()


@pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])
def test_eager_padded_step_matches_unpadded(dev, backbone, edge):
    """The padded step without capture (explicit noise and masks of capacity size, the real rows' slices for the reference), next to the
    eager unpadded step, both against the oracle; and padded() used directly around the backbone."""
    import dp_gsat_amd as G
    graphs = po.mutag_graphs(**po.STEP_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    cfg, oclf, oext, clf, ext = _models(dev, backbone, edge, graphs)
    params = list(clf.parameters()) + list(ext.parameters())
    names = [n for n, _ in clf.named_parameters()] + ["ext." + n for n, _ in ext.named_parameters()]
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), None, learn_edge_att=edge).train()
    ids = po.STEP_IDS[1]
    B = len(ids)
    N, E = po.totals(graphs, ids)
    N_cap, E_cap = cap = ds.capacity_for(B)
    M_cap, M = (E_cap, E) if edge else (N_cap, N)
    g = torch.Generator().manual_seed(11)
    u = torch.rand(M_cap, 1, generator=g).clamp_(1e-10, 1 - 1e-10)
    masks = [(torch.rand(M_cap, 4 * H if edge else 2 * H, generator=g) > 0.5).float(), (torch.rand(M_cap, H, generator=g) > 0.5).float()]
    clf_sd = {k: v.detach().clone().cpu() for k, v in clf.state_dict().items()}
    ext_sd = {k: v.detach().clone().cpu() for k, v in ext.state_dict().items()}
    idt = torch.tensor(ids, device=dev)
    ub = ds.collate(idt)
    r32, r64 = _oracle_step(oclf, oext, clf_sd, ext_sd, ub.to("cpu"), edge, 0, u[:M], [m[:M] for m in masks], 10)
    for padded in (True, False):
        clf.load_state_dict(clf_sd)
        for p in params:
            p.grad = None
        b = ds.collate_padded(idt, cap) if padded else ub
        rows = M_cap if padded else M
        att, loss, ld, logits = gsat.forward_pass(b, 0, True, noise=u[:rows].to(dev), dropout_masks=[m[:rows].to(dev) for m in masks])
        loss.backward()
        torch.cuda.synchronize()
        att = G.ops.edge_tensor(att)
        if padded:
            assert att.shape == (E_cap, 1) and logits.shape == (B + 1, 1) and torch.isfinite(logits).all()
        assert abs(ld["loss"] - float(r64[1])) < 1e-3
        _check_step(att, loss, logits, params, names, clf, r32, r64, E, B, "padded: " if padded else "unpadded: ")
    # padded() directly around the backbone: batch statistics of the real rows only
    clf.load_state_dict(clf_sd)
    b = ds.collate_padded(idt, cap)
    with G.padded(b.valid, b.capacity):
        z = clf(b.x, b.edge_index, b.batch, edge_attr=None)
    assert G.current_padding() is None
    refs = []
    for dt in (torch.float32, torch.float64):
        oc = copy.deepcopy(oclf)
        oc.load_state_dict(clf_sd)
        oc = oc.to(dt).train()
        c = ub.to("cpu")
        refs.append(oc(c.x.to(dt), c.edge_index, c.batch, None).detach())
    close(z[:B], refs[0], TOL, ref64=refs[1], what="clf inside padded()")
    G.clear_cache()


def test_replayed_step_reports_overflow_and_restores_on_failure(dev):
    """A capacity that graphs 0..B-1 do not fit: the constructor raises after its warm-up runs and leaves the model untrained.  A step whose
    batch does not fit a (tight) capacity is not skipped; overflowed() tells, once, that it happened."""
    import dp_gsat_amd as G
    graphs = po.mutag_graphs(**po.LAYOUT_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    cfg, _, _, clf, ext = _models(dev, "GIN", True, graphs)
    params = list(clf.parameters()) + list(ext.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, capturable=True, fused=True)
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), opt, learn_edge_att=True).train()
    before = {k: v.detach().clone() for k, v in gsat.state_dict().items()}
    N, E = po.totals(graphs, range(5))
    with pytest.raises(ValueError, match="do not fit"):
        G.ReplayedStep(gsat, ds, 5, capacity=(N + 1, E))
    for k, v in gsat.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not G.graph_index.sync_free() and gsat.sync_loss_dict
    rs = G.ReplayedStep(gsat, ds, 5, capacity=(N + 2, E))
    assert not rs.overflowed()
    rs.step([0, 1, 2, 3, 4], 0)
    assert rs.batch.valid.tolist() == [N, E, 5, 0] and not rs.overflowed()
    big = [0, 1, 2, 6, 7]
    assert po.totals(graphs, big)[0] > N
    with pytest.raises(ValueError, match="capacity"):
        rs.check_epoch(big)
    rs.step(big, 0)
    assert rs.batch.valid.tolist() == [0, 0, 5, 1] and torch.isfinite(rs.loss)
    rs.step([0, 1, 2, 3, 4], 0)
    assert rs.overflowed() and not rs.overflowed()
    G.clear_cache()


def test_padded_batches_are_refused_where_unsupported(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd.encoders import BatchNorm1d
    graphs = po.mutag_graphs(**po.LAYOUT_GRAPHS)
    ds = G.PackedDataset.from_data_list(graphs, dev)
    b = ds.collate_padded(torch.tensor(po.LAYOUT_IDS, device=dev), ds.capacity_for(5))
    cfg, _, _, clf, ext = _models(dev, "GIN", True, graphs)
    with pytest.raises(ValueError, match="multi-label"):
        G.GSAT(clf, ext, G.Criterion(2, True), None, learn_edge_att=True).train().forward_pass(b, 0, True)
    bn = BatchNorm1d(8).to(dev).train()
    bn.sync_group = True
    with G.padded(b.valid):
        with pytest.raises(ValueError, match="sync_group"):
            bn(torch.randn(b.x.shape[0], 8, device=dev))
    shared = {"learn_edge_att": False, "extractor_dropout_p": 0.5}
    mcfg = dict(pred_loss_coef=1, info_loss_coef=1, fix_r=False, decay_interval=10, decay_r=0.1, final_r=0.5)
    dual = G.DualGSAT(clf, G.ExtractorMLP(H, shared, "primal").to(dev), None, clf, G.ExtractorMLP(H, shared, "dual").to(dev), None,
                      mcfg, mcfg, False, False)
    with pytest.raises(ValueError, match="padded"):
        dual.dual_forward_pass(b, b, 0, True)
    with pytest.raises(ValueError, match="capturable"):
        G.ReplayedStep(G.GSAT(clf, ext, G.Criterion(2, False), torch.optim.Adam(clf.parameters()), learn_edge_att=True), ds, 5)
    G.clear_cache()
