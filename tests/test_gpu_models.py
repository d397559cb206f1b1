"""-m gpu: whole backbones and the GSAT step (example/trainer.py:28-36 row) vs the oracle and the committed goldens."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import modules as om
from tests.test_oracle_golden import build_oracle, load_case
from tests.util import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mk_pair(G, backbone, cfg, x_dim, e_dim, H, learn_edge_att, dev, num_class=2):
    oclf = {"GIN": om.GIN, "PNA": om.PNA, "SPMotifNet": om.SPMotifNet}[backbone](x_dim, e_dim, num_class, False, cfg)
    oext = om.ExtractorMLP(H, learn_edge_att)
    clf = G.get_model(x_dim, e_dim, num_class, False, cfg, dev)
    clf.load_state_dict(oclf.state_dict())
    ext = G.ExtractorMLP(H, learn_edge_att).to(dev)
    ext.load_state_dict(oext.state_dict())
    return oclf, oext, clf, ext


def _step(G, data, oclf, oext, clf, ext, learn_edge_att, H, dev, training=True, num_class=2, epoch=12):
    M = data.edge_index.shape[1] if learn_edge_att else data.x.shape[0]
    C1 = 4 * H if learn_edge_att else 2 * H
    g = torch.Generator().manual_seed(11)
    u = torch.rand(M, 1, generator=g).clamp_(1e-10, 1 - 1e-10)
    masks = [(torch.rand(M, C1, generator=g) > 0.5).float(), (torch.rand(M, H, generator=g) > 0.5).float()]
    ogsat = om.GSAT(oclf, oext, om.Criterion(num_class, False), learn_edge_att=learn_edge_att).train(training)
    o_att, o_loss, o_ld, o_logits, aux = ogsat.forward_pass(data, epoch, training, u=u, masks=masks)
    gsat = G.GSAT(clf, ext, G.Criterion(num_class, False), None, learn_edge_att=learn_edge_att).train(training)
    att, loss, ld, logits = gsat.forward_pass(data.to(dev), epoch, training, noise=u.to(dev), dropout_masks=[m.to(dev) for m in masks])
    close(att, o_att, what="edge_att")
    close(logits, o_logits, what="clf_logits")
    for k in ("loss", "pred", "info"):
        assert abs(ld[k] - o_ld[k]) <= 1e-4 * max(1.0, abs(o_ld[k])), (k, ld[k], o_ld[k])
    if training:
        o_loss.backward()
        loss.backward()
        # fp64 evaluation of the oracle: gradients are compared with slack for the fp32 oracle's own rounding error
        import copy
        oclf64, oext64 = copy.deepcopy(oclf).double(), copy.deepcopy(oext).double()
        for m in (oclf64, oext64):
            for p_ in m.parameters():
                p_.grad = None
        d64 = NS(x=data.x.double() if data.x.is_floating_point() else data.x, edge_index=data.edge_index, batch=data.batch,
                 edge_attr=None if data.edge_attr is None else data.edge_attr.double(), y=data.y.double() if data.y.is_floating_point() else data.y)
        og64 = om.GSAT(oclf64, oext64, om.Criterion(num_class, False), learn_edge_att=learn_edge_att).train(True)
        _, l64, _, _, _ = og64.forward_pass(d64, epoch, True, u=u.double(), masks=[m.double() for m in masks])
        l64.backward()
        for (k, p), (_, q), (_, q64) in zip(list(clf.named_parameters()) + list(ext.named_parameters()),
                                            list(oclf.named_parameters()) + list(oext.named_parameters()),
                                            list(oclf64.named_parameters()) + list(oext64.named_parameters())):
            if q.grad is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
                continue
            close(p.grad, q.grad, 1e-4, ref64=q64.grad, what="grad " + k)


@pytest.mark.parametrize("training", [True, False])
def test_gsat_gin_edge_attention_c2(dev, training):
    """C2: ba_2motifs + GIN, hidden 64, edge attention, symmetrised."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.ba2motifs_batch(num_graphs=24, seed=3)
    H = 64
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=H, dropout_p=0.0)
    pair = _mk_pair(G, "GIN", cfg, 10, 0, H, True, dev)
    _step(G, data, *pair, True, H, dev, training)


def test_gsat_gin_node_attention_c1_mutag(dev):
    """C1: real MUTAG topology (fixture) + GIN hidden 64, node attention (lift)."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.mutag_batch(os.path.join(ROOT, "tests", "golden", "mutag128.npz"), num_graphs=32)
    H = 64
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=H, dropout_p=0.0)
    pair = _mk_pair(G, "GIN", cfg, 14, 0, H, False, dev)
    _step(G, data, *pair, False, H, dev, True)


def test_gsat_pna_node_attention_c3(dev):
    """C3: molhiv-shaped + PNA (mean,min,max,std; identity), atom encoder, node attention."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.molhiv_batch(num_graphs=24, seed=5)
    H = 32
    cfg = dict(model_name="PNA", n_layers=3, hidden_size=H, dropout_p=0.0, use_edge_attr=False, atom_encoder=True,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=synth.in_degree_histogram(data))
    pair = _mk_pair(G, "PNA", cfg, 9, 0, H, False, dev)
    _step(G, data, *pair, False, H, dev, True)


def test_gsat_gine_directed_c4(dev):
    """C4: spmotif-shaped, single-direction edges (no symmetrisation), edge_attr = ones -> GINEConv, 3 classes."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.spmotif_batch(num_graphs=16, seed=7)
    H = 32
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=H, dropout_p=0.0)
    pair = _mk_pair(G, "GIN", cfg, 4, 1, H, True, dev, num_class=3)
    assert type(pair[2].convs[0]).__name__ == "GINEConv"
    _step(G, data, *pair, True, H, dev, True, num_class=3)


@pytest.mark.parametrize("name,backbone,edge", [("gin_edge", "GIN", True), ("pna_node", "PNA", False)])
def test_against_committed_golden(dev, name, backbone, edge):
    """train_one_batch row of SURVEY 8c: emb, att_log_logits, att, edge_att, clf_logits, loss dict, parameter grads."""
    import dp_gsat_amd as G
    c = load_case(name)
    cfg, oclf, oext = build_oracle(c, backbone, edge)
    H = 16
    clf = G.get_model(5, 0, 2, False, cfg, dev)
    clf.load_state_dict(oclf.state_dict())
    ext = G.ExtractorMLP(H, edge).to(dev)
    ext.load_state_dict(oext.state_dict())
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), None, learn_edge_att=edge).train()
    data = NS(x=c["x"].to(dev), edge_index=c["edge_index"].to(dev), batch=c["batch"].to(dev), edge_attr=None, y=c["y"].to(dev))
    emb = clf.get_emb(data.x, data.edge_index, batch=data.batch, edge_attr=None)
    close(emb, c["emb"], what="emb")
    z, att = ext.attend(emb, data.edge_index, data.batch, noise=c["u"].to(dev), dropout_masks=[c["mask1"].to(dev), c["mask2"].to(dev)])
    close(z, c["att_log_logits"], what="att_log_logits")
    close(att, c["att"], what="att")
    edge_att, loss, ld, logits = gsat.forward_pass(data, 12, True, noise=c["u"].to(dev),
                                                   dropout_masks=[c["mask1"].to(dev), c["mask2"].to(dev)])
    close(edge_att, c["edge_att"], what="edge_att")
    close(logits, c["clf_logits"], what="clf_logits")
    assert abs(ld["loss"] - c["loss"].item()) < 1e-4 and abs(ld["info"] - c["info"].item()) < 1e-4
    loss.backward()
    for k, p in ext.named_parameters():
        close(p.grad, c["grad.ext." + k], 1e-4, what="grad ext." + k)
    for k, p in clf.named_parameters():
        close(p.grad, c["grad.clf." + k], 1e-4, what="grad clf." + k)


def test_backbone_dropout_and_unmasked_call_forms(dev):
    """keyword call without edge_atten (src/pretrain_clf.py:61,69), get_pred_from_emb(emb, batch), dropout active in train."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.ba2motifs_batch(num_graphs=6, seed=1).to(dev)
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=32, dropout_p=0.3)
    clf = G.get_model(10, 0, 2, False, cfg, dev).eval()
    a = clf(data.x, edge_index=data.edge_index, edge_attr=None, batch=data.batch)
    emb = clf.get_emb(data.x, data.edge_index, batch=data.batch, edge_attr=None)
    b = clf.get_pred_from_emb(emb, data.batch)
    assert a.shape == (6, 1) and torch.allclose(a, b, atol=1e-5)
    clf.train()
    e1 = clf.get_emb(data.x, data.edge_index, batch=data.batch)
    assert (e1 == 0).float().mean() > 0.25                 # relu + dropout(0.3) zeros


def test_deterministic_bitwise(dev):
    """Run the same step twice: every output and gradient is bit-identical (no float atomics anywhere)."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.molhiv_batch(num_graphs=16, seed=2).to(dev)
    H = 32
    cfg = dict(model_name="PNA", n_layers=2, hidden_size=H, dropout_p=0.0, use_edge_attr=False, atom_encoder=True,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=synth.in_degree_histogram(data))
    clf = G.get_model(9, 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(H, False).to(dev)
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), None, learn_edge_att=False).train()
    u = torch.rand(data.num_nodes, 1, device=dev).clamp_(1e-10, 1 - 1e-10)
    outs = []
    for _ in range(2):
        for p in gsat.parameters():
            p.grad = None
        G.clear_cache()
        torch.manual_seed(123)                       # same Philox dropout seed for both runs
        att, loss, _, logits = gsat.forward_pass(data, 3, True, noise=u)
        loss.backward()
        outs.append([att.clone(), logits.clone(), loss.clone()] + [p.grad.clone() for p in gsat.parameters() if p.grad is not None])
    assert len(outs[0]) == len(outs[1]) > 10
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_atom_bond_encoders(dev):
    """ogb AtomEncoder / BondEncoder: gather forward, one-hot GEMM backward vs nn.Embedding sums."""
    import dp_gsat_amd as G
    from dp_gsat_amd.encoders import AtomEncoder, BondEncoder, ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS
    g = torch.Generator().manual_seed(0)
    for Enc, OEnc, dims, n in ((AtomEncoder, om.AtomEncoder, ATOM_FEATURE_DIMS, 5000), (BondEncoder, om.BondEncoder, BOND_FEATURE_DIMS, 777)):
        H = 80
        x = torch.stack([torch.randint(0, d, (n,), generator=g) for d in dims], dim=1)
        go = torch.randn(n, H, generator=g)
        oe = OEnc(H)
        oo = oe(x); oo.backward(go)
        e = Enc(H).to(dev); e.load_state_dict(oe.state_dict())
        assert list(e.state_dict()) == list(oe.state_dict())
        xd = x.to(dev)
        out = e(xd); out.backward(go.to(dev))
        close(out, oo, 1e-5)
        for (k, p), (_, q) in zip(e.named_parameters(), oe.named_parameters()):
            close(p.grad, q.grad, what=k)
        out2 = e(xd); out2.backward(go.to(dev))           # second step reuses the cached one-hot matrix
        close(list(e.parameters())[0].grad, 2 * list(oe.parameters())[0].grad)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("training", [True, False])
def test_batchnorm_kernels(dev, relu, training):
    from dp_gsat_amd.encoders import BatchNorm1d
    g = torch.Generator().manual_seed(3)
    N, C = 3001, 80
    x = torch.randn(N, C, generator=g) * 2 + 0.5
    go = torch.randn(N, C, generator=g)
    ref = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        ref.weight.uniform_(0.5, 1.5, generator=g); ref.bias.normal_(generator=g)
        ref.running_mean.normal_(generator=g); ref.running_var.uniform_(0.5, 2.0, generator=g)
    mine = BatchNorm1d(C).to(dev); mine.load_state_dict(ref.state_dict())
    ref.train(training); mine.train(training)
    xo = x.clone().requires_grad_(True)
    yo = ref(xo); yo = torch.relu(yo) if relu else yo
    yo.backward(go)
    xd = x.to(dev).requires_grad_(True)
    yd = mine(xd, fused_relu=relu); yd.backward(go.to(dev))
    close(yd, yo); close(xd.grad, xo.grad)
    close(mine.weight.grad, ref.weight.grad); close(mine.bias.grad, ref.bias.grad)
    close(mine.running_mean, ref.running_mean, 1e-5); close(mine.running_var, ref.running_var, 1e-5)
    assert int(mine.num_batches_tracked) == int(ref.num_batches_tracked)


def test_gsat_spmotifnet_leconv(dev):
    """src/configs/SPMotifNet-spmotif.yml: LEConv backbone, hidden 32, edge attention on directed spmotif graphs,
    edge_attr = ones passed as edge_weight."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.spmotif_batch(num_graphs=12, seed=3)
    H = 32
    cfg = dict(model_name="SPMotifNet", n_layers=2, hidden_size=H)
    pair = _mk_pair(G, "SPMotifNet", cfg, 4, 1, H, True, dev, num_class=3)
    assert list(pair[2].state_dict()) == list(pair[0].state_dict())
    _step(G, data, *pair, True, H, dev, True, num_class=3)


def test_hipgraph_capture_of_a_training_step(dev):
    """Sync-free mode: a whole GSAT step (index build, extractor with device-seeded Philox dropout, symmetrise with the
    device flag, masked backbone, backward) is captured into a hipGraph and replayed; replays draw new dropout masks and
    the first replay reproduces the eager result for the same seed word."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.ba2motifs_batch(num_graphs=16, seed=2).to(dev)
    H = 32
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=H, dropout_p=0.0)
    clf = G.get_model(10, 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(H, True).to(dev)
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), None, learn_edge_att=True).train()
    gsat.sync_loss_dict = False
    params = [p for p in gsat.parameters()]
    out = {}

    def step():
        G.clear_cache()
        for p in params:
            p.grad = None
        att, loss, _, logits = gsat.forward_pass(data, 0, True)
        loss.backward()
        out["att"], out["loss"], out["g"] = att, loss, ext.mlp.linears()[0].weight.grad

    G.set_sync_free(True)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(side)
        from tests.util import assert_no_memset_nodes, capture_with_dump
        graph, dot = capture_with_dump(step)
        assert_no_memset_nodes(dot, "captured GSAT training step")       # neither libgsat_hip nor the torch ops of the step may add one
        from dp_gsat_amd.ops import device_seed_state
        state0 = device_seed_state(dev).clone()
        res = []
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            res.append((out["att"].clone(), out["loss"].clone(), out["g"].clone()))
        # the first replay reproduces the eager result for the same seed word: rewind the device seed stream, run the step eagerly
        device_seed_state(dev).copy_(state0)
        step()
        torch.cuda.synchronize()
        for what, x, y in zip(("att", "loss", "grad W1"), (out["att"], out["loss"], out["g"]), res[0]):
            assert torch.equal(x, y), f"eager step != first replay: {what}"
    finally:
        G.set_sync_free(False)
    for att, loss, g in res:
        assert torch.isfinite(att).all() and torch.isfinite(loss) and torch.isfinite(g).all()
        assert att.shape == (data.num_edges, 1) and float(g.abs().max()) > 0
        index = G.get_index(data.edge_index, data.num_nodes)
        assert torch.equal(att[:, 0], att[index.rev.long(), 0])          # symmetrised inside the graph (device flag)
    assert not torch.equal(res[0][0], res[1][0])                           # new noise / dropout masks per replay


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("training", [True, False])
def test_batchnorm_fused_layer_tail(dev, p, training):
    """y = dropout(relu(BN(x)) + residual) in the BatchNorm kernels (src/models/pna.py:57-59); the Philox mask is read back
    through gsat_philox_keep_mask (stream 3) and applied explicitly on the torch side."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.ops import BatchNormFn
    g = torch.Generator().manual_seed(4)
    N, C, seed = 2050, 64, 987654321
    x = torch.randn(N, C, generator=g) * 1.5 - 0.2
    res = torch.randn(N, C, generator=g)
    go = torch.randn(N, C, generator=g)
    ref = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        ref.weight.uniform_(0.5, 1.5, generator=g); ref.bias.normal_(generator=g)
        ref.running_mean.normal_(generator=g); ref.running_var.uniform_(0.5, 2.0, generator=g)
    ref.train(training)
    keep = torch.ones(N, C, device=dev)
    if p > 0:
        call("gsat_philox_keep_mask", seed, 3, N, C, p, ptr(keep), stream())
        frac = float(keep.mean())
        assert abs(frac - (1 - p)) < 0.01, frac
    xo, ro = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    yo = (torch.relu(ref(xo)) + ro) * keep.cpu() / (1 - p)
    yo.backward(go)
    w, b = ref.weight.detach().clone().to(dev).requires_grad_(True), ref.bias.detach().clone().to(dev).requires_grad_(True)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    rm.copy_(torch.nn.BatchNorm1d(C).running_mean if training else ref.running_mean); rv.copy_(torch.nn.BatchNorm1d(C).running_var if training else ref.running_var)
    xd, rd = x.to(dev).requires_grad_(True), res.to(dev).requires_grad_(True)
    yd = BatchNormFn.apply(xd, w, b, rm, rv, training, 0.1, 1e-5, True, rd, p, seed, None)
    yd.backward(go.to(dev))
    close(yd, yo); close(xd.grad, xo.grad); close(rd.grad, ro.grad)
    close(w.grad, ref.weight.grad); close(b.grad, ref.bias.grad)
    # device-resident seed word (hipGraph mode) draws the same mask as the by-value seed
    sd = torch.tensor([seed], dtype=torch.int64, device=dev)
    yd2 = BatchNormFn.apply(x.to(dev), w.detach(), b.detach(), rm.clone(), rv.clone(), training, 0.1, 1e-5, True, res.to(dev), p, 0, sd)
    assert torch.equal(yd2, yd.detach()) or training     # training mode moved the running stats only; outputs still equal
    close(yd2, yd.detach(), 1e-6)


def test_colsum_matches_torch(dev):
    from dp_gsat_amd.ops import colsum
    g = torch.Generator().manual_seed(8)
    for R, C in [(1, 4), (63, 128), (51639, 128), (1000, 1)]:
        x = torch.randn(R, C, generator=g)
        close(colsum(x.to(dev)), x.double().sum(0).float(), 1e-5)


@pytest.mark.parametrize("backbone,edge", [("GIN", False), ("PNA", True)])
def test_training_trajectory_matches_oracle(dev, backbone, edge):
    """example/trainer.py:28-36 repeated: forward_pass, zero_grad, backward, Adam -- 25 steps on the real MUTAG topology (fixture),
    same noise / keep-masks on both sides.  The HIP stack and the CPU oracle must follow the same loss trajectory (the notebook's
    sanity band, SURVEY 8c: the loss goes down) within fp32 drift."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.mutag_batch(os.path.join(ROOT, "tests", "golden", "mutag128.npz"), num_graphs=64)
    H, steps = 32, 25
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=0.0, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=synth.in_degree_histogram(data))
    oclf, oext, clf, ext = _mk_pair(G, backbone, cfg, 14, 0, H, edge, dev)
    ogsat = om.GSAT(oclf, oext, om.Criterion(2, False), learn_edge_att=edge).train()
    oopt = torch.optim.Adam(list(oclf.parameters()) + list(oext.parameters()), lr=1e-3, weight_decay=3e-6)
    opt = torch.optim.Adam(list(clf.parameters()) + list(ext.parameters()), lr=1e-3, weight_decay=3e-6)
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), opt, learn_edge_att=edge).train()
    M = data.edge_index.shape[1] if edge else data.x.shape[0]
    C1 = 4 * H if edge else 2 * H
    ones = [torch.ones(M, C1), torch.ones(M, H)]
    ddev = data.to(dev)
    g = torch.Generator().manual_seed(21)
    ref_losses, got_losses = [], []
    for step in range(steps):
        u = torch.rand(M, 1, generator=g).clamp_(1e-10, 1 - 1e-10)
        _, ol, old, _, _ = ogsat.forward_pass(data, step, True, u=u, masks=ones)
        oopt.zero_grad(); ol.backward(); oopt.step()
        _, l, ld, _ = gsat.forward_pass(ddev, step, True, noise=u.to(dev), dropout_masks=[m.to(dev) for m in ones])
        opt.zero_grad(); l.backward(); opt.step()
        ref_losses.append(old["loss"]); got_losses.append(ld["loss"])
    for i, (a, b) in enumerate(zip(got_losses, ref_losses)):
        assert abs(a - b) <= 2e-2 * max(1.0, abs(b)), (i, a, b)
    assert got_losses[-1] < 0.9 * got_losses[0], got_losses          # it learns
    for (k, p), (_, q) in zip(list(clf.named_parameters()) + list(ext.named_parameters()),
                              list(oclf.named_parameters()) + list(oext.named_parameters())):
        assert torch.isfinite(p).all(), k
        assert float((p.detach().cpu() - q.detach()).abs().max()) <= 5e-2 * max(1.0, float(q.detach().abs().max())), k


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_relu_dropout_tail(dev, p):
    """GIN layer tail (src/models/gin.py:50-51) in one launch: relu, Bernoulli(1 - p) keep mask scaled by 1 / (1 - p), backward from y."""
    from dp_gsat_amd.ops import relu_dropout
    x = torch.randn(3001, 64, device=dev).requires_grad_(True)
    y = relu_dropout(x, p, True)
    r = torch.relu(x.detach())
    pos = r > 0
    keep = (y > 0)[pos].float().mean().item()
    assert abs(keep - (1 - p)) < 0.02
    s = 1.0 / (1.0 - p)
    assert torch.allclose(y[y > 0], (r * s)[y > 0], rtol=1e-6, atol=0) and bool((y[~pos] == 0).all())
    go = torch.randn_like(y)
    y.backward(go)
    assert torch.allclose(x.grad, torch.where(y > 0, go * s, torch.zeros_like(go)), rtol=1e-6, atol=0)
    assert torch.equal(relu_dropout(x.detach(), p, False), r)          # eval: plain relu
