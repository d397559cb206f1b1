"""-m gpu: whole GSAT steps under the freezes of fine-tuning and post-hoc explanation -- classifier frozen, extractor frozen, classifier in
eval mode (BatchNorm on its running statistics) while gradients flow to the extractor -- against the fp64 oracle model under the same
freeze, by the rule of tests/test_gpu_models.py.  The model-level part of the autograd contract suite (tests/test_gpu_autograd_contract.py):
these are the needs_input_grad branches of the wrappers as a training script reaches them."""
import copy
from types import SimpleNamespace as NS

import pytest
import torch

from oracle import modules as om
from oracle import ops as oops
from tests.test_gpu_models import _mk_pair
from tests.util import close

pytestmark = pytest.mark.gpu

SETTINGS = ("classifier_frozen", "extractor_frozen", "classifier_eval")

# What the inputs must satisfy, checked on the fp64 oracle alone before anything is compared.  The extractor's InstanceNorm divides by the
# per-graph sigma of every channel and a ReLU follows; the kernels' pre-activations carry a few 1e-7 of rounding (K <= 128 term fp32 sums
# of O(1) values), multiplied by 1 / sigma.  A normalised pre-activation closer to 0 than that may get another sign on the GPU than in
# fp64, and one such element moves whole rows of the weight gradients by 1e-3 (seen: ba_2motifs seed 3 with the classifier in eval mode).
# Such inputs test nothing (tests/extractor_cases.py, RELU_MARGIN): every batch here keeps 1 / sigma <= MAX_INV_SIGMA and every non-zero
# normalised pre-activation at least RELU_MARGIN_PER_INV_SIGMA / sigma away from 0.
# The PNA layers' std aggregator has the same problem in its own backward (1 / sigma of the messages of a row): the operator tests weigh
# the affected entries by tests/test_gpu_pna.py's std_conditioning; a whole-model comparison cannot, so its batch must need no weight
# above 1 (kappa <= 1e3 in every row of every layer).
MAX_INV_SIGMA = 50.0
RELU_MARGIN_PER_INV_SIGMA = 4e-7
MAX_STD_WEIGHT = 1.0
# No molecule batch meets that: two-neighbour rows with nearly equal messages are everywhere (the synthetic molhiv batches of seeds 5..12
# need weights of 240 to 800 in their worst setting).  The PNA test takes the best-conditioned of those seeds -- seed 10, weight 241 on the
# fp64 oracle -- and asserts that bound instead; its comparison is test_gpu_models.py's (the slack term carries the conditioning).
MOLHIV_STD_WEIGHT = 250.0


def _apply(setting, gsat, clf, ext):
    gsat.train()
    if setting == "classifier_frozen":
        for p in clf.parameters():
            p.requires_grad_(False)
    elif setting == "extractor_frozen":
        for p in ext.parameters():
            p.requires_grad_(False)
    else:
        clf.eval()


def _conditioning_spy(seen):
    """oracle.ops.instance_norm that also records (largest 1 / sigma, smallest non-zero |output|) of every call."""
    real = oops.instance_norm

    def spy(x, seg, num_seg, eps=1e-5):
        out = real(x, seg, num_seg, eps)
        n = oops.seg_count(seg, num_seg, x.dtype).clamp_(min=1).view(-1, 1)
        xc = x - (oops.scatter_sum(x, seg, num_seg) / n).index_select(0, seg)
        var = oops.scatter_sum(xc * xc, seg, num_seg) / n
        o = out.detach()
        seen.append((float((var.detach() + eps).rsqrt().max()), float(o[o != 0].abs().min())))
        return out
    return spy


def _std_conditioning_spy(seen):
    """oracle.ops.pna_aggregate that also records the largest conditioning weight of its std aggregator's gradient."""
    from tests.test_gpu_pna import std_conditioning
    real = oops.pna_aggregate

    def spy(x, edge_index, edge_atten, *args, **kwargs):
        w_dx, w_e = std_conditioning(x.detach(), edge_index, None if edge_atten is None else edge_atten.detach(), x.shape[0])
        seen.append(max(float(w_dx.max()), float(w_e.max())))
        return real(x, edge_index, edge_atten, *args, **kwargs)
    return spy


def _oracle(data, oclf, oext, H, learn_edge_att, setting, monkeypatch, epoch, max_std_weight=MAX_STD_WEIGHT):
    """(u, masks, fp32 reference, fp64 reference) of one step under ``setting``; asserts the conditioning rule on the fp64 evaluation."""
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():            # running statistics as training leaves them (30 steps at momentum 0.1): eval mode must read them
        warm = copy.deepcopy(oclf).double().train()          # (in fp64: the same statistics on every host)
        for _ in range(30):
            warm.get_emb(data.x.double() if data.x.is_floating_point() else data.x, data.edge_index, batch=data.batch, edge_attr=None)
        oclf.load_state_dict(warm.state_dict())
    assert any(float(b.abs().max()) > 0.01 for k, b in oclf.named_buffers() if k.endswith("running_mean"))
    M = data.edge_index.shape[1] if learn_edge_att else data.x.shape[0]
    C1 = 4 * H if learn_edge_att else 2 * H
    u = torch.rand(M, 1, generator=g).clamp_(1e-10, 1 - 1e-10)
    masks = [(torch.rand(M, C1, generator=g) > 0.5).float(), (torch.rand(M, H, generator=g) > 0.5).float()]
    oclf64, oext64 = copy.deepcopy(oclf).double(), copy.deepcopy(oext).double()
    d64 = NS(x=data.x.double() if data.x.is_floating_point() else data.x, edge_index=data.edge_index, batch=data.batch, edge_attr=None,
             y=data.y.double() if data.y.is_floating_point() else data.y)
    ref = []
    for c_, e_, d_, cast in ((oclf, oext, data, lambda t: t), (oclf64, oext64, d64, lambda t: t.double())):
        og = om.GSAT(c_, e_, om.Criterion(2, False), learn_edge_att=learn_edge_att)
        _apply(setting, og, c_, e_)
        seen_norms, seen_std = [], []
        with monkeypatch.context() as m:
            m.setattr(oops, "instance_norm", _conditioning_spy(seen_norms))
            m.setattr(oops, "pna_aggregate", _std_conditioning_spy(seen_std))
            o_att, o_loss, o_ld, o_logits, _ = og.forward_pass(d_, epoch, True, u=cast(u), masks=[cast(m_) for m_ in masks])
        if c_ is oclf64:
            inv_sigma, margin = max(a for a, _ in seen_norms), min(b for _, b in seen_norms)
            assert len(seen_norms) == 2 and inv_sigma <= MAX_INV_SIGMA and margin >= RELU_MARGIN_PER_INV_SIGMA * inv_sigma, \
                f"ill-conditioned inputs: 1/sigma {inv_sigma:.1f}, closest pre-activation {margin:.2e}"
            assert max(seen_std, default=1.0) <= max_std_weight, f"ill-conditioned inputs: std weight {max(seen_std, default=1.0):.2f}"
        o_loss.backward()
        ref.append(NS(att=o_att.detach(), loss=o_loss.detach(), logits=o_logits.detach(), ld=o_ld,
                      params=list(c_.named_parameters()) + list(e_.named_parameters())))
    return u, masks, ref[0], ref[1]


def _run(G, data, backbone, cfg, x_dim, H, learn_edge_att, dev, setting, monkeypatch, epoch=12, max_std_weight=MAX_STD_WEIGHT):
    oclf, oext, clf, ext = _mk_pair(G, backbone, cfg, x_dim, 0, H, learn_edge_att, dev)
    u, masks, r32, r64 = _oracle(data, oclf, oext, H, learn_edge_att, setting, monkeypatch, epoch, max_std_weight)
    clf.load_state_dict(oclf.state_dict())
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), None, learn_edge_att=learn_edge_att)
    _apply(setting, gsat, clf, ext)
    for p, (_, q) in zip(list(clf.parameters()) + list(ext.parameters()), r32.params):
        p.requires_grad_(q.requires_grad)
    att, loss, ld, logits = gsat.forward_pass(data.to(dev), epoch, True, noise=u.to(dev), dropout_masks=[m.to(dev) for m in masks])
    loss.backward()
    close(att, r32.att, ref64=r64.att, what="edge_att")
    close(logits, r32.logits, ref64=r64.logits, what="clf_logits")
    close(loss, r32.loss, ref64=r64.loss, what="loss")
    for k in ("loss", "pred", "info"):
        assert abs(ld[k] - r32.ld[k]) <= 1e-4 * max(1.0, abs(r32.ld[k])), (k, ld[k], r32.ld[k])
    seen = 0
    for (k, p), (_, q), (_, q64) in zip(list(clf.named_parameters()) + list(ext.named_parameters()), r32.params, r64.params):
        assert p.requires_grad == q.requires_grad
        if not q.requires_grad:
            assert p.grad is None and q.grad is None, f"{k} is frozen"
            continue
        if q.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, f"grad {k} is missing"
        close(p.grad, q.grad, 1e-4, ref64=q64.grad, what="grad " + k)
        seen += 1
    assert seen > 0
    if setting == "classifier_eval":
        for (k, b), (_, ob) in zip(clf.named_buffers(), oclf.named_buffers()):
            close(b.float(), ob.float(), 1e-6, what="buffer " + k)                 # eval mode moved no running statistic


@pytest.mark.parametrize("setting", SETTINGS)
def test_gin_edge_attention_under_freezes(dev, monkeypatch, setting):
    """ba_2motifs seed 7: the first of 3, 4, 5, ... whose batch meets the conditioning rule above in all three settings."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    data = synth.ba2motifs_batch(num_graphs=12, seed=7)
    H = 32
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=H, dropout_p=0.0)
    _run(G, data, "GIN", cfg, 10, H, True, dev, setting, monkeypatch)


@pytest.mark.parametrize("setting", SETTINGS)
def test_pna_node_attention_under_freezes(dev, monkeypatch, setting):
    """H = 64: the layers form the lifted node attention inside their kernels and share one d node_att buffer."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    monkeypatch.setattr("dp_gsat_amd.graph_index._HUBS_SEEN", [False])
    data = synth.molhiv_batch(num_graphs=12, seed=10)
    H = 64
    cfg = dict(model_name="PNA", n_layers=3, hidden_size=H, dropout_p=0.0, use_edge_attr=False, atom_encoder=True,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=synth.in_degree_histogram(data))
    _run(G, data, "PNA", cfg, 9, H, False, dev, setting, monkeypatch, max_std_weight=MOLHIV_STD_WEIGHT)
