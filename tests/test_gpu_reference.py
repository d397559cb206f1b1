"""-m gpu: the HIP step against recordings of the REFERENCE'S OWN classes (tests/golden/ref_*, oracle/record_reference.py).

The model is built from the recorded ``state_dict``, runs ``forward_pass`` and the backward with the recorded noise and keep-masks, and is
compared by the suite's rule, ``close(actual, fp32 recording, TOL, ref64=fp64 recording)``: both references come from the reference's
code, none from oracle/.  Only the fixtures are read: the reference and the recording stand-in do not exist on a GPU machine."""
import pytest
import torch

from tests import ref_fixtures as rf
from tests.test_extractor_cases_host import SWITCHES
from tests.util import TOL, close

pytestmark = pytest.mark.gpu

STAGED_DEFAULT = dict(fwd_kind=0, bwd_fused=0, bwd_ncht=0, bwd_dual_l2=0, bwd_dual_l1=0, bwd_pair_l2=0, bwd_pair_l1=0, bwd_split=1,
                      bwd_merged=1)          # a few hundred rows: staged forward, split-bf16 merged backward, nothing paired


@pytest.fixture(autouse=True)
def _stop_on_a_hip_error():
    """A HIP error (a kernel fault is sticky) ends the whole run: nothing more is started on a faulted device."""
    from tests.extractor_driver import _sync
    yield
    if torch.cuda.is_available():
        _sync()


def _default_switches(monkeypatch):
    for k in SWITCHES + ("GSAT_PNA_TILED", "GSAT_NODE_ATT_LIFT", "GSAT_NODE_ATT_SHARED_GRAD", "GSAT_PNA_TILE_LDS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr("dp_gsat_amd.graph_index._HUBS_SEEN", [False])


def _build(G, c, dev):
    s = c.s
    clf = G.get_model(s["x_dim"], s["edge_attr_dim"], s["num_class"], s["multi_label"], rf.model_config(c), dev)
    ext = G.ExtractorMLP(s["H"], s["learn_edge_att"]).to(dev)
    assert list(clf.state_dict()) == s["state_keys"]["clf"] and list(ext.state_dict()) == s["state_keys"]["ext"], \
        "the library's state_dict keys are not the reference's"
    clf.load_state_dict(rf.state(c, "clf"))
    ext.load_state_dict(rf.state(c, "ext"))
    gsat = G.GSAT(clf, ext, G.Criterion(s["num_class"], s["multi_label"]), None, learn_edge_att=s["learn_edge_att"])
    return clf, ext, gsat


def _extractor_paths(c, training):
    """What the library says it runs for the extractor call of this case (gsat_attn_paths on the call's extents, library policy)."""
    from dp_gsat_amd._lib import attn_paths
    from tests.extractor_driver import shape_args
    s = c.s
    edge = s["learn_edge_att"]
    case = dict(edge_mode=edge, H=s["H"], M=s["num_edges"] if edge else s["num_nodes"], N=s["num_nodes"], G=s["num_graphs"], training=training)
    p = attn_paths(shape_args(case, 0, edge))
    return {k: p[k] for k in STAGED_DEFAULT}


def _compare_outputs(c, tag, emb, z, att, edge_att, logits, loss, ld):
    r32, r64 = (lambda k: c.a[f"f32.{tag}{k}"]), (lambda k: c.a[f"f64.{tag}{k}"])
    close(emb, r32("emb"), TOL, ref64=r64("emb"), what="emb")
    close(z, r32("att_log_logits"), TOL, ref64=r64("att_log_logits"), what="att_log_logits")
    close(att, r32("att"), TOL, ref64=r64("att"), what="att")
    close(edge_att, r32("edge_att"), TOL, ref64=r64("edge_att"), what="edge_att")
    close(logits, r32("clf_logits"), TOL, ref64=r64("clf_logits"), what="clf_logits")
    close(loss.view(1), r32("loss"), TOL, ref64=r64("loss"), what="loss")
    for k in ("loss", "pred", "info"):
        close(torch.tensor([ld[k]], dtype=torch.float64), r32(k), TOL, ref64=r64(k), what="loss_dict " + k)


@pytest.mark.parametrize("name", rf.case_names())
def test_training_step_equals_the_reference_recording(dev, monkeypatch, name):
    """emb, att_log_logits, att, edge_att, clf_logits, the loss and its parts, and the gradient of every parameter."""
    import dp_gsat_amd as G
    from dp_gsat_amd import ops
    _default_switches(monkeypatch)
    c = rf.load_case(name)
    s = c.s
    clf, ext, gsat = _build(G, c, dev)
    gsat.train()
    data = rf.batch(c).to(dev)
    u, masks = rf.draws(c)
    u, masks = u.to(dev), [m.to(dev) for m in masks]
    assert _extractor_paths(c, True) == STAGED_DEFAULT
    emb = clf.get_emb(data.x, data.edge_index, batch=data.batch, edge_attr=data.edge_attr)
    z, att = ext.attend(emb, data.edge_index, data.batch, noise=u, dropout_masks=masks)
    assert ops.ExtractorAttention.last_forward_kind == 0
    for m in (clf, ext):              # the two calls above are the first half of forward_pass: put the BatchNorm statistics back
        m.zero_grad(set_to_none=True)
    clf.load_state_dict(rf.state(c, "clf"))
    edge_att, loss, ld, logits = gsat.forward_pass(data, s["epoch"], True, noise=u, dropout_masks=masks)
    index = G.get_index(data.edge_index, data.x.shape[0])
    if s["learn_edge_att"]:
        assert isinstance(edge_att, torch.Tensor)
        assert bool(index.is_undirected) == s["undirected"]          # the symmetrise branch ran, or did not
        if s["undirected"]:
            assert torch.equal(edge_att, edge_att[index.rev.long()])
    else:
        assert isinstance(edge_att, ops.LiftedAttention)
        tiled = s["backbone"] == "PNA" and s["H"] >= 64 and s["edge_attr_dim"] == 0
        assert bool(index.pna_tiles(s["H"])) == (s["H"] >= 64), "tile plan"
        # PNA at H >= 64 forms node_att[src] * node_att[dst] inside its kernels: no [E, 1] tensor exists after the forward
        assert (edge_att._edge is None) == tiled
    loss.backward()
    if not s["learn_edge_att"]:
        if tiled:
            assert edge_att._edge is None, "the tiled backward wrote the lifted attention out"
        # the reference callers' own expressions on the returned attention (src/run_gsat.py eval loop, example/trainer.py)
        flat = edge_att.data.cpu().reshape(-1)
        arr = edge_att.detach().cpu().numpy()
        want32, want64 = c.a["f32.edge_att"], c.a["f64.edge_att"]
        close(flat, want32.reshape(-1), TOL, ref64=want64.reshape(-1), what="att.data.cpu().reshape(-1)")
        close(torch.from_numpy(arr), want32, TOL, ref64=want64, what="att.detach().cpu().numpy()")
    _compare_outputs(c, "", emb, z, att, edge_att if s["learn_edge_att"] else edge_att.edge(), logits, loss, ld)
    seen = 0
    for prefix, m in (("clf.", clf), ("ext.", ext)):
        for k, p in m.named_parameters():
            if prefix + k not in c.grad32:                         # the reference gave it no gradient (SPMotifNet's unused heads)
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, prefix + k
                continue
            assert p.grad is not None, f"grad {prefix + k} is missing"
            close(p.grad, c.grad32[prefix + k], TOL, ref64=c.grad64[prefix + k], what="grad " + prefix + k)
            seen += 1
    assert seen == len(c.grad32)


def test_eval_step_equals_the_reference_recording(dev, monkeypatch):
    """gin_edge in eval mode: BatchNorm on the recorded running statistics, no noise, no dropout, symmetrised sigmoid(logits)."""
    import dp_gsat_amd as G
    _default_switches(monkeypatch)
    c = rf.load_case("gin_edge")
    clf, ext, gsat = _build(G, c, dev)
    gsat.eval()
    data = rf.batch(c).to(dev)
    assert _extractor_paths(c, False)["fwd_kind"] == 0
    with torch.no_grad():
        emb = clf.get_emb(data.x, data.edge_index, batch=data.batch, edge_attr=data.edge_attr)
        z, att = ext.attend(emb, data.edge_index, data.batch)
        edge_att, loss, ld, logits = gsat.forward_pass(data, c.s["epoch"], False)
    _compare_outputs(c, "eval.", emb, z, att, edge_att, logits, loss, ld)
    for k, v in rf.state(c, "clf").items():
        assert torch.equal(clf.state_dict()[k].cpu(), v), f"eval mode moved {k}"
