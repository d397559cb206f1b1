"""-m gpu: the memory-bounded extractor through the public API -- ``ExtractorMLP.stream_rows`` against the same module without it, one
GSAT step both ways, every refusal, and the memory it exists to save."""
import copy
from types import SimpleNamespace as NS

import pytest
import torch

from oracle import modules as om
from tests import extractor_cases as ec
from tests import extractor_oracle as eo
from tests.graphs import shuffle_edges
from tests.util import TOL, close

pytestmark = pytest.mark.gpu
KEYS = [f"feature_extractor.{i}.{p}" for i in (0, 4, 8) for p in ("weight", "bias")]
GRADS = dict(zip(KEYS, ("dW1", "db1", "dW2", "db2", "dW3", "db3")))


def _extractor(dev, case, stream_rows, edge_mode=True):
    import dp_gsat_amd as G
    ext = G.ExtractorMLP(case["H"], edge_mode, stream_rows=stream_rows).to(dev)
    if edge_mode:
        ext.load_state_dict(dict(zip(KEYS, case["params"])))
    return ext.train(case["training"])


def _attend(dev, ext, case, ei=None):
    ext.zero_grad(set_to_none=True)
    e = case["emb"].to(dev).clone().requires_grad_(True)
    M = case["M"]
    z, a = ext.attend(e, (case["ei"] if ei is None else ei).to(dev), case["batch"].to(dev), noise=case["u"].to(dev).view(M, 1),
                      dropout_masks=[m.to(dev) for m in case["masks"]])
    torch.autograd.backward([z, a], [case["dlogits"].to(dev).view(M, 1), case["datt"].to(dev).view(M, 1)])
    return dict(logits=z.detach().view(-1), att=a.detach().view(-1), demb=e.grad, **{GRADS[k]: p.grad.clone() for k, p in ext.named_parameters()})


def test_streamed_module_against_the_unstreamed_one(dev):
    """stream_rows = 64 (eight groups) against None: same weights, masks and noise; the fp64 reference as ref64."""
    case = ec.make_case("regular", "boundaries", True, 16, True, sorted_edges=True)
    _, r64 = eo.references(case)
    staged = _attend(dev, _extractor(dev, case, None), case)
    ext = _extractor(dev, case, None)
    ext.stream_rows = 64                                      # the attribute form
    streamed = _attend(dev, ext, case)
    for k in ("logits", "att", "demb") + tuple(GRADS.values()):
        close(streamed[k].reshape(r64[k].shape), staged[k].reshape(r64[k].shape), TOL, ref64=r64[k], what=k)
    kw = _attend(dev, _extractor(dev, case, 64), case)        # the keyword form: the same plan, the same bits
    for k in streamed:
        assert torch.equal(kw[k], streamed[k]), k
    # the DP-GSAT constructor form takes the keyword too
    import dp_gsat_amd as G
    dp = G.ExtractorMLP(16, dict(learn_edge_att=True, extractor_dropout_p=0.5), "primal", stream_rows=64)
    assert dp.stream_rows == 64 and G.ExtractorMLP(16, True).stream_rows is None


def test_one_gsat_step_both_ways(dev):
    """GSAT.forward_pass + backward on a GIN edge-attention model with and without stream_rows: loss and every parameter gradient."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    from tests.test_gpu_models import _mk_pair
    data = synth.ba2motifs_batch(num_graphs=12, seed=3)
    H = 32
    cfg = dict(model_name="GIN", n_layers=2, hidden_size=H, dropout_p=0.0)
    oclf, oext, clf, ext = _mk_pair(G, "GIN", cfg, 10, 0, H, True, dev)
    M = data.edge_index.shape[1]
    g = torch.Generator().manual_seed(11)
    u = torch.rand(M, 1, generator=g).clamp_(1e-10, 1 - 1e-10)
    masks = [(torch.rand(M, 4 * H, generator=g) > 0.5).float(), (torch.rand(M, H, generator=g) > 0.5).float()]
    oclf64, oext64 = copy.deepcopy(oclf).double(), copy.deepcopy(oext).double()
    d64 = NS(x=data.x.double() if data.x.is_floating_point() else data.x, edge_index=data.edge_index, batch=data.batch, edge_attr=None, y=data.y)
    og64 = om.GSAT(oclf64, oext64, om.Criterion(2, False), learn_edge_att=True).train(True)
    _, l64, _, _, _ = og64.forward_pass(d64, 12, True, u=u.double(), masks=[m.double() for m in masks])
    l64.backward()
    ddev = data.to(dev)
    runs = {}
    for rows in (None, 60):
        ext.stream_rows = rows
        gsat = G.GSAT(clf, ext, G.Criterion(2, False), None, learn_edge_att=True).train(True)
        clf.zero_grad(set_to_none=True)
        ext.zero_grad(set_to_none=True)
        _, loss, _, _ = gsat.forward_pass(ddev, 12, True, noise=u.to(dev), dropout_masks=[m.to(dev) for m in masks])
        loss.backward()
        runs[rows] = (loss.detach().clone(), {k: p.grad.clone() for k, p in list(clf.named_parameters()) + list(ext.named_parameters()) if p.grad is not None})
    close(runs[60][0], runs[None][0], TOL, ref64=l64.detach(), what="loss")
    ref = dict(list(oclf64.named_parameters()) + list(oext64.named_parameters()))
    assert set(runs[60][1]) == set(runs[None][1])
    for k, gr in runs[60][1].items():
        close(gr, runs[None][1][k], TOL, ref64=ref[k].grad, what="grad " + k)


def test_every_refusal_and_none_changes_nothing(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd.graph_index import set_sync_free
    from dp_gsat_amd.ops import ExtractorAttention
    from tests.extractor_driver import run
    case = ec.make_case("regular", "boundaries", True, 16, True, sorted_edges=True)
    # None: the outputs of the C ABI's default path, bit for bit, and last_forward_kind as that call reports it
    ExtractorAttention.last_forward_kind = -1
    plain = _attend(dev, _extractor(dev, case, None), case)
    want = run(dev, case, fused=0, order="auto")
    assert ExtractorAttention.last_forward_kind == want["paths"]["fwd_kind"] == 0
    for k in ("logits", "att", "demb") + tuple(GRADS.values()):
        assert torch.equal(plain[k].reshape(-1), want[k].reshape(-1)), k
    ext = _extractor(dev, case, 64)
    ExtractorAttention.last_forward_kind = -1
    _attend(dev, ext, case)
    assert ExtractorAttention.last_forward_kind == -1, "the streamed call reports no forward kind of the default paths"
    # refusals
    node = ec.make_case("regular", "boundaries", False, 16, True)
    with pytest.raises(ValueError, match="edge-attention"):
        _attend(dev, _extractor(dev, node, 64, edge_mode=False), node)
    with pytest.raises(ValueError, match="edge order"):
        _attend(dev, ext, case, ei=shuffle_edges(case["ei"], 3))
    cross = case["ei"].clone()
    cross[1, 0] = int((case["batch"] == 2).nonzero()[0])
    with pytest.raises(ValueError, match="between two graphs"):
        _attend(dev, ext, case, ei=cross)
    for bad in (0, -5, 2.5, True):
        with pytest.raises(ValueError, match="stream_rows"):
            _attend(dev, _extractor(dev, case, bad), case)
    set_sync_free(True)
    try:
        with pytest.raises(ValueError, match="set_sync_free"):
            _attend(dev, ext, case)
    finally:
        set_sync_free(False)
    with G.padded(torch.tensor([case["N"], case["M"], case["G"], 0], dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError, match="padded"):
            _attend(dev, ext, case)
    x = torch.zeros(8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x + 1
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    e, eid, bd = case["emb"].to(dev), case["ei"].to(dev), case["batch"].to(dev)
    with torch.cuda.graph(graph):
        y = x + 1                                             # the capture holds one node: the refusal launches nothing
        with pytest.raises(ValueError, match="capture"):
            ext.attend(e, eid, bd)
    graph.replay()
    torch.cuda.synchronize()
    assert bool((y == 1).all())
    _attend(dev, ext, case)                                   # and the module still works afterwards


def test_streaming_saves_the_memory_of_both_activations(dev):
    """8 graphs of 2560 directed edges on 160 nodes, H = 64: M = 20480, C1 = 256, one [M, C1] tensor is 20.97 MB.  Staged holds a1 (saved)
    and da1 (workspace), 2 * M * C1 * 4 bytes; streamed with stream_rows = 2560 holds two scratches of M / 8 rows.  The peak of forward +
    backward above the level before the call must drop by at least ONE [M, C1] tensor (the expected gap is ~36.7 MB and more: the rest is
    room for whatever else differs).  Seen on an MI355X: staged 81.98 MB, streamed 23.41 MB."""
    import dp_gsat_amd as G
    from dp_gsat_amd.ops import ExtractorAttention
    from tests.attn_stream_driver import workspace_bytes
    H, n, deg, graphs = 64, 160, 16, 8
    src = torch.arange(n).repeat_interleave(deg)
    dst = (src + torch.arange(1, deg + 1).repeat(n)) % n
    ei = torch.cat([torch.stack([src, dst]) + g * n for g in range(graphs)], dim=1).to(dev)
    batch = torch.arange(graphs).repeat_interleave(n).to(dev)
    M, C1 = ei.shape[1], 4 * H
    assert (M, C1) == (20480, 256)
    act = M * C1 * 4
    gen = torch.Generator().manual_seed(3)
    emb = torch.randn(graphs * n, H, generator=gen).to(dev)
    gz, ga = torch.randn(M, 1, generator=gen).to(dev), torch.randn(M, 1, generator=gen).to(dev)
    ext = G.ExtractorMLP(H, True).to(dev).train()

    def peak(rows):
        ext.stream_rows = rows
        out = None
        for _ in range(2):                                   # the first pass builds the batch index and the plan
            ext.zero_grad(set_to_none=True)
            e = emb.clone().requires_grad_(True)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            z, a = ext.attend(e, ei, batch, noise="philox", seed=5)
            torch.autograd.backward([z, a], [gz, ga])
            torch.cuda.synchronize()
            out = torch.cuda.max_memory_allocated() - base
            res = (z.detach().clone(), e.grad.clone())
            del z, a, e
        return out, res

    staged, r0 = peak(None)
    assert ExtractorAttention.last_forward_kind == 0, "the default path of this shape is the staged pipeline, which saves a1"
    streamed, r1 = peak(2560)
    assert G.get_index(ei, graphs * n).graphs(batch).stream_plan(2560).n_groups == 8
    print(f"\npeak above the level before the call: staged {staged / 1e6:.2f} MB, streamed {streamed / 1e6:.2f} MB, one [M, C1] tensor {act / 1e6:.2f} MB")
    assert staged - streamed >= act, f"staged {staged} - streamed {streamed} = {staged - streamed} < {act}"
    close(r1[0], r0[0], TOL, what="logits, streamed against staged")          # the same draws: keyed by the global row
    close(r1[1], r0[1], TOL, what="demb, streamed against staged")
    fwd, bwd, gp, scratch = workspace_bytes([2560] * graphs, [n] * graphs, H, 2560)
    assert len(gp) == 9 and scratch == 2560 and fwd < act and bwd < act, (fwd, bwd, act)
