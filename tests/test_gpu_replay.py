"""-m gpu: captured, replayed steps (what bench.py times) against the fp64-checked oracle -- the bench's scope-A step, the step replayed
on batches it was not captured on, a whole training step with fused capturable Adam, and the device seed stream across torch.manual_seed."""
import copy
import math
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import bookkeeping as obk
from oracle import modules as om
from tests.replay import SeedRecorder, capture, fresh_batch, philox_inputs, pin_seed_stream, scope_a_reference, seed_next_ref, seed_state
from tests.util import TOL, close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_BASE = 0x5EED      # every replay test restarts the device seed stream here after capturing


def _snapshot(outputs):
    return {k: v.detach().clone() for k, v in outputs.items()}


def _hot_inputs(hot):
    return dict(emb=hot.emb, xs=hot.xs, ees=hot.edge_emb, gouts=hot.gouts, ext_state=hot.ext.state_dict())


def _check_against_oracle(wl, data, hot_inputs, got, word, dev, skip=()):
    """Regenerate the step's Philox inputs from its seed word and compare every output of the step (but ``skip``) with the oracle in
    fp32 / fp64."""
    H, edge = wl["H"], wl["edge_att"]
    M = data.edge_index.shape[1] if edge else data.batch.shape[0]
    masks, u = philox_inputs(word, M, 4 * H if edge else 2 * H, H, 0.5, dev)
    r32 = scope_a_reference(wl, data, u=u, masks=masks, dtype=torch.float32, **hot_inputs)
    r64 = scope_a_reference(wl, data, u=u, masks=masks, dtype=torch.float64, **hot_inputs)
    missing = set(got) - set(r32)
    assert not missing, f"outputs without a reference: {sorted(missing)}"
    for k, v in got.items():
        if k not in skip:
            close(v, r32[k], TOL, ref64=r64[k], what=k)


def _hot_path(wl_name, data, dev):
    import bench
    wl = dict(bench.WORKLOADS[wl_name], key=wl_name)
    hot = bench.HotPath(wl, data.to(dev), dev, seed=0)
    hot.keep_outputs = True
    return wl, hot


@pytest.mark.parametrize("workload", ["c1", "c2", "c3", "c4"])
def test_replayed_hot_path_matches_oracle(dev, workload):
    """The step bench.py times -- HotPath.step captured after three warm-ups and replayed, index rebuilt inside the graph -- checked
    output by output against the oracle for two replays, each with the Philox masks and noise of the seed word it drew; the last
    replay also bitwise against the same step run eagerly on its seed word.

    At C3 size only the forward outputs are compared with the oracle; every gradient of the last replay is compared bitwise with the eager step.  The C3
    gradients depend on the backward of PNA's std aggregator next to near-zero variances, and so does every gradient above it (d node
    attention feeds the extractor's backward).  Their error against fp64 varies with the seed word: the eager step gives the same
    numbers, and with exact-fp32 extractor products too.  For some words it exceeds the fp32 / fp64 slack of tests.util.close (the
    extractor's output bias gradient, a sum over 51 639 rows that cancels to ~4.6, is off by ~0.19).  The eager scope-A test and the
    fresh-batch C3 cases compare every gradient on their own inputs."""
    import bench
    import dp_gsat_amd as G
    from dp_gsat_amd.ops import ExtractorAttention, device_seed_state
    data, _, _ = bench.make_batch(workload, bench.WORKLOADS[workload]["graphs"], 0)
    wl, hot = _hot_path(workload, data, dev)
    skip = ()
    G.set_sync_free(True)
    try:
        with SeedRecorder() as rec:
            graph = capture(hot.step)
        pin_seed_stream(dev, STREAM_BASE)
        if workload == "c3":
            assert ExtractorAttention.last_forward_kind == 2        # the one-launch split-bf16 x 6 forward is what the bench reports
        words = []
        for _ in range(2):
            state0 = device_seed_state(dev).clone()
            base, counter = seed_state(dev)
            graph.replay()
            torch.cuda.synchronize()
            w = rec.check(base, counter)
            assert len(w) == 1, w
            words.append(w[0])
            got = _snapshot(hot.outputs())
            if workload == "c3":
                skip = {k for k in got if k.startswith("grad_")}
            _check_against_oracle(wl, data, _hot_inputs(hot), got, w[0], dev, skip)
        device_seed_state(dev).copy_(state0)                      # the eager step draws the last replay's seed word
        hot.step()
        torch.cuda.synchronize()
        for k, v in hot.outputs().items():
            assert torch.equal(v, got[k]), f"eager step != replay: {k}"
    finally:
        G.set_sync_free(False)
        G.clear_cache()
    assert words[0] != words[1]
    names = set(hot.outputs())
    assert {"att_log_logits", "att", "grad_emb", "grad_ext.feature_extractor.8.bias"} <= names
    assert ("edge_att" in names) == wl["edge_att"]


def _sizes(batch, G):
    return torch.bincount(batch, minlength=G).numpy().astype(np.int64)


def _moved_sizes(sizes, seed, big=300):
    """Graph node counts of ``sizes`` with single nodes moved from other graphs into graph 0 until it has ``big`` nodes, then the graphs
    shuffled (graph 0 keeps its place)."""
    rng = np.random.RandomState(seed)
    s = sizes.copy()
    donors = [g for g in rng.permutation(np.arange(1, s.size)) if s[g] >= 3]
    for g in donors[: max(big - int(s[0]), 0)]:
        s[g] -= 1
        s[0] += 1
    s[1:] = s[1:][rng.permutation(s.size - 1)]
    return s


CASES = {
    # name: (workload, graphs of batch A (None: the BASELINE count), fresh_batch arguments of batch B)
    "c2_rewired": ("c2", None, dict(undirected=True)),
    "c2_undirected_to_directed": ("c2", None, dict(undirected=True, redirect=40)),
    "c4_directed_to_undirected": ("c4", None, dict(undirected=True)),
    "c1_gin_hub": ("c1", None, dict(undirected=True, hub_edges=4 * 256 + 37)),
    "c3_pna_hub": ("c3", 256, dict(undirected=True, hub_edges=4 * 256 + 37)),
    "c3_moved_graph_sizes": ("c3", None, dict(undirected=True)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_replay_recomputes_the_index_for_a_fresh_batch(dev, case, monkeypatch):
    """Captured on batch A, replayed on batch B copied into the captured inputs in place (same N, E, G): CSRs, reverse permutation,
    the symmetrise flag, hub rows, segments and the fused extractor's tile plan must all come from B."""
    import bench
    import dp_gsat_amd as G
    from dp_gsat_amd import graph_index
    workload, graphs, kw = CASES[case]
    a, _, _ = bench.make_batch(workload, graphs or bench.WORKLOADS[workload]["graphs"], 0)
    N = a.batch.shape[0]
    if case == "c3_moved_graph_sizes":
        kw = dict(kw, sizes=_moved_sizes(_sizes(a.batch, a.num_graphs), 5))
    b = fresh_batch(a, 17, **kw)
    und_a, und_b = obk.is_undirected(a.edge_index, N), obk.is_undirected(b.edge_index, N)
    if case == "c2_undirected_to_directed":
        assert und_a and not und_b
    if case == "c4_directed_to_undirected":
        assert not und_a and und_b
    if "hub" in case:
        indeg = torch.bincount(b.edge_index[1], minlength=N)
        assert int(indeg.max()) >= 4 * 256 and int(torch.bincount(a.edge_index[1], minlength=N).max()) <= 256
        monkeypatch.setattr(graph_index, "_HUBS_SEEN", [False])           # no earlier batch of the process may have switched the hub path on
    wl, hot = _hot_path(workload, a, dev)
    d = hot.data
    G.set_sync_free(True)
    try:
        with SeedRecorder() as rec:
            graph = capture(hot.step)
        pin_seed_stream(dev, STREAM_BASE)
        if case == "c3_moved_graph_sizes":
            from dp_gsat_amd.ops import ExtractorAttention
            assert ExtractorAttention.last_forward_kind == 2
        ix = G.get_index(d.edge_index, N)                                     # the index object the graph rebuilds on every replay
        d.edge_index.copy_(b.edge_index.to(dev))
        d.batch.copy_(b.batch.to(dev))
        if d.edge_attr is not None:
            d.edge_attr.copy_(b.edge_attr.to(dev))
        base, counter = seed_state(dev)
        graph.replay()
        torch.cuda.synchronize()
        (word,) = rec.check(base, counter)
        got = _snapshot(hot.outputs())
        rp, perm = obk.csr_by(b.edge_index[1], N)
        assert np.array_equal(ix.rowptr_dst.cpu().numpy().astype(np.int64), rp)
        assert np.array_equal(ix.eid_by_dst.cpu().numpy().astype(np.int64), perm)
        if wl["edge_att"]:
            rev, flags = ix.rev_and_flag
            assert bool(int(flags[0])) == und_b                               # the replay's own symmetrise decision
            if und_b:
                assert np.array_equal(rev.cpu().numpy().astype(np.int64), obk.reverse_edge_perm(b.edge_index, N))
        _check_against_oracle(wl, b, _hot_inputs(hot), got, word, dev)
    finally:
        G.set_sync_free(False)
        G.clear_cache()


def _adam64(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=3e-6):
    """torch.optim.Adam's update (L2 weight decay, bias-corrected) in fp64, from the pre-step parameter and state."""
    p, g, m, v = (x.detach().cpu().double() for x in (p, g, m, v))
    g = g + wd * p
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    bc1, bc2 = 1 - betas[0] ** t, 1 - betas[1] ** t
    return p - lr / bc1 * m / (v.sqrt() / math.sqrt(bc2) + eps)


@pytest.mark.parametrize("backbone,edge", [("GIN", True), ("PNA", False)], ids=["GIN-edge", "PNA-node"])
def test_replayed_training_step_matches_oracle(dev, backbone, edge):
    """forward_pass (in-kernel Philox dropout and concrete noise), backward and fused capturable Adam -- bench.FullStep's step -- captured
    and replayed once: loss, attention and every gradient against the oracle fed with the replay's regenerated Philox inputs; the
    parameters after the step against an fp64 Adam update from the pre-step parameters and the replay's own gradients."""
    import dp_gsat_amd as G
    from dp_gsat_amd import synth
    from dp_gsat_amd.ops import edge_tensor
    data = synth.mutag_batch(os.path.join(ROOT, "tests", "golden", "mutag128.npz"), num_graphs=64)
    H = 32
    cfg = dict(model_name=backbone, n_layers=2, hidden_size=H, dropout_p=0.0, use_edge_attr=False,
               aggregators=["mean", "min", "max", "std"], scalers=False, deg=synth.in_degree_histogram(data))
    oclf = {"GIN": om.GIN, "PNA": om.PNA}[backbone](14, 0, 2, False, cfg)
    oext = om.ExtractorMLP(H, edge)
    clf = G.get_model(14, 0, 2, False, cfg, dev)
    ext = G.ExtractorMLP(H, edge).to(dev)
    params = list(clf.parameters()) + list(ext.parameters())
    names = [n for n, _ in clf.named_parameters()] + ["ext." + n for n, _ in ext.named_parameters()]
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-6, capturable=True, fused=True)
    gsat = G.GSAT(clf, ext, G.Criterion(2, False), opt, learn_edge_att=edge).train()
    gsat.sync_loss_dict = False
    ddev = data.to(dev)
    out = {}

    def step():
        G.clear_cache()
        att, loss, _, _ = gsat.forward_pass(ddev, 0, True)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        out["att"], out["loss"] = edge_tensor(att), loss

    G.set_sync_free(True)
    try:
        with SeedRecorder() as rec:
            graph = capture(step)
        pin_seed_stream(dev, STREAM_BASE)
        pre = [p.detach().clone() for p in params]
        st = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), float(opt.state[p]["step"])) for p in params]
        base, counter = seed_state(dev)
        graph.replay()
        torch.cuda.synchronize()
        (word,) = rec.check(base, counter)
    finally:
        G.set_sync_free(False)
        G.clear_cache()
    M = data.edge_index.shape[1] if edge else data.x.shape[0]
    masks, u = philox_inputs(word, M, 4 * H if edge else 2 * H, H, 0.5, dev)
    state = {n: t.cpu() for n, t in zip(names, pre)}
    assert {n for n, _ in oclf.named_parameters()} <= set(state)
    oclf.load_state_dict({k: state[k] for k in oclf.state_dict() if k in state}, strict=False)     # running stats: unused in training mode
    oext.load_state_dict({k: state["ext." + k] for k in oext.state_dict()})
    runs = {}
    for dt in (torch.float32, torch.float64):
        oc, oe = copy.deepcopy(oclf).to(dt), copy.deepcopy(oext).to(dt)
        d = NS(x=data.x.to(dt), edge_index=data.edge_index, batch=data.batch, edge_attr=None, y=data.y.to(dt))
        og = om.GSAT(oc, oe, om.Criterion(2, False), learn_edge_att=edge).train()
        o_att, o_loss, _, _, _ = og.forward_pass(d, 0, True, u=u.to(dt), masks=[m.to(dt) for m in masks])
        o_loss.backward()
        runs[dt] = (o_att.detach(), o_loss.detach(), [p.grad for p in list(oc.parameters()) + list(oe.parameters())])
    (a32, l32, g32), (a64, l64, g64) = runs[torch.float32], runs[torch.float64]
    close(out["loss"].reshape(()), l32.reshape(()), TOL, ref64=l64.reshape(()), what="loss")
    close(out["att"], a32, TOL, ref64=a64, what="edge_att")
    for n, p, q32, q64, p0, (m, v, t) in zip(names, params, g32, g64, pre, st):
        if q32 is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        close(p.grad, q32, TOL, ref64=q64, what="grad " + n)
        close(p, _adam64(p0, p.grad, m, v, t + 1), 1e-6, what="adam " + n)


def test_philox_inputs_match_a_device_seed_word(dev):
    """The masks and noise regenerated from a seed word equal the in-kernel draws also when the kernels read the word from seed_dev."""
    import dp_gsat_amd as G
    from dp_gsat_amd.ops import ExtractorAttention
    from tests.graphs import random_batch
    H = 32
    ei, batch, N = random_batch(9, 12, 4, 30)
    ei, batch = ei.to(dev), batch.to(dev)
    for edge in (True, False):
        ext = G.ExtractorMLP(H, edge).to(dev).train()
        emb = torch.randn(N, H, device=dev)
        M = ei.shape[1] if edge else N
        word = 0x1234_5678_9ABC_DEF
        masks, u = philox_inputs(word, M, 4 * H if edge else 2 * H, H, 0.5, dev)
        index = G.get_index(ei, N)
        seg = index.graphs(batch)
        l1, l2, l3 = ext.mlp.linears()
        wts = (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
        sd = torch.tensor([word], dtype=torch.int64, device=dev)
        z1, a1 = ExtractorAttention.apply(emb, *wts, index, seg, edge, True, 0.5, 0, None, None, None, sd, True)
        z2, a2 = ext.attend(emb, ei, batch, noise=u.to(dev), dropout_masks=[m.to(dev) for m in masks])
        assert torch.equal(z1, z2) and torch.equal(a1, a2)


def test_device_seed_survives_reseeding(dev):
    """A captured graph holds the address of the device seed state.  torch.manual_seed plus one eager device_seed call must re-base that
    state in place: the replay then draws the next word of the new stream and touches no memory but its own state."""
    import dp_gsat_amd as G
    from dp_gsat_amd import ops
    from tests.graphs import random_batch
    H = 32
    ei, batch, N = random_batch(4, 8, 4, 20)
    ei, batch = ei.to(dev), batch.to(dev)
    ext = G.ExtractorMLP(H, True).to(dev).train()
    emb = torch.randn(N, H, device=dev)
    out = {}

    def step():
        out["att"] = ext.attend(emb, ei, batch, noise="philox")[1]

    G.set_sync_free(True)
    try:
        torch.manual_seed(4321)
        ops.device_seed(dev)                                  # the stream's state is (re)made on the default stream, outside any capture
        with SeedRecorder() as rec:
            graph = capture(step)
        torch.cuda.synchronize()
        torch.manual_seed(99)
        g = torch.Generator()
        g.manual_seed(99)
        base = int(torch.empty((), dtype=torch.int64).random_(generator=g)) & ((1 << 64) - 1)      # ops.new_seed()'s first draw
        eager = int(ops.device_seed(dev).item())
        assert eager == seed_next_ref(base, 0)
        sentinel = -0x5A5A5A5A5A5A5A5
        blocks = [torch.full((2,), sentinel, dtype=torch.int64, device=dev) for _ in range(64)]
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for t in blocks:
            assert t.tolist() == [sentinel, sentinel], "a replay wrote into memory it does not own"
        assert rec.words() == [seed_next_ref(base, 1)]
        assert seed_state(dev) == (base, 2)
    finally:
        G.set_sync_free(False)
        G.clear_cache()
