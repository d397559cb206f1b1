"""-m gpu: every extractor path that draws its dropout masks and its concrete-sampler noise inside the kernels from a seed, against the
same call fed the masks and the noise as tensors built by numpy (tests/philox_ref.py): staged forward and backward at the five
lane-group widths of the head kernel, sliced segments, the one-launch forward, the fused backward (staged keep bits and keep_one), and
the public module.  Both runs do the same arithmetic on the same 0 / 1 values, so every output, every saved tensor and every gradient
is compared bit for bit: there is no tolerance in this file."""
import pytest
import torch

from tests import philox_ref as pr
from tests.graphs import shuffle_edges
from tests.test_gpu_attn_fused import BWD_CASES, CASES, _fwd_bwd, _params, _run, _sized_batch

pytestmark = pytest.mark.gpu
S = (0x9ABCDEF1 << 32) | 0x2468ACE1             # >= 2^63: both key words matter, and the word is negative as an int64
OTHER = 123                                     # the by-value seed that must lose against a device word


def _word(seed, dev):
    """The seed as a device word: int64 holds the bits of a uint64."""
    return torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device=dev)


def _assert_same(got, want, what):
    """Bit equality of every tensor of ``want`` (and nothing left unwritten in it)."""
    for k, w in want.items():
        if w is None or not torch.is_tensor(w):
            assert got[k] == w, f"{what}: {k}"
            continue
        assert not torch.isnan(w).any(), f"{what}: {k} of the explicit-tensor run has unwritten or NaN entries"
        g = got[k]
        if not torch.equal(g.view(torch.int32), w.view(torch.int32)):
            bad = (g.view(torch.int32) != w.view(torch.int32)).reshape(-1).nonzero().reshape(-1)
            cols = w.shape[-1] if w.dim() > 1 else 1
            i = int(bad[0])
            raise AssertionError(f"{what}: {k} differs in {bad.numel()} of {w.numel()} entries, the first at (row {i // cols}, column "
                                 f"{i % cols}): {float(g.reshape(-1)[i])!r} with the seed, {float(w.reshape(-1)[i])!r} with the numpy tensors")


class _Problem:
    """One batch, its parameters and upstream gradients, and the numpy draws of seed S for it."""

    def __init__(self, dev, sizes, H, edge_mode, seed):
        ei, self.batch, N = _sized_batch(sizes, seed=seed)
        self.ei = shuffle_edges(ei, 3)
        self.G = len(sizes)
        self.edge_mode, self.dev, self.H = edge_mode, dev, H
        g = torch.Generator().manual_seed(5)
        self.emb = torch.randn(N, H, generator=g).to(dev)
        self.params = _params(H, edge_mode, dev, 11)
        self.M = self.ei.shape[1] if edge_mode else N
        self.C1, self.C2 = self.params[0].shape[0], self.params[2].shape[0]
        self.dl, self.da = torch.randn(self.M, generator=g).to(dev), torch.randn(self.M, generator=g).to(dev)
        self.u = torch.from_numpy(pr.concrete_uniform(S, self.M)).to(dev)

    def masks(self, p):
        return tuple(torch.from_numpy(pr.keep_mask(S, layer, self.M, C, p)).to(self.dev) for layer, C in ((1, self.C1), (2, self.C2)))

    def ones(self):
        return torch.ones(self.M, self.C1, device=self.dev), torch.ones(self.M, self.C2, device=self.dev)

    def fwd(self, p, masks, u, fused, training=True, **kw):
        return _run(self.dev, self.emb, self.params, self.ei, self.batch, self.G, self.edge_mode, training, p, masks, u, fused=fused, **kw)

    def fwd_bwd(self, p, masks, u, fused_bwd, monkeypatch, training=True, **kw):
        return _fwd_bwd(self.dev, self.emb, self.params, self.ei, self.batch, self.G, self.edge_mode, masks, u, self.dl, self.da, fused_bwd,
                        monkeypatch, p=p, training=training, saved=True, **kw)


def _draws_matter(a, b, what):
    """The comparison is not vacuous: another mask / another noise gives other numbers."""
    assert not torch.equal(a["att"], b["att"]), f"{what}: the attention does not depend on the draw"


@pytest.mark.parametrize("H", [16, 32, 64, 128, 256])              # k_head_fwd with 4, 8, 16, 32, 64 lanes per row
@pytest.mark.parametrize("edge_mode", [False, True])
def test_staged_forward_and_backward_draw_the_numpy_masks_and_noise(dev, H, edge_mode, monkeypatch):
    pb = _Problem(dev, CASES["molecules"], H, edge_mode, seed=H + 3)
    word = _word(S, dev)
    runs = {}
    for p in (0.1, 0.5, 0.8):
        want = pb.fwd_bwd(p, pb.masks(p), pb.u, False, monkeypatch)
        _assert_same(pb.fwd_bwd(p, None, None, False, monkeypatch, seed=S), want, f"p={p}, seed by value")
        _assert_same(pb.fwd_bwd(p, None, None, False, monkeypatch, seed=OTHER, seed_dev=word), want, f"p={p}, seed read on the device")
        runs[p] = want
    _draws_matter(runs[0.1], runs[0.5], "p = 0.1 / 0.5")
    _draws_matter(pb.fwd_bwd(0.5, None, None, False, monkeypatch, seed=OTHER), runs[0.5], "another seed")


@pytest.mark.parametrize("edge_mode", [False, True])
def test_sliced_segments_draw_the_numpy_masks_and_noise(dev, edge_mode, monkeypatch):
    """Two graphs of more than 4096 rows each: the statistics are taken in two slices per graph and the activations, dh2 and dh1 by the
    elementwise kernels (k_norm_apply, k_dh2, k_dh1) instead of inside the statistics launches."""
    sizes = [1945, 1920] if edge_mode else [4200, 4150]             # edge mode: 2.16 edges per node -> about 4200 and 4150 rows
    pb = _Problem(dev, sizes, 16, edge_mode, seed=21)
    assert 4096 < pb.M // 2 <= 8192, f"{pb.M} rows in 2 graphs: not the two-slice path"
    p = 0.3
    want = pb.fwd_bwd(p, pb.masks(p), pb.u, False, monkeypatch)
    _assert_same(pb.fwd_bwd(p, None, None, False, monkeypatch, seed=S), want, "seed by value")
    _assert_same(pb.fwd_bwd(p, None, None, False, monkeypatch, seed=OTHER, seed_dev=_word(S, dev)), want, "seed read on the device")
    _draws_matter(pb.fwd_bwd(p, None, None, False, monkeypatch, seed=OTHER), want, "another seed")


def _fused_forward_case(dev, case, H, edge_mode):
    pb = _Problem(dev, CASES[case], H, edge_mode, seed=H + len(CASES[case]))
    assert pb.M > 0
    kinds = set()
    for p in (0.1, 0.5):
        want = pb.fwd(p, pb.masks(p), pb.u, True)
        _assert_same(pb.fwd(p, None, None, True, seed=S), want, f"p={p}, seed by value")
        _assert_same(pb.fwd(p, None, None, True, seed=OTHER, seed_dev=_word(S, dev)), want, f"p={p}, seed read on the device")
        kinds.add(want["kind"])
    _draws_matter(pb.fwd(0.5, None, None, True, seed=OTHER), want, "another seed")
    assert kinds <= {1, 2}, f"kind {kinds}: the library did not take the one-launch forward"
    return kinds


@pytest.mark.parametrize("case", ["molecules", "big_graphs", "empty_and_tiny"])
@pytest.mark.parametrize("H", [16, 64, 80, 128])
@pytest.mark.parametrize("edge_mode", [False, True])
def test_fused_forward_draws_the_numpy_masks_and_noise(dev, case, H, edge_mode, monkeypatch):
    """The one-launch forward: keep4f at both layers, and the in-kernel concrete noise at both of its sites (whole-graph tiles and the
    slab walk of graphs larger than a tile)."""
    monkeypatch.delenv("GSAT_ATTN_FUSED_PQG", raising=False)
    monkeypatch.delenv("GSAT_ATTN_FUSED_X6", raising=False)
    _fused_forward_case(dev, case, H, edge_mode)


@pytest.mark.parametrize("case", ["molecules", "big_graphs", "empty_and_tiny"])
@pytest.mark.parametrize("edge_mode,x6,pqg", [(False, "0", None), (True, "0", None), (True, None, "0"), (True, "0", "0")])
def test_fused_forward_variants_draw_the_numpy_masks_and_noise(dev, case, x6, pqg, edge_mode, monkeypatch):
    """H = 64 with P | Q through global memory or kept in the tile (GSAT_ATTN_FUSED_PQG) and with the split-bf16 or the fp32 products
    (GSAT_ATTN_FUSED_X6), each switched off (both at their defaults: the H = 64 cases of the test above; node mode has no P | Q)."""
    for name, val in (("GSAT_ATTN_FUSED_X6", x6), ("GSAT_ATTN_FUSED_PQG", pqg)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    kinds = _fused_forward_case(dev, case, 64, edge_mode)
    assert kinds == ({1} if x6 == "0" else {2}), kinds


@pytest.mark.parametrize("case", list(BWD_CASES))
@pytest.mark.parametrize("H", [16, 64, 80, 128])
@pytest.mark.parametrize("edge_mode", [False, True])
def test_fused_backward_regenerates_the_numpy_masks(dev, case, H, edge_mode, monkeypatch):
    """GSAT_ATTN_BWD_FUSED=1: the keep bits the backward stages per tile ("molecules", "tiny") and the per-element keep_one of graphs
    larger than a tile ("big_graphs") are the bits the forward dropped with."""
    pb = _Problem(dev, BWD_CASES[case], H, edge_mode, seed=H + 1)
    assert pb.M > 0 and pb.C1 <= 512                                # the widths the fused backward takes
    word = _word(S, dev)
    for p in (0.1, 0.5):
        want = pb.fwd_bwd(p, pb.masks(p), pb.u, True, monkeypatch)             # the fused backward's own explicit-mask run
        _assert_same(pb.fwd_bwd(p, None, None, True, monkeypatch, seed=S), want, f"p={p}, seed by value")
        _assert_same(pb.fwd_bwd(p, None, None, True, monkeypatch, seed=OTHER, seed_dev=word), want, f"p={p}, seed read on the device")
    other = pb.fwd_bwd(0.5, None, None, True, monkeypatch, seed=OTHER)
    assert not torch.equal(other["dW2"], want["dW2"]), "another seed, the same gradients"


@pytest.mark.parametrize("paths", ["default", "fused"])
@pytest.mark.parametrize("edge_mode", [False, True])
def test_module_with_a_seed_equals_module_with_numpy_masks_and_noise(dev, edge_mode, paths, monkeypatch):
    """ExtractorMLP.attend of the DP-GSAT constructor (extractor_dropout_p = 0.3): seed + noise="philox" against explicit tensors --
    logits, attention and every gradient -- on the library's default paths and with the one-launch forward and the fused backward."""
    import dp_gsat_amd as G
    if paths == "fused":
        monkeypatch.setenv("GSAT_ATTN_FUSED", "1")
        monkeypatch.setenv("GSAT_ATTN_BWD_FUSED", "1")
    else:
        monkeypatch.delenv("GSAT_ATTN_FUSED", raising=False)
        monkeypatch.delenv("GSAT_ATTN_BWD_FUSED", raising=False)
    H, p = 32, 0.3
    sizes = [30, 200, 12, 45, 0, 70]
    ei, batch, N = _sized_batch(sizes, seed=9)
    ei = shuffle_edges(ei, 1)
    M = ei.shape[1] if edge_mode else N
    ext = G.ExtractorMLP(H, dict(learn_edge_att=edge_mode, extractor_dropout_p=p), type="primal").to(dev).train()
    assert ext.mlp.dropout_p == p
    C1 = 4 * H if edge_mode else 2 * H
    g = torch.Generator().manual_seed(H)
    emb = torch.randn(N, H, generator=g).to(dev)
    gz, ga = torch.randn(M, 1, generator=g).to(dev), torch.randn(M, 1, generator=g).to(dev)
    masks = [torch.from_numpy(pr.keep_mask(S, 1, M, C1, p)).to(dev), torch.from_numpy(pr.keep_mask(S, 2, M, H, p)).to(dev)]
    u = torch.from_numpy(pr.concrete_uniform(S, M)).to(dev).view(M, 1)
    runs = []
    for how in ("numpy tensors", "seed", "another seed"):
        ext.zero_grad(set_to_none=True)
        e = emb.clone().requires_grad_(True)
        if how == "numpy tensors":
            z, a = ext.attend(e, ei.to(dev), batch.to(dev), noise=u, dropout_masks=masks)
        else:
            z, a = ext.attend(e, ei.to(dev), batch.to(dev), noise="philox", seed=S if how == "seed" else OTHER)
        torch.autograd.backward([z, a], [gz, ga])
        runs.append(dict(logits=z.detach(), att=a.detach(), demb=e.grad, **{k: q.grad.clone() for k, q in ext.named_parameters()}))
    assert len(runs[0]) == 3 + 6
    if paths == "fused":
        from dp_gsat_amd.ops import ExtractorAttention
        assert ExtractorAttention.last_forward_kind in (1, 2), "the library did not take the one-launch forward"
    _assert_same(runs[1], runs[0], "attend(seed, noise='philox')")
    _draws_matter(runs[2], runs[0], "another seed")


@pytest.mark.parametrize("fused_fwd,fused_bwd", [(False, False), (False, True), (True, None)])
@pytest.mark.parametrize("edge_mode", [False, True])
def test_no_draw_where_none_is_due(dev, edge_mode, fused_fwd, fused_bwd, monkeypatch):
    """Evaluation mode with a seed and p = 0.5, and training mode with p = 0, equal the run with all-ones masks: nothing is dropped
    (with p = 0 the concrete noise is still drawn)."""
    for case in ("molecules", "big_graphs"):
        pb = _Problem(dev, BWD_CASES[case], 64, edge_mode, seed=65)
        for training, p, u in ((False, 0.5, None), (True, 0.0, pb.u)):
            if fused_fwd:
                want = pb.fwd(p, pb.ones(), u, True, training=training)
                got = pb.fwd(p, None, None, True, training=training, seed=S)
                assert want["kind"] in (1, 2)
            else:
                want = pb.fwd_bwd(p, pb.ones(), u, fused_bwd, monkeypatch, training=training)
                got = pb.fwd_bwd(p, None, None, fused_bwd, monkeypatch, training=training, seed=S)
            _assert_same(got, want, f"{case}, training={training}, p={p}")
