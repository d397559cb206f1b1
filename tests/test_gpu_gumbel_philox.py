"""-m gpu: the Gumbel-sigmoid sampler that draws its uniform inside the kernel (gsat_gumbel_sigmoid_philox) against the numpy Philox
restatement and against gsat_sample_fwd(mode 2) on the reported noise.  Everything is compared bit for bit: no tolerance."""
import numpy as np
import pytest
import torch

from tests import philox_ref as pr

pytestmark = pytest.mark.gpu
SIZES = [1, 3, 4, 5, 255, 1023, 1024, 1025, 4099]          # the four-per-thread tail and the 256 x 4 block edge
TAU, EPS = 0.1, 1e-10                                       # DualGSAT's values
SEEDS = (0x5EED, (0x9ABCDEF1 << 32) | 0x2468ACE1)           # the second is >= 2^32: both key words matter


def _word(seed, dev):
    """The seed as a device word: int64 holds the bits of a uint64."""
    return torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device=dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _noise(seed, M, dev):
    from dp_gsat_amd._lib import call, ptr, stream
    u = torch.full((M + 8,), -1.0, device=dev)               # guard entries behind the M the kernel may write
    call("gsat_philox_gumbel_noise", int(seed), M, ptr(u), stream())
    assert bool((u[M:] == -1.0).all()), f"M={M}: the reporter wrote beyond M"
    return u[:M].clone()


def _philox_att(z, seed, dev, seed_dev=None, out_offset=0):
    """att of the C entry on the logits view ``z``, written into a guarded buffer at ``out_offset`` floats from an aligned address."""
    from dp_gsat_amd._lib import call, ptr, stream
    M = z.numel()
    buf = torch.full((M + out_offset + 8,), -1.0, device=dev)
    att = buf[out_offset:out_offset + M]
    call("gsat_gumbel_sigmoid_philox", ptr(z), M, TAU, EPS, int(seed), ptr(seed_dev), ptr(att), stream())
    assert bool((buf[:out_offset] == -1.0).all()) and bool((buf[out_offset + M:] == -1.0).all()), f"M={M}: written out of bounds"
    return att.clone()


def _sample_fwd(z, u, dev):
    from dp_gsat_amd._lib import call, ptr, stream
    att = torch.empty(z.numel(), device=dev)
    call("gsat_sample_fwd", ptr(z.contiguous()), ptr(u), 2, TAU, EPS, z.numel(), ptr(att), stream())
    return att


def _logits(M, dev):
    g = torch.Generator().manual_seed(M)
    buf = (torch.randn(M + 1, generator=g) * 3).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf


@pytest.mark.parametrize("M", SIZES)
def test_reported_noise_is_the_numpy_philox_stream(dev, M):
    big = {}
    for seed in SEEDS:
        u = _noise(seed, M, dev)
        want = pr.gumbel_uniform(seed, M)
        assert np.array_equal(_bits(u), want.view(np.int32)), f"M={M} seed={seed:#x}"
        assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
        big[seed] = _noise(seed, SIZES[-1], dev)
        assert torch.equal(big[seed][:M], u), f"M={M}: U[:M] depends on M"
    assert not torch.equal(big[SEEDS[0]], big[SEEDS[1]])


@pytest.mark.parametrize("M", SIZES)
def test_sampler_is_bitwise_sample_fwd_on_the_reported_noise(dev, M):
    buf = _logits(M, dev)
    seed = SEEDS[1]
    u = _noise(seed, M, dev)
    word = _word(seed, dev)
    for z_off in (0, 1):                                     # aligned logits, and logits one float off 16-byte alignment
        z = buf[z_off:z_off + M]
        assert (z.data_ptr() % 16 == 0) == (z_off == 0)
        want = _sample_fwd(z, u, dev)
        assert bool(((want >= 0) & (want <= 1)).all())
        for out_off in (0, 1):                               # and the same for the output
            got = _philox_att(z, seed, dev, out_offset=out_off)
            assert np.array_equal(_bits(got), _bits(want)), f"M={M} logits+{z_off} att+{out_off}"
            dev_got = _philox_att(z, 123, dev, seed_dev=word, out_offset=out_off)       # the device word wins over the value
            assert np.array_equal(_bits(dev_got), _bits(want)), f"M={M} logits+{z_off} att+{out_off}: seed read on the device"
    # another seed, another attention: on zero logits, where U[0] = 0.180 / 0.734 of the two seeds give 0.0045 / 0.99999 (random logits
    # may push a single entry to the same saturated 1.0 under both seeds at tau = 0.1)
    flat = torch.zeros(M, device=dev)
    assert not torch.equal(_philox_att(flat, SEEDS[0], dev), _philox_att(flat, SEEDS[1], dev)), f"M={M}: another seed, the same attention"


def test_empty_input_and_bad_arguments(dev):
    from dp_gsat_amd._lib import GsatHipError, call, ptr, stream
    assert call("gsat_gumbel_sigmoid_philox", None, 0, TAU, EPS, 1, None, None, stream()) == 0
    assert call("gsat_philox_gumbel_noise", 1, 0, None, stream()) == 0
    z = torch.zeros(4, device=dev)
    for args in ((ptr(z), 4, 0.0, EPS, 1, None, ptr(z)), (None, 4, TAU, EPS, 1, None, ptr(z)), (ptr(z), 4, TAU, EPS, 1, None, None),
                 (ptr(z), 2 ** 31, TAU, EPS, 1, None, ptr(z))):
        with pytest.raises(GsatHipError, match="code -2"):
            call("gsat_gumbel_sigmoid_philox", *args, stream())
    with pytest.raises(GsatHipError, match="code -2"):
        call("gsat_philox_gumbel_noise", 1, 4, None, stream())


@pytest.mark.parametrize("M", [5, 1025])
def test_operator_and_its_backward_equal_sample_with_the_same_noise(dev, M):
    import dp_gsat_amd as G
    from dp_gsat_amd.ops import Sample, SamplePhilox
    seed = SEEDS[1]
    z0 = _logits(M, dev)[:M].view(M, 1)
    u = _noise(seed, M, dev).view(M, 1)
    gout = torch.randn(M, 1, generator=torch.Generator().manual_seed(3)).to(dev)
    runs = []
    for how in ("noise", "int seed", "device seed", "noise wins"):
        z = z0.clone().requires_grad_(True)
        if how == "noise":
            att = Sample.apply(z, u, 2, TAU, EPS)
        elif how == "int seed":
            att = G.gumbel_sigmoid(z, tau=TAU, eps=EPS, seed=seed)
            assert att.grad_fn is not None and type(att.grad_fn).__name__.startswith(SamplePhilox.__name__)
        elif how == "device seed":
            att = G.gumbel_sigmoid(z, tau=TAU, eps=EPS, seed=_word(seed, dev))
        else:
            att = G.gumbel_sigmoid(z, tau=TAU, eps=EPS, noise=u, seed=SEEDS[0])
        att.backward(gout)
        runs.append((how, att.detach(), z.grad))
    for how, att, dz in runs[1:]:
        assert np.array_equal(_bits(att), _bits(runs[0][1])), how
        assert np.array_equal(_bits(dz), _bits(runs[0][2])), how + ": backward"
    with pytest.raises(ValueError, match="seed"):
        G.gumbel_sigmoid(z0, tau=TAU, eps=EPS, seed=torch.tensor([1, 2], dtype=torch.int64, device=dev))
    torch.manual_seed(5)                                     # with neither, torch's generator as before
    a = G.gumbel_sigmoid(z0, tau=TAU, eps=EPS)
    torch.manual_seed(5)
    b = Sample.apply(z0, torch.rand_like(z0), 2, TAU, EPS)
    assert torch.equal(a, b)
