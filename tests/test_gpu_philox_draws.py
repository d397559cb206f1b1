"""-m gpu: the library's Philox reporters (gsat_philox_keep_mask, gsat_philox_noise) against the numpy restatement of
tests/philox_ref.py, bit for bit: no tolerance.  The reporters call the device functions the consumers call (philox_keep4,
philox_noise_u), and the consumers are compared with the reporters elsewhere (BatchNorm tail and ReLU+dropout in test_gpu_norm.py, the
staged extractor in test_gpu_attention.py, the sliced-segment run in test_gpu_scale.py, the replayed steps in tests/replay.py): with
this file those comparisons reach a statement of the draw that shares no code with the library."""
import numpy as np
import pytest
import torch

from tests import philox_ref as pr

pytestmark = pytest.mark.gpu
SEEDS = (0x5EED, (0x9ABCDEF1 << 32) | 0x2468ACE1)           # the second is >= 2^32: both key words matter
STREAMS = (1, 2, 3, 5)                                      # extractor layers 1 / 2, BatchNorm tail, ReLU+dropout
PS = (0.1, 0.3, 0.5, 0.8)
GUARD = 64


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _reported_mask(seed, stream, M, C, p, dev):
    from dp_gsat_amd._lib import call, ptr, stream as hip_stream
    buf = torch.full((M * C + GUARD,), -1.0, device=dev)     # guard entries behind the M * C the kernel may write
    call("gsat_philox_keep_mask", int(seed), stream, M, C, p, ptr(buf), hip_stream())
    assert bool((buf[M * C:] == -1.0).all()), f"M={M} C={C}: the reporter wrote beyond M * C"
    return buf[:M * C].view(M, C)


def _reported_noise(seed, M, dev):
    from dp_gsat_amd._lib import call, ptr, stream as hip_stream
    buf = torch.full((M + GUARD,), -1.0, device=dev)
    call("gsat_philox_noise", int(seed), M, ptr(buf), hip_stream())
    assert bool((buf[M:] == -1.0).all()), f"M={M}: the reporter wrote beyond M"
    return buf[:M]


# one row; less than a block; a ragged width (17 float4 groups per row, rows straddle blocks); several blocks at the widest extractor layer
@pytest.mark.parametrize("M,C", [(1, 4), (255, 8), (257, 68), (1030, 256)])
@pytest.mark.parametrize("stream", STREAMS)
def test_keep_mask_is_the_numpy_philox_stream(dev, stream, M, C):
    for seed in SEEDS:
        for p in PS:
            got = _reported_mask(seed, stream, M, C, p, dev)
            want = pr.keep_mask(seed, stream, M, C, p)
            bad = np.flatnonzero(_bits(got).reshape(-1) != want.view(np.int32).reshape(-1))
            assert bad.size == 0, (f"stream {stream} seed={seed:#x} p={p} [{M}, {C}]: {bad.size} entries differ, the first at "
                                   f"(row {bad[0] // C}, column {bad[0] % C})")


@pytest.mark.parametrize("seed,stream,p", [(SEEDS[0], 1, 0.3), (SEEDS[1], 5, 0.5)])
def test_keep_mask_beyond_the_grid_stride_cap(dev, seed, stream, p):
    """4100 * 2048 / 4 = 2 099 200 float4 items, more than the 8192 blocks x 256 threads that ew_blocks launches at most: the last
    2048 items are written on the second trip of the grid-stride loop."""
    M, C = 4100, 2048
    assert M * C // 4 > 8192 * 256
    got = _reported_mask(seed, stream, M, C, p, dev)
    want = torch.from_numpy(pr.keep_mask(seed, stream, M, C, p)).to(dev)             # 0.0 / 1.0: equal values are equal bits
    assert bool(((got == 0) | (got == 1)).all())
    bad = (got != want).reshape(-1).nonzero().reshape(-1)
    assert bad.numel() == 0, (f"{bad.numel()} entries differ, the first at (row {int(bad[0]) // C}, column {int(bad[0]) % C}), the last "
                              f"at row {int(bad[-1]) // C}")


@pytest.mark.parametrize("M", [1, 255, 256, 257, 70001])       # the 256-thread block edge; 274 blocks
def test_noise_is_the_numpy_philox_stream(dev, M):
    for seed in SEEDS:
        got = _reported_noise(seed, M, dev)
        want = pr.concrete_uniform(seed, M)
        bad = np.flatnonzero(_bits(got) != want.view(np.int32))
        assert bad.size == 0, f"M={M} seed={seed:#x}: {bad.size} entries differ, the first at row {bad[0]}"
        assert float(got.min()) >= 2.0 ** -24 and float(got.max()) <= 1.0 - 2.0 ** -24


def test_empty_input(dev):
    from dp_gsat_amd._lib import call, stream as hip_stream
    assert call("gsat_philox_keep_mask", 1, 1, 0, 4, 0.5, None, hip_stream()) == 0
    assert call("gsat_philox_noise", 1, 0, None, hip_stream()) == 0
