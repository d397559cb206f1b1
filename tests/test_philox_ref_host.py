"""Host checks of tests/philox_ref.py, the numpy restatement the GPU draws are compared with bit for bit: the published Random123
known answers of Philox4x32-10, the definitions of the four draws, and the statistics a sound generator must show (each stream, key
word, row and column group an independent fair coin).  Every statistical bound is 5 standard deviations of the binomial (or uniform)
law of the quantity -- about 6e-7 per check for a true generator -- and the seed is fixed, so nothing here is flaky; the deviations
observed when the test was written are noted beside each check."""
import numpy as np
import pytest

from tests import philox_ref as pr

S = (0x9ABCDEF1 << 32) | 0x2468ACE1             # >= 2^32: both key words matter
M, C = 4096, 64

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_known_answers(ctr, key, want):
    got = tuple(int(w) for w in pr.philox4x32(key, *ctr))
    assert got == want, [hex(w) for w in got]
    # the same through arrays: the vector path is the scalar path
    arr = pr.philox4x32(key, *(np.full(3, c, dtype=np.uint64) for c in ctr))
    assert all(w.dtype == np.uint32 and w.tolist() == [x] * 3 for w, x in zip(arr, want))


def _unit24(w):
    return (int(w) >> 8) / 2.0 ** 24            # exact in double, and exactly a float32


def test_draws_equal_their_definitions_entry_by_entry():
    """Each draw, recomputed for single entries from scalar philox4x32 calls with python integers."""
    key = (S & 0xFFFFFFFF, S >> 32)
    g = pr.gumbel_uniform(S, 23)
    assert g.dtype == np.float32 and g.shape == (23,)
    for m in (0, 1, 3, 4, 17, 22):
        assert float(g[m]) == _unit24(pr.philox4x32(key, m >> 2, 0, 5, 0x5A17)[m & 3]), m
    for layer in (1, 2, 3, 5):
        k = pr.keep_uniform(S, layer, 9, 12)
        assert k.dtype == np.float32 and k.shape == (9, 12)
        for row, c in ((0, 0), (0, 3), (0, 4), (5, 7), (8, 11), (3, 9)):
            assert float(k[row, c]) == _unit24(pr.philox4x32(key, row, c >> 2, layer, 0x5A17)[c & 3]), (layer, row, c)
        for p in (0.1, 0.3, 0.5, 0.8):
            mask = pr.keep_mask(S, layer, 9, 12, p)
            assert mask.dtype == np.float32 and np.array_equal(mask, (k >= np.float32(p)).astype(np.float32))
            assert set(np.unique(mask)) <= {0.0, 1.0}
    u = pr.concrete_uniform(S, 11)
    assert u.dtype == np.float32 and u.shape == (11,)
    for row in (0, 1, 10):
        x = int(pr.philox4x32(key, row, 0, 4, 0x5A17)[0])
        assert float(u[row]) == ((x >> 9) + 0.5) / 2.0 ** 23, row
    # p = 0 keeps everything, p = 1 nothing (the uniforms are in [0, 1))
    assert pr.keep_mask(S, 1, 4, 4, 0.0).min() == 1.0 and pr.keep_mask(S, 1, 4, 4, 1.0).max() == 0.0
    # only the low 64 bits of the seed count, and a negative int64 is its two's complement
    assert np.array_equal(pr.keep_uniform(S - (1 << 64), 1, 3, 4), pr.keep_uniform(S, 1, 3, 4))
    assert np.array_equal(pr.concrete_uniform(S + (1 << 64), 3), pr.concrete_uniform(S, 3))


def test_relu_dropout_and_gumbel_share_stream_5_edit_here_if_relu_dropout_gets_its_own_stream():
    """ReLU+dropout (csrc/norm.hip: RELU_DROPOUT_STREAM) and the Gumbel uniform (csrc/edgeops.hip: gumbel_uniform4) both use Philox
    stream 5: under one seed, the uniforms behind columns 0..3 of ReLU+dropout row r ARE the Gumbel uniforms of entries 4r..4r+3.
    Latent today, because every caller draws a fresh seed per call.  THIS is the test to edit if ReLU+dropout ever gets a stream of
    its own (which changes every seeded GIN run): the equality below then becomes an inequality, and the stream table of
    tests/philox_ref.py and the stream argument of the ReLU+dropout cases in tests/test_gpu_philox_draws.py change with it."""
    rows = 257
    for seed in (0x5EED, S):
        assert np.array_equal(pr.gumbel_uniform(seed, 4 * rows).reshape(rows, 4), pr.keep_uniform(seed, 5, rows, C)[:, :4])
        assert not np.array_equal(pr.gumbel_uniform(seed, 4 * rows).reshape(rows, 4), pr.keep_uniform(seed, 3, rows, C)[:, :4])


def test_first_rows_do_not_depend_on_the_row_count():
    for m in (1, 5, 255):
        for layer in (1, 5):
            assert np.array_equal(pr.keep_uniform(S, layer, m, 20), pr.keep_uniform(S, layer, 300, 20)[:m])
            assert np.array_equal(pr.keep_mask(S, layer, m, 20, 0.3), pr.keep_mask(S, layer, 300, 20, 0.3)[:m])
        assert np.array_equal(pr.concrete_uniform(S, m), pr.concrete_uniform(S, 300)[:m])
        assert np.array_equal(pr.gumbel_uniform(S, m), pr.gumbel_uniform(S, 300)[:m])
    # and the first column groups do not depend on the width
    assert np.array_equal(pr.keep_uniform(S, 2, 40, 8), pr.keep_uniform(S, 2, 40, 64)[:, :8])
    assert pr.keep_uniform(S, 1, 0, 8).shape == (0, 8) and pr.concrete_uniform(S, 0).shape == (0,)


def test_ranges():
    for layer in (1, 2, 3, 5):
        k = pr.keep_uniform(S, layer, M, C)
        assert k.min() >= 0.0 and k.max() < 1.0
        assert k.max() <= np.float32(1.0 - 2.0 ** -24)
    u = pr.concrete_uniform(S, 1 << 16)
    assert u.min() >= np.float32(2.0 ** -24) and u.max() <= np.float32(1.0 - 2.0 ** -24)
    g = pr.gumbel_uniform(S, 1 << 16)
    assert g.min() >= 0.0 and g.max() < 1.0


def _z(count, n, q):
    """Deviation of a Binomial(n, q) count from its mean, in standard deviations."""
    return (count - n * q) / np.sqrt(n * q * (1.0 - q))


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5, 0.8])
def test_keep_fraction_is_one_minus_p(p):
    """n = 4096 * 64 coins per stream; 5 sigma = 5 * sqrt(p (1 - p) / n), e.g. 0.0049 at p = 0.5.
    Observed worst |z| of the four streams: p = 0.1: 1.54, 0.3: 1.48, 0.5: 1.93, 0.8: 1.84."""
    # the threshold is float32(p) on a 2^-24 grid: P(keep) = 1 - ceil(float32(p) * 2^24) / 2^24, within 6e-8 of 1 - p
    q = 1.0 - np.ceil(float(np.float32(p)) * 2.0 ** 24) / 2.0 ** 24
    assert abs(q - (1.0 - p)) < 1e-7
    for layer in (1, 2, 3, 5):
        z = _z(float(pr.keep_mask(S, layer, M, C, p).sum()), M * C, q)
        print(f"p={p} stream {layer}: z = {z:+.2f}")
        assert abs(z) < 5.0, (layer, z)


def test_streams_key_words_rows_and_column_groups_are_independent_coins():
    """Two independent fair masks agree on each entry with probability 1/2: the number of agreeing entries is Binomial(n, 1/2), and the
    bound is 5 of its standard deviations.  A draw that ignored the stream word, the upper key word, the row or the column group would
    agree on ALL entries (z = +512 at n = 2^18).
    Observed z: layer 1 vs 2 +1.64, 1 vs 3 +1.42, 1 vs 5 +0.01, key bit 40 -2.43, key bit 0 +1.76, rows +1.65, columns by four -0.49,
    columns by one -1.00."""
    base = pr.keep_mask(S, 1, M, C, 0.5)
    pairs = {
        "layer 1 vs 2": (base, pr.keep_mask(S, 2, M, C, 0.5)),
        "layer 1 vs 3": (base, pr.keep_mask(S, 3, M, C, 0.5)),
        "layer 1 vs 5": (base, pr.keep_mask(S, 5, M, C, 0.5)),
        "upper key word, bit 40": (base, pr.keep_mask(S ^ (1 << 40), 1, M, C, 0.5)),
        "lower key word, bit 0": (base, pr.keep_mask(S ^ 1, 1, M, C, 0.5)),
        "rows shifted by one": (base[1:], base[:-1]),
        "columns shifted by four": (base[:, 4:], base[:, :-4]),
        "columns shifted by one": (base[:, 1:], base[:, :-1]),
    }
    for what, (a, b) in pairs.items():
        z = _z(float((a == b).sum()), a.size, 0.5)
        print(f"{what}: z = {z:+.2f}")
        assert abs(z) < 5.0, (what, z)
    # swapping the row and the column-group counter words would transpose the uniforms of word 0
    k = pr.keep_uniform(S, 1, 16, 64)[:, ::4]
    assert not np.array_equal(k, k.T)


def test_concrete_noise_mean_and_independence_from_the_dropout_streams():
    """Over n = 2^16 rows the mean of a uniform on (0, 1) has standard deviation sqrt(1 / (12 n)) = 0.00113: bound 5 sigma.  Observed
    z = +2.17.  The noise is also no copy of a dropout uniform of the same row."""
    n = 1 << 16
    u = pr.concrete_uniform(S, n).astype(np.float64)
    z = (u.mean() - 0.5) / np.sqrt(1.0 / (12.0 * n))
    print(f"concrete noise mean: z = {z:+.2f}")
    assert abs(z) < 5.0, z
    for layer in (1, 2, 3, 5):
        k = pr.keep_uniform(S, layer, 4096, 4)[:, 0]
        agree = float(((k >= 0.5) == (u[:4096] >= 0.5)).sum())
        assert abs(_z(agree, 4096, 0.5)) < 5.0, layer
    assert not np.array_equal(pr.concrete_uniform(S, 64), pr.concrete_uniform(S ^ (1 << 40), 64))
