"""numpy restatement of Philox4x32-10 (csrc/common.h: philox4x32) and of every draw the kernels make from it, operation for operation.

The key is (low, high) 32-bit word of the 64-bit seed; counter word c3 is always 0x5A17; counter word c2 is the stream:

  stream  draw                                   counter (c0, c1, c2, c3)        device function          restated by
  ------  -------------------------------------  ------------------------------  -----------------------  ----------------------------
  1, 2    extractor dropout, layers 1 / 2        (row, c >> 2, layer, 0x5A17)    philox_keep4             keep_uniform / keep_mask
  3       BatchNorm tail dropout                 (row, c >> 2, 3, 0x5A17)        philox_keep4             keep_uniform / keep_mask
  4       concrete-sampler noise, word x only    (row, 0, 4, 0x5A17)             philox_noise_u           concrete_uniform
  5       Gumbel uniform, entry m = word m & 3   (m >> 2, 0, 5, 0x5A17)          gumbel_uniform4          gumbel_uniform
  5       ReLU+dropout                           (row, c >> 2, 5, 0x5A17)        philox_keep4             keep_uniform / keep_mask

ReLU+dropout and the Gumbel uniform SHARE stream 5.  Under one seed they read the same Philox block: the uniforms behind columns 0..3
of ReLU+dropout row r are the Gumbel uniforms of entries 4r..4r+3, i.e. gumbel_uniform(S, 4 M).reshape(M, 4) ==
keep_uniform(S, 5, M, C)[:, :4].  The callers draw a fresh seed per call, so no training step pairs the two; the stream id stays as it
is because changing it would change every seeded GIN run.  tests/test_philox_ref_host.py pins the overlap."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32(key, c0, c1, c2, c3):
    """Ten rounds on uint32 arrays (or scalars) of one shape; ``key`` = (k0, k1) ints.  Returns the four output words as uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _LO for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def gumbel_uniform(seed, M):
    """float32[M]: U[m] = word m & 3 of philox4x32(seed, m >> 2, 0, 5, 0x5A17), as (float)(word >> 8) * 2^-24 -- in [0, 1)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((int(M) + 3) // 4, dtype=np.uint64)
    words = philox4x32((seed & 0xFFFFFFFF, seed >> 32), q, 0, 5, 0x5A17)
    w = np.stack(words, axis=1).reshape(-1)[:int(M)]
    return ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def keep_uniform(seed, layer, M, C):
    """float32[M, C]: entry [row, c] = word c & 3 of philox4x32(seed, row, c >> 2, layer, 0x5A17), as (float)(word >> 8) * 2^-24 --
    in [0, 1), the number philox_keep4 compares with p.  C must be a multiple of 4 (as in the library)."""
    M, C = int(M), int(C)
    assert C > 0 and C % 4 == 0
    row = np.arange(M, dtype=np.uint64)[:, None]
    grp = np.arange(C // 4, dtype=np.uint64)[None, :]
    words = philox4x32(_key(seed), row, grp, int(layer), 0x5A17)
    w = np.stack(words, axis=2).reshape(M, C)                   # [M, C/4, 4] -> column 4 * group + word
    return ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def keep_mask(seed, layer, M, C, p):
    """float32[M, C] of 0 / 1: keep iff keep_uniform >= p, with p rounded to float32 as the C ABI's ``float`` argument is."""
    return (keep_uniform(seed, layer, M, C) >= np.float32(p)).astype(np.float32)


def concrete_uniform(seed, M):
    """float32[M]: u[row] = ((float)(x >> 9) + 0.5) * 2^-23 with x = word 0 of philox4x32(seed, row, 0, 4, 0x5A17) -- in
    [2^-24, 1 - 2^-24]; x >> 9 < 2^23, so the conversion, the half step and the scaling are all exact in float32."""
    row = np.arange(int(M), dtype=np.uint64)
    x = philox4x32(_key(seed), row, 0, 4, 0x5A17)[0]
    return (((x >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)).astype(np.float32)
