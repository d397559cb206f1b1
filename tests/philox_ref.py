"""numpy restatement of Philox4x32-10 (csrc/common.h: philox4x32) and of the uniform the Gumbel-sigmoid sampler draws from it
(Philox stream 5, csrc/edgeops.hip: gumbel_uniform4)."""
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
