"""not gpu: the numpy Philox restatement against the published Random123 vector, and the two Gumbel-sigmoid symbols in the header, the
ctypes table and the built library."""
import ctypes
import os
import re

import numpy as np

from tests import philox_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"gsat_gumbel_sigmoid_philox": 8, "gsat_philox_gumbel_noise": 4}          # name -> number of arguments


def test_philox_restatement_gives_the_random123_vectors():
    # Random123 kat_vectors, philox4x32 10 rounds: zero counter and key; all-ones counter and key
    got = [int(v) for v in pr.philox4x32((0, 0), 0, 0, 0, 0)]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [hex(v) for v in got]
    f = 0xFFFFFFFF
    got = [int(v) for v in pr.philox4x32((f, f), f, f, f, f)]
    assert got == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD], [hex(v) for v in got]
    # arrays: every lane is the scalar result
    lanes = pr.philox4x32((7, 9), np.arange(5), 0, 5, 0x5A17)
    for i in range(5):
        assert [int(w[i]) for w in lanes] == [int(v) for v in pr.philox4x32((7, 9), i, 0, 5, 0x5A17)]


def test_gumbel_uniform_layout():
    seed = (0xABCDEF12 << 32) | 0x13572468
    u = pr.gumbel_uniform(seed, 11)
    assert u.dtype == np.float32 and u.shape == (11,) and (u >= 0).all() and (u < 1).all()
    for m in (0, 3, 4, 10):
        word = int(pr.philox4x32((0x13572468, 0xABCDEF12), m >> 2, 0, 5, 0x5A17)[m & 3])
        assert u[m] == np.float32(word >> 8) * np.float32(2.0 ** -24)
    assert np.array_equal(pr.gumbel_uniform(seed, 5), u[:5])                        # a prefix does not depend on M
    assert not np.array_equal(pr.gumbel_uniform(seed ^ (1 << 40), 11), u)            # the high key word matters
    assert pr.gumbel_uniform(seed, 0).shape == (0,)


def test_header_signatures_and_library_agree_on_the_new_symbols():
    import __graft_entry__ as ge
    ge.build()
    from dp_gsat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsat_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert decl, f"{name} is not declared in include/gsat_hip.h"
        assert len(decl.group(1).split(",")) == nargs, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported"
    res, args = _lib.SIGNATURES["gsat_gumbel_sigmoid_philox"]
    assert args[4] is ctypes.c_uint64 and args[1] is ctypes.c_int64 and args[2] is ctypes.c_float and args[3] is ctypes.c_float
    assert _lib.SIGNATURES["gsat_philox_gumbel_noise"][1][0] is ctypes.c_uint64
    assert _lib.load().gsat_abi_version() == 4
