"""Seeded inputs of the streamed-extractor tests (tests/test_gpu_attn_stream.py) beyond the table of tests/extractor_cases.py, built the same
way (extractor_cases._finish) and held to the same conditions on the reference alone by tests/test_attn_stream_host.py: every centred
pre-activation at least RELU_MARGIN from the kink of ReLU, and 4 * |r32 - r64| within the regular family's cap.  Edge mode, H = 16,
training, edges grouped by graph."""
import functools

import torch

from tests import extractor_cases as ec
from tests import extractor_oracle as eo
from tests import philox_ref as pr

H = 16
S = (0x9ABCDEF1 << 32) | 0x2468ACE1             # seed of the in-kernel draws, >= 2^63 (as tests/test_gpu_extractor_philox.py)
STAR_LEAVES = 300                               # the centre has 300 entries in both CSRs: above GSAT_LONG_ROW_EDGES = 256


def _sliced():
    """Two graphs of more than 4096 rows each: seg_slices > 1, for the whole batch and for a group that holds one of them."""
    ei, batch, N = ec.sized_batch([1945, 1920], 21)
    rows = torch.bincount(batch[ei[0]], minlength=2).tolist()
    assert all(4096 < r <= 8192 for r in rows), rows
    return ei, batch, N, 2


def _hub():
    """40 rows, a star with 300 leaves (600 rows, every edge in both directions), 12 rows."""
    e0, b0, n0 = ec.edge_sized_batch([40], 31)
    e2, b2, n2 = ec.edge_sized_batch([12], 32)
    c = n0
    leaves = torch.arange(c + 1, c + 1 + STAR_LEAVES)
    centre = torch.full_like(leaves, c)
    star = torch.stack([torch.cat([centre, leaves]), torch.cat([leaves, centre])])
    off = c + 1 + STAR_LEAVES
    ei = torch.cat([e0, star, e2 + off], dim=1)
    batch = torch.cat([b0, torch.full((1 + STAR_LEAVES,), 1, dtype=torch.int64), b2 + 2])
    return ei, batch, off + n2, 3


def _philox():
    base = ec.make_case("regular", "boundaries", True, H, True, sorted_edges=True)
    return base["ei"], base["batch"], base["N"], base["G"]


BUILDERS = {"sliced": (_sliced, 41), "hub": (_hub, 43), "philox": (_philox, 47)}
# the first draw of 0, 1, 2, ... that meets the conditions of tests/test_attn_stream_host.py (found on the CPU reference alone)
REDRAW = {"sliced": 6, "hub": 0, "philox": 1}
# db1 and db2 of the "sliced" case.  A bias in front of an InstanceNorm has a gradient that is exactly 0 in exact arithmetic; the fp64
# reference returns <= 3e-13 there and the library writes exact zeros by construction.  The fp32 reference sums ~4200 cancelling terms
# per graph and is left with 3e-5 .. 9e-5 of rounding noise in every draw, and 4 x that is above the regular cap of 1e-4 -- so for these two tensors of
# this case the slack term is not used at all: the GPU test asserts exact zeros and the host test |r64| <= EXACT_ZERO (stricter than
# the rule, which would allow TOL + slack).
NO_SLACK = {"sliced": ("db1", "db2")}
EXACT_ZERO = 1e-9


@functools.lru_cache(maxsize=None)
def make_stream_case(name, redraw=None):
    build, seed = BUILDERS[name]
    ei, batch, N, G = build()
    c = ec._finish(ei, batch, N, G, H, True, True, seed, REDRAW[name] if redraw is None else redraw)
    if name == "philox":          # the masks and the noise the kernels draw from S themselves, restated in numpy
        _, C1, C2 = ec.widths(True, H)
        c["masks"] = tuple(torch.from_numpy(pr.keep_mask(S, layer, c["M"], C, ec.P_DROP)) for layer, C in ((1, C1), (2, C2)))
        c["u"] = torch.from_numpy(pr.concrete_uniform(S, c["M"]))
    c.update(family="regular", name=name, sorted_edges=True)
    return c


def stream_references(name):
    return eo.references(make_stream_case(name), key=("stream", name))
