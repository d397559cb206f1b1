"""gpu: the agreement of two rankings (gsat_level_overlap / _reset, dp_gsat_amd.level_overlap) against the numpy restatement of
tests/fidelity_multi_oracle.py, exactly: integer counts, entries beyond the valid count never loaded, accumulation, reset, capture."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import fidelity_multi_cases as fc
from tests import fidelity_multi_oracle as fmo
from tests import train_log as tl
from tests.util import assert_no_memset_nodes

pytestmark = pytest.mark.gpu


def _levels(E, S, seed):
    """Two level vectors that agree on about half of their entries; level S (in no level) occurs."""
    rng = np.random.RandomState(31 * E + S + seed)
    a = rng.randint(0, S + 1, size=E).astype(np.uint8)
    b = np.where(rng.rand(E) < 0.5, a, rng.randint(0, S + 1, size=E)).astype(np.uint8)
    return a, b


@pytest.mark.parametrize("E", fc.EDGE_COUNTS)
@pytest.mark.parametrize("S", [1, 5, 16])
def test_counts_equal_the_restatement_and_accumulate(dev, E, S):
    import dp_gsat_amd as G
    from dp_gsat_amd.explain import level_overlap_reset
    a, b = _levels(E, S, 0)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    out = G.level_overlap(da, db, S)
    assert out.dtype == torch.int64 and tuple(out.shape) == (S, 3)
    want = fmo.overlap_counts(a, b, S)
    assert np.array_equal(out.cpu().numpy(), want), (E, S)
    assert np.array_equal(G.level_overlap(da, db, S).cpu().numpy(), want)                    # repeatable
    # entries at or beyond valid[1] hold level 0 -- they would count at every level -- and are never loaded
    real = max(E - 7, 0)
    pa, pb = a.copy(), b.copy()
    pa[real:], pb[real:] = 0, 0
    total = want.copy()
    for k, (x, y) in enumerate(((pa, pb), (pb, pa), (pa, pa))):                              # three appends into the same block
        valid = torch.tensor([3, real, 2, 0], dtype=torch.int32, device=dev)
        assert G.level_overlap(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), S, valid=valid, out=out) is out
        total += fmo.overlap_counts(x, y, S, real)
        assert np.array_equal(out.cpu().numpy(), total), (E, S, k)
    # a count outside [0, E] is clamped; an overflowed batch counts nothing
    for word, count in (([0, E + 9, 0, 0], E), ([0, -4, 0, 0], 0), ([0, E, 0, 1], 0)):
        G.level_overlap(da, db, S, valid=torch.tensor(word, dtype=torch.int32, device=dev), out=out)
        total += fmo.overlap_counts(a, b, S, count)
        assert np.array_equal(out.cpu().numpy(), total), (E, S, word)
    level_overlap_reset(out)
    assert not out.any()


def test_capture_holds_one_kernel_node_and_refusals(dev):
    import dp_gsat_amd as G
    from dp_gsat_amd._lib import GsatHipError
    E, S = 2049, 5
    a, b = _levels(E, S, 1)
    a2, b2 = _levels(E, S, 2)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    valid = torch.tensor([0, E - 3, 0, 0], dtype=torch.int32, device=dev)
    out = torch.zeros(S, 3, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        G.level_overlap(da, db, S, valid=valid, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = tl.kept_debug_graph()
    assert graph is not None, "this torch cannot keep a captured hipGraph for debug_dump"
    with torch.cuda.graph(graph):
        G.level_overlap(da, db, S, valid=valid, out=out)
    path = os.path.join(tempfile.mkdtemp(), "graph.dot")
    graph.debug_dump(path)
    dot = open(path, errors="replace").read()
    assert assert_no_memset_nodes(dot, "gsat_level_overlap") and "memcpy" not in dot.lower()
    nodes = tl.kernel_nodes(dot)
    assert nodes is not None and len(nodes) == 1 and "k_level_overlap" in nodes[0], nodes
    total = fmo.overlap_counts(a, b, S, E - 3)
    graph.replay()
    total = total + fmo.overlap_counts(a, b, S, E - 3)
    da.copy_(torch.from_numpy(a2))
    db.copy_(torch.from_numpy(b2))
    valid.copy_(torch.tensor([0, 1500, 0, 0], dtype=torch.int32))
    graph.replay()
    total = total + fmo.overlap_counts(a2, b2, S, 1500)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), total)
    for bad in (lambda: G.level_overlap(da, db[:-1], S), lambda: G.level_overlap(da, db, 0), lambda: G.level_overlap(da, db, 17),
                lambda: G.level_overlap(da, db.to(torch.int32), S), lambda: G.level_overlap(da, db, S, out=torch.zeros(S, 2, dtype=torch.int64, device=dev)),
                lambda: G.level_overlap(da, db, S, valid=torch.zeros(4, dtype=torch.int64, device=dev))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(GsatHipError):
        G.level_overlap(da.cpu(), db, S)
