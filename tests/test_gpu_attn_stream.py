"""-m gpu: the memory-bounded extractor through the C ABI (gsat_attn_stream_fwd / gsat_attn_stream_bwd, csrc/attn_stream.h) against the fp64
reference of tests/extractor_oracle.py, by the rule of tests/test_gpu_extractor_paths.py: close64 with the caps of
extractor_cases.cap_for, every output NaN-prefilled and checked for leftovers, the run stopped at the first HIP error.  No a1 buffer and
no row order is passed: all forward tensors except a1, and all seven gradients, are compared."""
import ctypes

import pytest
import torch

from tests import attn_stream_cases as sc
from tests import extractor_cases as ec
from tests import extractor_oracle as eo
from tests.attn_stream_driver import run_stream, verdict

pytestmark = pytest.mark.gpu

FWD = tuple(k for k in ec.FWD_TENSORS if k != "a1")
OUTPUTS = ("logits", "att", "P", "Q", "h2", "stats", "demb", "dW1", "db1", "dW2", "db2", "dW3", "db3")


def _compare(out, refs, what, no_slack=()):
    r32, r64 = refs
    for k in OUTPUTS:
        assert not torch.isnan(out[k]).any(), f"{what}: {k} has unwritten (NaN) entries"
    for k in FWD + ec.GRAD_TENSORS:
        if k in ("var1", "var2"):          # the library saves 1/sigma: compare var + eps (as tests/test_gpu_extractor_paths.py)
            a, b32, b64 = out["rstd" + k[-1]].double() ** -2, r32[k] + eo.EPS, r64[k] + eo.EPS
        else:
            a, b32, b64 = out[k], r32[k], r64[k]
        if k in no_slack:                  # attn_stream_cases.NO_SLACK: exact zeros against an fp64 reference within EXACT_ZERO of 0
            assert not bool(a.any()) and float(b64.abs().max()) <= sc.EXACT_ZERO, f"{what}: {k}"
            continue
        eo.close64(a.reshape(b64.shape), b32, b64, f"{what}: {k}", ec.cap_for("regular", k))
    assert not bool(out["db1"].any()) and not bool(out["db2"].any()), "a bias in front of an InstanceNorm has an exactly zero gradient"


@pytest.mark.parametrize("budget,groups", [(1, [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12]), (64, [0, 3, 4, 5, 6, 7, 8, 10, 12]), (200, [0, 5, 7, 8, 10, 12]),
                                           (10 ** 6, [0, 12])])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("H", [16, 80])
def test_boundary_graphs_at_every_budget(dev, H, training, budget, groups):
    """Rows per graph 4, 5, 32, 33, 64, 65, 128, 129, 257, 0, 12, 40.  Budget 1: every graph alone (the empty one joins the graph in
    front of it); 64: groups that close exactly at 64, and oversize graphs; 200; 10^6: one group."""
    case = ec.make_case("regular", "boundaries", True, H, training, sorted_edges=True)
    out = run_stream(dev, case, budget)
    assert out["plan"].groups() == groups
    assert out["plan"].scratch_rows == (769 if budget == 10 ** 6 else 257)
    _compare(out, eo.references(case), f"boundaries H={H} train={training} budget={budget}")
    lone = case["batch"] == 9                                  # the graph without edges: its node still owns a row of demb
    assert int(lone.sum()) == 1 and not bool(out["demb"][lone.to(dev)].any()), "demb of a graph with nodes but no edges is exactly zero"


@pytest.mark.parametrize("budget,groups", [(4500, [0, 1, 2]), (10 ** 4, [0, 2])])
def test_sliced_statistics(dev, budget, groups):
    """Two graphs of more than 4096 rows: a group of one of them takes its layer-1 statistics, forward and backward, in two slices per
    graph and its activation and dh1 from the elementwise kernels; so does the one group of both."""
    case = sc.make_stream_case("sliced")
    out = run_stream(dev, case, budget)
    assert out["plan"].groups() == groups
    _compare(out, sc.stream_references("sliced"), f"sliced budget={budget}", no_slack=sc.NO_SLACK["sliced"])


def test_hub_rows_stay_chunked_in_a_group_of_their_own(dev):
    """40 rows, a star of 300 leaves, 12 rows at budget 100: the star is the second group, its centre is a long row of both CSRs, and its
    chunks are items [chunk_ptr[n0], chunk_ptr[n1]) of the batch's table -- a chunk base of 0 would sum the wrong partials."""
    case = sc.make_stream_case("hub")
    out = run_stream(dev, case, 100)
    assert out["plan"].groups() == [0, 1, 2, 3] and out["plan"].scratch_rows == 600
    assert out["hubs"] == (True, True), "the batch has no long row: the chunked gather did not run"
    _compare(out, sc.stream_references("hub"), "hub budget=100")
    one = run_stream(dev, case, 10 ** 6)             # the star in the middle of one group: its rows start at scratch row 40
    _compare(one, sc.stream_references("hub"), "hub, one group")


def test_in_kernel_philox_is_keyed_by_the_global_row(dev):
    """No mask and no noise tensor, the seed by value >= 2^63; the reference is fed the numpy restatement of the draws
    (tests/philox_ref.py) for GLOBAL rows.  With several groups a group-local row key would draw other masks from the second group on."""
    case = sc.make_stream_case("philox")
    assert sc.S >= 1 << 63
    out = run_stream(dev, case, 64, philox_seed=sc.S)
    assert out["plan"].n_groups == 8
    _compare(out, sc.stream_references("philox"), "philox budget=64")


def test_a_batch_without_edges(dev):
    """M == 0: three graphs of one node each.  One group of only empty graphs, a scratch of one row, nothing to write forward, every
    gradient exactly zero."""
    case = dict(ec._finish(torch.zeros(2, 0, dtype=torch.int64), torch.arange(3), 3, 3, 16, True, True, 1), family="regular", name="empty")
    assert case["M"] == 0
    out = run_stream(dev, case, 64)
    assert out["plan"].groups() == [0, 3] and out["plan"].scratch_rows == 1
    for k in ec.GRAD_TENSORS:
        assert out[k].numel() > 0 and not torch.isnan(out[k]).any() and not bool(out[k].any()), k


def test_two_runs_with_one_plan_are_bitwise_equal(dev):
    case = sc.make_stream_case("hub")
    a, b = run_stream(dev, case, 100), run_stream(dev, case, 100)
    for k in OUTPUTS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k} differs between two runs"
    case = ec.make_case("regular", "boundaries", True, 80, True, sorted_edges=True)
    a, b = run_stream(dev, case, 64), run_stream(dev, case, 64)
    for k in OUTPUTS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k} differs between two runs"


def test_node_mode_is_unsupported_and_the_check_names_the_fault(dev):
    from dp_gsat_amd import _lib
    from tests.graphs import shuffle_edges
    lib = _lib.load()
    a = _lib.AttnArgs()
    a.M, a.N, a.G, a.H, a.C1, a.C2, a.edge_mode = 8, 8, 1, 16, 32, 16, 0
    one = (ctypes.c_int32 * 2)(0, 1)
    seg = (ctypes.c_int32 * 2)(0, 8)
    GSAT_ERR_UNSUPPORTED = -4          # include/gsat_hip.h
    assert lib.gsat_attn_stream_fwd(ctypes.byref(a), one, 1, seg, seg, 8, None) == GSAT_ERR_UNSUPPORTED
    g = _lib.AttnGrads()
    g.demb = g.dW1 = g.db1 = g.dW2 = g.db2 = g.dW3 = g.db3 = 8          # placeholders: the mode is refused before anything is read
    assert lib.gsat_attn_stream_bwd(ctypes.byref(a), ctypes.byref(g), one, 1, seg, seg, 8, None) == GSAT_ERR_UNSUPPORTED
    case = ec.make_case("regular", "boundaries", True, 16, True, sorted_edges=True)
    ei, batch, G = case["ei"], case["batch"], case["G"]
    assert verdict(dev, ei, batch, G) == 0
    assert verdict(dev, shuffle_edges(ei, 3), batch, G) == 1, "shuffled edges: the rows are not grouped by graph"
    cross = ei.clone()
    cross[1, 0] = int((batch == 2).nonzero()[0])          # the first edge of graph 0 now ends in graph 2
    assert verdict(dev, cross, batch, G) == 2, "an edge between two graphs"
    with pytest.raises(ValueError, match="edge order"):
        run_stream(dev, dict(case, ei=shuffle_edges(ei, 3)), 64)
    with pytest.raises(ValueError, match="between two graphs"):
        run_stream(dev, dict(case, ei=cross), 64)
