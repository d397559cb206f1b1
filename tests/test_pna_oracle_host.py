"""CPU only: the plain PNA reference (tests/pna_oracle.py) against oracle.ops.pna_aggregate under fp64 autograd, its tie rules pinned by
hand, and the premise of the GPU bit comparisons: on the exact recipe a float32 evaluation in any visiting order IS the float64 result."""
import numpy as np
import pytest

from oracle import ops as oops
from tests import pna_oracle as po

AVG = {"lin": 2.5, "log": 1.25}
ALL_SCALERS = ["identity", "amplification", "attenuation", "linear", "inverse_linear"]


def _autograd(x, ei, aggr, scalers, att, na, emb, dout):
    xo = x.double().clone().requires_grad_(True)
    leaf = None if att is None and na is None else (att if att is not None else na).double().view(-1, 1).clone().requires_grad_(True)
    eo = None if emb is None else emb.double().clone().requires_grad_(True)
    w = None if leaf is None else (leaf if att is not None else oops.lift_node_att_to_edge_att(leaf, ei))
    out = oops.pna_aggregate(xo, ei, w, aggr, scalers, AVG, eo)
    out.backward(dout.double())
    return out.detach(), xo.grad, None if leaf is None else leaf.grad.view(-1), None if eo is None else eo.grad


@pytest.mark.parametrize("mode", ["none", "edge", "node"])
@pytest.mark.parametrize("edge_emb", [False, True])
@pytest.mark.parametrize("aggr,scalers", [(po.AGG_ALL, ALL_SCALERS), (po.AGG5, ["identity"]), (["sum", "var"], ["linear", "inverse_linear"])])
def test_reference_agrees_with_the_autograd_oracle(mode, edge_emb, aggr, scalers):
    """Every aggregator and scaler, with and without an edge embedding, edge / lifted node / no attention: out, dx, datt or d node_att
    and dedge within 1e-12 of oracle.ops under fp64 autograd, rows without in-edges included."""
    ei, N = po.row_length_graph()
    H = 12
    inp = po.float_inputs(ei, N, H, 5, edge_emb)
    parts = 3 if edge_emb else 2
    dout = po.float_dout(N, H, aggr, scalers, parts, 6)
    att = inp.att if mode == "edge" else None
    na = inp.na if mode == "node" else None
    want = _autograd(inp.x, ei, aggr, scalers, att, na, inp.emb, dout)
    got = po.pna_reference(inp.x, ei, aggr, scalers, AVG, att=att, node_att=na, edge_emb=inp.emb, dout=dout)
    gatt = got.datt if mode == "edge" else got.dna
    for name, a, b in (("out", got.out, want[0]), ("dx", got.dx, want[1]), ("datt", gatt, want[2]), ("dedge", got.dedge, want[3])):
        assert (a is None) == (b is None), name
        if a is not None:
            err = np.abs(a - b.numpy()).max()
            assert err <= 1e-12 * max(1.0, np.abs(b.numpy()).max()), f"{name}: {err:.3e}"


def _ref(x, src, dst, aggr, att=None, dout=None, **kw):
    ei = np.array([src, dst], dtype=np.int64)
    return po.pna_reference(np.array(x, dtype=np.float64), ei, aggr, ["identity"], AVG, att=None if att is None else np.array(att), dout=dout, **kw)


def test_three_way_tie_goes_to_the_first_edge_not_the_lowest_source():
    """Row 0 has in-edges from 3, 1, 2 in edge order, all with x_j = -1 (node 4, x_j = 5, is the fourth): min ties three ways and its
    gradient reaches node 3, the first edge, only."""
    x = [[7.0], [-1.0], [-1.0], [-1.0], [5.0]]
    dout = np.array([[0.0, 1.0]] + [[0.0, 0.0]] * 4)             # d min, x_j part of row 0
    r = _ref(x, [3, 1, 2, 4], [0, 0, 0, 0], ["min"], dout=dout)
    assert r.out[0].tolist() == [7.0, -1.0]
    assert r.dx[:, 0].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0]


@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_zero_self_feature_routes_to_the_first_edge(zero):
    """x_i = +0 or -0: every att * x_i is a zero, min and max of the x_i part tie on every edge, the gradient goes through the row's
    first edge: dx_i = (g_min + g_max) * att[first], datt = 0 (x_i = 0)."""
    x = [[zero], [1.0], [2.0]]
    att = [0.25, 0.75, 0.5]                                      # edges 1->0, 2->0, 1->0
    dout = np.array([[3.0, 0.0, 5.0, 0.0]] + [[0.0] * 4] * 2)    # [min x_i, min x_j, max x_i, max x_j]
    r = _ref(x, [1, 2, 1], [0, 0, 0], ["min", "max"], att=att, dout=dout)
    assert r.out[0, 0] == 0.0 and r.out[0, 2] == 0.0
    assert r.dx[0, 0] == (3.0 + 5.0) * 0.25
    assert r.datt.tolist() == [0.0, 0.0, 0.0]


def test_negative_self_feature_takes_its_min_at_the_first_largest_attention():
    """x_i = -2, att = (0.5, 1, 0.25, 1): min of att * x_i = -2 at edges 1 and 3, the first wins; max = -0.5 at edge 2."""
    x = [[-2.0], [1.0]]
    att = [0.5, 1.0, 0.25, 1.0]
    dout = np.array([[3.0, 0.0, 5.0, 0.0], [0.0] * 4])
    r = _ref(x, [1, 1, 1, 1], [0, 0, 0, 0], ["min", "max"], att=att, dout=dout)
    assert r.out[0, 0] == -2.0 and r.out[0, 2] == -0.5
    assert r.datt.tolist() == [0.0, 3.0 * -2.0, 5.0 * -2.0, 0.0]
    assert r.dx[0, 0] == 3.0 * 1.0 + 5.0 * 0.25


def test_negative_zero_message_ties_with_positive_zero():
    """Edge 0 carries att = 0 on x_j = -1 (message -0.0), edge 1 carries att = 1 on x_j = +0.0, edge 2 a positive message: min is a zero
    attained first by edge 0; -0.0 does not beat +0.0 either way (edge order 1, 0 gives edge 1)."""
    x = [[4.0], [-1.0], [0.0], [3.0]]
    dout = np.array([[0.0, 1.0]] + [[0.0, 0.0]] * 3)
    r = _ref(x, [1, 2, 3], [0, 0, 0], ["min"], att=[0.0, 1.0, 1.0], dout=dout)
    assert r.out[0, 1] == 0.0
    assert r.datt.tolist() == [-1.0, 0.0, 0.0] and r.dx[:, 0].tolist() == [0.0, 0.0, 1.0 * 0.0 + 0.0, 0.0]      # d att_0 = g * x_j; dx_j = g * att_0 = 0
    r = _ref(x, [2, 1, 3], [0, 0, 0], ["min"], att=[1.0, 0.0, 1.0], dout=dout)
    assert r.datt.tolist() == [0.0, 0.0, 0.0] and r.dx[:, 0].tolist() == [0.0, 0.0, 1.0, 0.0]


def test_empty_row():
    """No in-edges: sum, mean, min, max, var are 0, std is sqrt(1e-5), the row's own gradient is 0 whatever dout holds."""
    x = [[1.5, -2.0], [0.5, 0.25], [1.0, 3.0]]
    dout = np.ones((3, 6 * 4))
    r = _ref(x, [2], [1], po.AGG_ALL, dout=dout)                 # node 0 neither receives nor sends; node 2 sends only
    want = np.zeros(6 * 4)
    want[3 * 4:4 * 4] = np.sqrt(1e-5)
    assert r.out[0].tolist() == want.tolist() and r.out[2].tolist() == want.tolist()
    assert r.dx[0].tolist() == [0.0, 0.0]
    assert r.dx[2].tolist() == [4.0, 4.0]                      # row 2's own part is 0: only the edge's gradient (sum, mean, min, max: 1 each; var, std: 0)
    r0 = _ref(x, [], [], po.AGG_ALL, dout=dout)
    assert r0.dx.tolist() == [[0.0, 0.0]] * 3 and r0.out[1].tolist() == want.tolist()


# ---- the exact recipe is exact -----------------------------------------------------------------------------------------------------------
def _assert_exact(ei, N, inp, aggr, H, mode, dout, what):
    att = inp.att if mode == "edge" else None
    na = inp.na if mode == "node" else None
    kw = dict(att=att, node_att=na, edge_emb=inp.emb, dout=dout)
    r64 = po.pna_reference(inp.x, ei, aggr, ["identity"], AVG, dtype=np.float64, **kw)
    std = [ai for ai, a in enumerate(aggr) if a == "std"]
    F = r64.out.shape[1] // len(aggr)
    live = np.ones(r64.out.shape[1], dtype=bool)
    for ai in std:
        live[ai * F:(ai + 1) * F] = False
    for order in (None, "reverse", 7):
        r32 = po.pna_reference(inp.x, ei, aggr, ["identity"], AVG, dtype=np.float32, order=order, **kw)
        pow2 = (lambda d: (d > 0) & ((d & (d - 1)) == 0))(po.in_degree(ei, N))
        cmp = [("dx", r32.dx, r64.dx), ("datt", r32.datt, r64.datt), ("dna", r32.dna, r64.dna), ("dedge", r32.dedge, r64.dedge)]
        mean = [ai for ai, a in enumerate(aggr) if a == "mean"]
        o32, o64 = r32.out.copy(), r64.out.copy()
        for ai in mean:                                          # the mean output is compared bit for bit on power-of-two rows only
            o32[~pow2, ai * F:(ai + 1) * F] = 0
            o64[~pow2, ai * F:(ai + 1) * F] = 0
        cmp.append(("out", o32[:, live], o64[:, live]))
        for name, a, b in cmp:
            if b is not None:
                assert a.dtype == np.float32
                assert np.array_equal(a.astype(np.float64), b), f"{what} {name}, order {order}: fp32 differs from fp64 by {np.abs(a - b).max():.3e}"


GPU_WIDTHS_A = (4, 12, 16, 32, 64, 72, 80, 100, 128, 132, 256, 260, 336, 512)


@pytest.mark.parametrize("H", GPU_WIDTHS_A)
def test_exact_recipe_is_exact_on_the_row_length_graph(H):
    ei, N = po.row_length_graph()
    for aggr in (po.AGG4, po.AGG5, po.AGG_STAGED):
        for mode in ("none", "edge", "node"):
            for ee in (False, True):
                if mode == "node" and ee:
                    continue
                inp = po.exact_inputs(ei, N, H, 100 + H, edge_emb=ee)
                dout, _ = po.exact_dout(ei, N, H, aggr, ["identity"], 3 if ee else 2, 200 + H)
                _assert_exact(ei, N, inp, aggr, H, mode, dout, f"A H={H} {aggr} {mode} ee={ee}")
    if H in (16, 80):
        inp = po.self_part_inputs(ei, N, H, 300 + H)
        for aggr in (po.AGG4, po.AGG5):
            dout, _ = po.exact_dout(ei, N, H, aggr, ["identity"], 2, 400 + H)
            _assert_exact(ei, N, inp, aggr, H, "edge", dout, f"B H={H}")


@pytest.mark.parametrize("H", (16, 32, 64, 80, 100, 256, 336))
@pytest.mark.parametrize("ee", [False, True])
def test_exact_recipe_is_exact_on_the_hub_graph(H, ee):
    ei, N, _ = po.hub_graph()
    inp = po.hub_exact_inputs(H, 500 + H, edge_emb=ee)
    for aggr in (po.AGG4, po.AGG5, po.AGG_STAGED):
        dout, _ = po.exact_dout(ei, N, H, aggr, ["identity"], 3 if ee else 2, 600 + H)
        for mode in ("none", "edge"):
            _assert_exact(ei, N, inp, aggr, H, mode, dout, f"C H={H} {aggr} {mode} ee={ee}")
    ei1, N1 = po.one_chunk_graph()
    inp = po.exact_inputs(ei1, N1, H, 700 + H, edge_emb=ee)
    dout, _ = po.exact_dout(ei1, N1, H, po.AGG5, ["identity"], 3 if ee else 2, 800 + H)
    _assert_exact(ei1, N1, inp, po.AGG5, H, "edge", dout, f"C one chunk H={H}")


@pytest.mark.parametrize("H", (8, 12, 16, 32, 48, 72, 100, 132))
def test_exact_recipe_is_exact_on_the_window_graph(H):
    ei, _, N = po.window_graph()
    inp = po.exact_inputs(ei, N, H, 900 + H, pool=2)
    for aggr in (po.AGG4, po.AGG5):
        dout, _ = po.exact_dout(ei, N, H, aggr, ["identity"], 2, 1000 + H)
        for mode in ("edge", "node"):
            _assert_exact(ei, N, inp, aggr, H, mode, dout, f"F H={H} {aggr} {mode}")


def test_exact_recipe_is_exact_on_the_window_size_graphs():
    """Case E: the ring and path graphs of tests/test_gpu_pna_tile_keep.py (in-degrees 0, 1, 2) at their widths, the added dx_add and
    existing d node_att included."""
    from tests.test_gpu_pna_tile_keep import CASES, _graph
    for name, (H, _, planned) in CASES.items():
        ei, _, N, _ = _graph(H, planned)
        aggr = po.AGG5 if H == 80 else po.AGG4
        inp = po.exact_inputs(ei, N, H, 1100 + H + planned % 7)
        dout, _ = po.exact_dout(ei, N, H, aggr, ["identity"], 2, 1200 + H)
        for mode in ("edge", "node"):
            _assert_exact(ei, N, inp, aggr, H, mode, dout, f"E {name} {mode}")
            kw = dict(att=inp.att) if mode == "edge" else dict(node_att=inp.na)
            r32, r64 = (po.pna_reference(inp.x, ei, aggr, ["identity"], AVG, dout=dout, dtype=dt, **kw) for dt in (np.float32, np.float64))
            assert np.array_equal((r32.dx + inp.dx_add.numpy()).astype(np.float64), r64.dx + inp.dx_add.double().numpy()), f"{name}: dx + dx_add"
            if mode == "node":
                assert np.array_equal((r32.dna + inp.dna0.numpy()).astype(np.float64), r64.dna + inp.dna0.double().numpy()), f"{name}: dna + dna0"


def test_hub_inputs_place_the_ties_where_the_chunks_meet():
    """The plan of hub_exact_inputs holds: per hub row the x_j maximum of a group-0 channel is attained at slot 3 and in a later chunk,
    of a group-1 channel only at the last slot, and the att minimum 0 twice."""
    ei, N, slots = po.hub_graph()
    H = 16
    inp = po.hub_exact_inputs(H, 500 + H)
    x, att, src = inp.x.numpy(), inp.att.numpy(), ei[0].numpy()
    for r, sl in slots.items():
        d = len(sl)
        m = att[sl, None] * x[src[sl]]
        for c in range(H):
            top = np.nonzero(np.abs(m[:, c]) == np.abs(m[:, c]).max())[0]
            if c % 3 == 0:
                assert top.tolist() == [3, 300 if d > 300 else 200] and abs(m[3, c]) == 2.0
            if c % 3 == 1:
                assert top.tolist() == [d - 1] and abs(m[d - 1, c]) == 2.0
        assert (att[sl] == 0).sum() == 2 and att[sl].min() == 0
    assert sorted(len(s) for s in slots.values()) == sorted(po.HUB_DEGREES)
