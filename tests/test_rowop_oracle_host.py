"""The row-operator references of tests/rowop_oracle.py against the oracle's operators under torch autograd in fp64 (what makes them
trustworthy), the premise of the bitwise GPU assertions -- under the exact recipe an fp32 sum in any order is the fp64 result -- checked
without a kernel at the largest degree and width the GPU tests use, and hand-written cases for the conventions a formula leaves open."""
import pytest
import torch

from oracle import ops as oops
from tests import rowop_oracle as ro


def _rel(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max())) if a.numel() else 0.0


def _batches():
    ei, N = ro.small_graph()
    g = torch.Generator().manual_seed(3)
    ei2 = torch.randint(0, 23, (2, 70), generator=g)
    return [(ei, N), (ei2, 23)]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("variant", ["gin", "gin_att", "gine", "gine_att"])
def test_aggregation_reference_matches_oracle_autograd(which, variant):
    ei, N = _batches()[which]
    E, H = ei.shape[1], 12
    g = torch.Generator().manual_seed(17 + which)
    x = torch.randn(N, H, generator=g, dtype=torch.float64).requires_grad_(True)
    att = torch.rand(E, 1, generator=g, dtype=torch.float64).requires_grad_(True) if variant.endswith("att") else None
    ee = torch.randn(E, H, generator=g, dtype=torch.float64).requires_grad_(True) if variant.startswith("gine") else None
    dout = torch.randn(N, H, generator=g, dtype=torch.float64)
    eps = 0.5
    out = oops.gine_aggregate(x, ei, ee, att, eps) if ee is not None else oops.gin_aggregate(x, ei, att, eps)
    out.backward(dout)
    rp, col, eid = ro.csr(ei, N, 1)
    ref, abs_sum = ro.aggr_sum(x.detach(), None, None if att is None else att.detach(), None if ee is None else ee.detach(), rp, col, eid,
                               1 + eps)
    assert _rel(ref, out.detach()) <= 1e-12
    assert (abs_sum >= ref.abs() - 1e-12).all()
    rps, dst, eids = ro.csr(ei, N, 0)
    b = ro.aggr_sum_bwd(x.detach(), None if att is None else att.detach(), None if ee is None else ee.detach(), dout, rps, dst, eids,
                        1 + eps)
    assert _rel(b.dx, x.grad) <= 1e-12
    assert (b.dx_abs >= b.dx.abs() - 1e-12).all() and (b.datt_abs >= b.datt.abs() - 1e-12).all()
    if att is not None:
        assert _rel(b.datt, att.grad.view(-1)) <= 1e-12
    if ee is not None:
        assert _rel(b.dedge_emb, ee.grad) <= 1e-12
    else:
        assert b.dedge_emb is None


def test_datt_without_attention_is_the_message_dot_product():
    ei, N = ro.small_graph()
    inp = ro.rowop_inputs(N, ei.shape[1], 8, "float")
    rps, dst, eids = ro.csr(ei, N, 0)
    b = ro.aggr_sum_bwd(inp.x, None, None, inp.dout, rps, dst, eids, 1.0)
    want = (inp.x.double()[ei[0]] * inp.dout.double()[ei[1]]).sum(1)
    assert _rel(b.datt, want) <= 1e-12


@pytest.mark.parametrize("which", [0, 1])
def test_pool_lift_symmetrise_references_match_oracle_autograd(which):
    ei, N = _batches()[which]
    E, H = ei.shape[1], 8
    g = torch.Generator().manual_seed(5 + which)
    lengths = torch.tensor([0, 3, 1, 0, N - 4, 0])
    ptr = torch.zeros(7, dtype=torch.int64)
    ptr[1:] = torch.cumsum(lengths, 0)
    batch = torch.repeat_interleave(torch.arange(6), lengths)
    for mean in (0, 1):
        x = torch.randn(N, H, generator=g, dtype=torch.float64).requires_grad_(True)
        dout = torch.randn(6, H, generator=g, dtype=torch.float64)
        out = (oops.global_mean_pool if mean else oops.global_add_pool)(x, batch, 6)
        out.backward(dout)
        assert _rel(ro.segment_pool(x.detach(), ptr, mean), out.detach()) <= 1e-12
        assert _rel(ro.segment_pool_bwd(dout, ptr, mean), x.grad) <= 1e-12
    a = torch.rand(N, 1, generator=g, dtype=torch.float64).requires_grad_(True)
    d = torch.randn(E, 1, generator=g, dtype=torch.float64)
    e = oops.lift_node_att_to_edge_att(a, ei)
    e.backward(d)
    assert _rel(ro.lift(a.detach(), ei[0], ei[1]), e.detach().view(-1)) <= 1e-12
    assert _rel(ro.lift_bwd(a.detach(), d, ei[0], ei[1]), a.grad.view(-1)) <= 1e-12
    rev = ro.involution(E, 9, 3)
    assert torch.equal(rev[rev], torch.arange(E)) and int((rev == torch.arange(E)).sum()) >= 3
    att = torch.rand(E, generator=g, dtype=torch.float64).requires_grad_(True)
    s = oops.symmetrise(att, rev)
    s.backward(d.view(-1))
    assert _rel(ro.symmetrise(att.detach(), rev), s.detach()) <= 1e-12
    assert _rel(ro.symmetrise(d, rev), att.grad) <= 1e-12            # an involution: the operator is its own backward
    assert torch.equal(ro.symmetrise(att.detach(), rev, flag=0), att.detach())


@pytest.mark.parametrize("prior", ["scalar", "tensor"])
def test_info_loss_reference_matches_oracle_autograd(prior):
    M = 300
    att, pr = ro.info_att(M, M)
    r = pr.double() if prior == "tensor" else 0.6
    a = att.double().requires_grad_(True)
    loss = oops.info_loss(a, r)
    (loss * 1.7).backward()
    loss = loss.detach()
    got, scale = ro.info_loss(att, r)
    assert abs(float(got - loss)) <= 1e-12 * max(1.0, abs(float(loss))) and float(scale) >= abs(float(got))
    assert _rel(ro.info_loss_bwd(att, r, 1.7), a.grad) <= 1e-12
    cut, _ = ro.info_loss(att, r, 120)
    want = oops.info_loss(att[:120].double(), r[:120] if prior == "tensor" else r)
    assert abs(float(cut - want)) <= 1e-12
    assert not ro.info_loss_bwd(att, r, 1.7, 120)[120:].any()
    assert float(ro.info_loss(att, r, -3)[0]) == 0.0 and ro.info_counted(M + 9, M) == M


def test_encoder_references():
    dims = ro.table_dims(3)                                   # 5, 3, 7
    W = torch.arange(15 * 4, dtype=torch.float32).view(15, 4)
    x = torch.tensor([[0, 0, 0], [4, 2, 6], [-1, 3, 7], [2, -5, 100]])
    out = ro.embsum(x, dims, W)
    want = torch.stack([W[0] + W[5] + W[8], W[4] + W[7] + W[14], W[0] + W[7] + W[14], W[2] + W[5] + W[14]]).double()
    assert torch.equal(out, want)
    O = ro.onehot_rows(x, dims, 16)
    assert torch.equal(O.sum(1), torch.full((4,), 3.0)) and not O[:, 15].any()
    assert O[2, 0] == 1 and O[2, 7] == 1 and O[2, 14] == 1
    assert torch.equal(O[:, :15].double() @ W.double(), out)
    t = torch.tensor([10, 11, 12])
    assert ro.gather_clamped(t, torch.tensor([-1, 0, 2, 3])).tolist() == [10, 10, 12, 12]


# ---- the premise of the bitwise GPU assertions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("gine", [False, True])
def test_exact_recipe_is_order_independent_in_fp32(gine):
    """Degree 1300 at width 2048: the fp32 evaluation in forward, reversed and a seeded random edge (and column) order is the fp64 result
    cast to fp32, bit for bit -- for out, dx, datt and dedge_emb."""
    d, H = max(ro.HUB_DEGREES), max(ro.WIDTHS)
    ei = torch.cat([ro.star_graph(d)[0], ro.star_graph(d, True)[0]], 1)          # node 0: in- and out-degree 1300
    N, E = d + 1, 2 * d
    inp = ro.rowop_inputs(N, E, H, "exact")
    ee = inp.edge_emb if gine else None
    rp, col, eid = ro.csr(ei, N, 1)
    rps, dst, eids = ro.csr(ei, N, 0)
    assert int((rp[1:] - rp[:-1]).max()) == d and int((rps[1:] - rps[:-1]).max()) == d
    out64, _ = ro.aggr_sum(inp.x, None, inp.att, ee, rp, col, eid, 1.5)
    b64 = ro.aggr_sum_bwd(inp.x, inp.att, ee, inp.dout, rps, dst, eids, 1.5)
    assert float(out64.abs().max()) > 100 and float(b64.datt.abs().max()) > 100          # the sums are not trivially small
    g = torch.Generator().manual_seed(1)
    orders = [(None, None), (torch.arange(E).flip(0), torch.arange(H).flip(0)), (torch.randperm(E, generator=g), torch.randperm(H, generator=g))]
    for order, col_order in orders:
        out32, _ = ro.aggr_sum(inp.x, None, inp.att, ee, rp, col, eid, 1.5, torch.float32, order)
        assert out32.dtype == torch.float32 and torch.equal(out32, out64.float())
        b32 = ro.aggr_sum_bwd(inp.x, inp.att, ee, inp.dout, rps, dst, eids, 1.5, torch.float32, order, col_order)
        assert torch.equal(b32.dx, b64.dx.float()) and torch.equal(b32.datt, b64.datt.float())
        if gine:
            assert torch.equal(b32.dedge_emb, b64.dedge_emb.float())
    for t in (out64, b64.dx, b64.datt):
        assert torch.equal(t.float().double(), t) and torch.equal(t * 8, (t * 8).round())          # multiples of 1/8, exact in fp32


def test_graph_recipes():
    ei, N = ro.small_graph()
    assert N == 40 and ei.shape[1] <= 256
    for by in (0, 1):
        deg = torch.bincount(ei[by], minlength=N)
        assert set(range(6)) <= set(deg.tolist()), (by, sorted(set(deg.tolist())))
    assert int((ei[0] == ei[1]).sum()) >= 3
    pairs = (ei[0] * N + ei[1]).tolist()
    assert len(set(pairs)) == len(pairs) - 1                       # exactly one duplicate edge
    assert not torch.equal(torch.sort(ei[1], stable=True).values, ei[1])          # edge ids are shuffled
    assert ro.small_graph(3)[0].shape[1] > 256
    ei, N = ro.hubs_graph()
    assert N == 1400 and ei.shape[1] > 256
    for by in (0, 1):
        deg = torch.bincount(ei[by], minlength=N)
        assert deg[:9].tolist() == list(ro.HUB_DEGREES) and int(deg[9:].max()) <= 9 and int((deg == 0).sum()) >= 10
        assert ro.chunk_counts(ro.csr(ei, N, by)[0])[:9].tolist() == [0, 0, 2, 2, 2, 2, 2, 3, 6]
    assert len(set((ei[0] * N + ei[1]).tolist())) == ei.shape[1]          # stars to distinct leaves
    ei, N = ro.ring_graph(65540)
    assert torch.equal(torch.bincount(ei[1], minlength=N), torch.full((N,), 2)) and ei.shape[1] == 2 * N
    assert [ro.row_geom(H) for H in ro.WIDTHS] == [(4, 1), (4, 1), (8, 1), (8, 1), (16, 1), (16, 1), (32, 1), (32, 1), (64, 1), (64, 1),
                                                   (64, 2), (64, 2), (64, 4), (64, 4), (64, 8), (64, 8)]


# ---- conventions pinned by hand --------------------------------------------------------------------------------------------------------
def test_relu_tie_gives_no_gradient():
    """Three nodes, edges 0 -> 1 and 2 -> 1; x[0] + e[0] == 0 exactly: the message is 0 and neither dx[0] nor dedge_emb[0] get dout."""
    ei = torch.tensor([[0, 2], [1, 1]])
    x = torch.tensor([[1.0, -2.0], [0.0, 0.0], [1.0, 1.0]])
    ee = torch.tensor([[-1.0, 3.0], [1.0, 1.0]])
    dout = torch.tensor([[0.0, 0.0], [5.0, 7.0], [0.0, 0.0]])
    rp, col, eid = ro.csr(ei, 3, 1)
    out, _ = ro.aggr_sum(x, None, None, ee, rp, col, eid, 0.0)
    assert out.tolist() == [[0, 0], [2, 3], [0, 0]]
    rps, dst, eids = ro.csr(ei, 3, 0)
    b = ro.aggr_sum_bwd(x, None, ee, dout, rps, dst, eids, 0.0)
    assert b.dx.tolist() == [[0, 7], [0, 0], [5, 7]]
    assert b.dedge_emb.tolist() == [[0, 7], [5, 7]]
    assert b.datt.tolist() == [7.0, 24.0]


def test_lift_bwd_counts_a_self_loop_twice():
    a = torch.tensor([0.5, 2.0, 1.0])
    src, dst = torch.tensor([0, 1]), torch.tensor([0, 2])          # a self loop at 0, 1 -> 2
    d = torch.tensor([3.0, 4.0])
    assert ro.lift(a, src, dst).tolist() == [0.25, 2.0]
    assert ro.lift_bwd(a, d, src, dst).tolist() == [3.0, 4.0, 8.0]          # d(a0^2) = 2 a0 d = 3


def test_empty_segment_pools_to_zero():
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    ptr = torch.tensor([0, 0, 2, 2, 3])
    assert ro.segment_pool(x, ptr, 0).tolist() == [[0, 0], [4, 6], [0, 0], [5, 6]]
    assert ro.segment_pool(x, ptr, 1).tolist() == [[0, 0], [2, 3], [0, 0], [5, 6]]
    dout = torch.tensor([[9.0, 9.0], [2.0, 4.0], [9.0, 9.0], [1.0, 1.0]])
    assert ro.segment_pool_bwd(dout, ptr, 1).tolist() == [[1, 2], [1, 2], [1, 1]]
    assert ro.segment_pool_bwd(dout, ptr, 0).tolist() == [[2, 4], [2, 4], [1, 1]]
