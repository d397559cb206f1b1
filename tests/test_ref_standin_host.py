"""not gpu: the recording stand-in (oracle/standin/) against dense Python loops on tiny graphs.

The stand-in supplies the third-party names the reference imports when oracle/record_reference.py records tests/golden/ref_*.  These
tests keep it from becoming a restatement nobody checks: scatter, propagate, InstanceNorm, the edge utilities and the encoders are
compared with loops over edges and rows that share no code with it (nor with oracle/ops.py).  The stand-in is on sys.path for this
module's tests only and is taken out of sys.path and sys.modules afterwards; where a real package of one of its names is installed the
tests skip, as the recorder refuses to use it there."""
import importlib.util
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "oracle", "standin")
NAMES = ("_placeholder", "torch_scatter", "torch_sparse", "torch_geometric", "ogb")


@pytest.fixture(scope="module")
def standin():
    """The stand-in packages, imported with oracle/standin first on sys.path and removed from sys.path / sys.modules afterwards."""
    for name in NAMES[1:]:
        if name in sys.modules or importlib.util.find_spec(name) is not None:
            pytest.skip(f"a real {name} is installed: the stand-in is not used on this machine")
    before = set(sys.modules)
    sys.path.insert(0, STANDIN)
    try:
        import torch_geometric.nn as tgnn
        import torch_geometric.nn.conv as conv
        import torch_geometric.utils as tgu
        import torch_scatter
        import torch_sparse
        from ogb.graphproppred.mol_encoder import AtomEncoder, BondEncoder
        yield dict(nn=tgnn, conv=conv, utils=tgu, scatter=torch_scatter.scatter, transpose=torch_sparse.transpose,
                   AtomEncoder=AtomEncoder, BondEncoder=BondEncoder)
    finally:
        sys.path.remove(STANDIN)
        for name in set(sys.modules) - before:
            if name.split(".")[0] in NAMES:
                del sys.modules[name]


def _graph(seed, N=9, E=20, empty=(2, 7)):
    """Random directed edges (no duplicates) on N nodes; the nodes in ``empty`` receive none, node 0 exactly one."""
    g = torch.Generator().manual_seed(seed)
    pairs = set()
    while len(pairs) < E:
        a, b = (int(t) for t in torch.randint(0, N, (2,), generator=g))
        if a != b and b not in empty and (b != 0 or not any(q == 0 for _, q in pairs)):
            pairs.add((a, b))
    pairs = sorted(pairs, key=lambda p: hash((p, seed)))
    return torch.tensor(pairs, dtype=torch.int64).t().contiguous(), N


@pytest.mark.parametrize("reduce", ["sum", "add", "mean", "min", "max"])
def test_scatter_equals_a_loop(standin, reduce):
    ei, N = _graph(1)
    g = torch.Generator().manual_seed(2)
    src = torch.randn(ei.shape[1], 3, dtype=torch.float64, generator=g).requires_grad_(True)
    cot = torch.randn(N, 3, dtype=torch.float64, generator=g)
    out = standin["scatter"](src, ei[1], 0, None, N, reduce=reduce)
    out.backward(cot)
    want, want_grad = torch.zeros(N, 3, dtype=torch.float64), torch.zeros_like(src)
    for i in range(N):
        rows = [e for e in range(ei.shape[1]) if int(ei[1, e]) == i]
        if not rows:
            continue                                                  # a row nothing arrives at stays 0
        for c in range(3):
            vals = [float(src.detach()[e, c]) for e in rows]
            if reduce in ("sum", "add", "mean"):
                k = len(rows) if reduce == "mean" else 1
                want[i, c] = math.fsum(vals) / k
                for e in rows:
                    want_grad[e, c] = cot[i, c] / k
            else:
                pick = min(range(len(rows)), key=lambda j: vals[j]) if reduce == "min" else max(range(len(rows)), key=lambda j: vals[j])
                want[i, c] = vals[pick]
                want_grad[rows[pick], c] = cot[i, c]
    assert torch.allclose(out, want, rtol=0, atol=1e-14)
    assert torch.allclose(src.grad, want_grad, rtol=0, atol=1e-14)
    assert bool((out[[2, 7]] == 0).all())
    assert standin["scatter"](src.detach(), ei[1], 0, reduce=reduce).shape[0] == int(ei[1].max()) + 1      # dim_size defaults to max + 1
    wide = standin["scatter"](src.detach().t().contiguous(), ei[1], -1, None, N, reduce=reduce)            # the last dimension, 1-D index
    assert torch.equal(wide.t(), out.detach())


def test_degree_sort_transpose_is_undirected(standin):
    u, ei = standin["utils"], _graph(3)[0]
    N = 9
    deg = u.degree(ei[1], N, dtype=torch.float64)
    assert deg.tolist() == [float(sum(1 for e in range(ei.shape[1]) if int(ei[1, e]) == i)) for i in range(N)]
    assert u.degree(ei[1]).shape[0] == int(ei[1].max()) + 1
    vals = torch.arange(ei.shape[1], dtype=torch.float64) * 1.5
    sei, sv = u.sort_edge_index(ei, vals)
    order = sorted(range(ei.shape[1]), key=lambda e: (int(ei[0, e]), int(ei[1, e])))
    assert torch.equal(sei, ei[:, order]) and torch.equal(sv, vals[order])
    tei, tv = standin["transpose"](ei, vals, None, None, coalesced=False)
    assert torch.equal(tei, ei.flip(0)) and tv is vals                                   # swapped rows, nothing moved
    assert not u.is_undirected(ei)
    both = torch.cat([ei, ei.flip(0)], dim=1)
    both = both[:, torch.randperm(both.shape[1], generator=torch.Generator().manual_seed(4))]
    assert u.is_undirected(both)
    assert not u.is_undirected(both[:, 1:])


def test_propagate_gathers_by_suffix_and_aggregates_at_the_target(standin):
    """x_j = x[edge_index[0]], x_i = x[edge_index[1]], a pair gives (source side, target side), other arguments pass through by name
    with their defaults, the sum lands on edge_index[1] with one row per node (empty rows 0)."""
    conv = standin["conv"]
    ei, N = _graph(5)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(N, 4, dtype=torch.float64, generator=g)
    a, b = torch.randn(N, 4, dtype=torch.float64, generator=g), torch.randn(N, 4, dtype=torch.float64, generator=g)
    w = torch.rand(ei.shape[1], 1, dtype=torch.float64, generator=g)

    class Layer(conv.MessagePassing):
        def __init__(self, **kw):
            super().__init__(**kw)

        def message(self, x_j, a_j, b_i, weight, shift=0.25):
            return (x_j + a_j - b_i) * weight + shift

    out = Layer(aggr="add", node_dim=0).propagate(ei, x=(x, None), a=a, b=b, weight=w, unused=1)
    want = torch.zeros(N, 4, dtype=torch.float64)
    for e in range(ei.shape[1]):
        s, d = int(ei[0, e]), int(ei[1, e])
        want[d] += (x[s] + a[s] - b[d]) * w[e] + 0.25
    assert out.shape == (N, 4) and torch.allclose(out, want, rtol=0, atol=1e-14)
    assert bool((out[[2, 7]] == 0).all())
    with pytest.raises(TypeError):
        Layer(aggr="add", node_dim=0).propagate(ei, x=x, a=a, b=b)                    # `weight` has no default

    class Own(conv.MessagePassing):                                                   # aggr=None: the layer's own aggregate, as PNAConvSimple
        def message(self, x_i, x_j):
            return torch.cat([x_i, x_j], dim=-1)

        def aggregate(self, inputs, index, dim_size=None):
            return inputs.new_zeros(dim_size, inputs.shape[1]).index_add_(0, index, inputs) * 2

    out = Own(aggr=None, node_dim=0).propagate(ei, x=x, size=None)
    want = torch.zeros(N, 8, dtype=torch.float64)
    for e in range(ei.shape[1]):
        s, d = int(ei[0, e]), int(ei[1, e])
        want[d] += 2 * torch.cat([x[d], x[s]])
    assert torch.allclose(out, want, rtol=0, atol=1e-14)


def test_conv_bases_keep_pyg_parameter_names(standin):
    conv, nn = standin["conv"], torch.nn
    mlp = lambda: nn.Sequential(nn.Linear(6, 6), nn.BatchNorm1d(6), nn.ReLU(), nn.Linear(6, 6))
    gin = conv.GINConv(mlp())
    assert "eps" in dict(gin.named_buffers()) and "eps" not in dict(gin.named_parameters()) and float(gin.eps) == 0.0
    assert "eps" in dict(conv.GINConv(mlp(), train_eps=True).named_parameters())
    gine = conv.GINEConv(mlp(), edge_dim=3)
    assert tuple(gine.lin.weight.shape) == (6, 3) and conv.GINEConv(mlp()).lin is None
    le = conv.LEConv(5, 7)
    assert sorted(le.state_dict()) == ["lin1.bias", "lin1.weight", "lin2.weight", "lin3.bias", "lin3.weight"]
    bn = standin["nn"].BatchNorm(6)
    assert sorted(bn.state_dict()) == ["module.bias", "module.num_batches_tracked", "module.running_mean", "module.running_var", "module.weight"]
    assert list(standin["nn"].InstanceNorm(6).state_dict()) == []


def test_instance_norm_and_pools_equal_loops(standin):
    g = torch.Generator().manual_seed(7)
    batch = torch.tensor([0, 0, 0, 1, 1, 2, 3, 3, 3, 3])               # graph 2 has one row
    x = torch.randn(10, 3, dtype=torch.float64, generator=g)
    norm = standin["nn"].InstanceNorm(3)
    assert torch.equal(norm.train()(x, batch), norm.eval()(x, batch))
    out = norm(x, batch)
    for gid in range(4):
        rows = x[batch == gid]
        mean = rows.sum(0) / len(rows)
        var = ((rows - mean) ** 2).sum(0) / len(rows)                  # biased
        assert torch.allclose(out[batch == gid], (rows - mean) / (var + 1e-5).sqrt(), rtol=0, atol=1e-13)
    assert bool((out[5] == 0).all())
    add, mean = standin["nn"].global_add_pool(x, batch), standin["nn"].global_mean_pool(x, batch)
    for gid in range(4):
        assert torch.allclose(add[gid], x[batch == gid].sum(0), rtol=0, atol=1e-14)
        assert torch.allclose(mean[gid], x[batch == gid].mean(0), rtol=0, atol=1e-14)


def test_encoders_sum_one_lookup_per_column(standin):
    for Enc, name, cols in ((standin["AtomEncoder"], "atom_embedding_list", 9), (standin["BondEncoder"], "bond_embedding_list", 3)):
        enc = Enc(4)
        tables = getattr(enc, name)
        assert len(tables) == cols
        x = torch.stack([torch.randint(0, t.num_embeddings, (6,)) for t in tables], dim=1)
        want = sum(tables[i].weight[x[:, i]] for i in range(cols))
        assert torch.equal(enc(x), want)


def test_placeholders_are_inert_and_never_shadow(standin):
    import _placeholder
    assert _placeholder.install("json") is False and _placeholder.install("torch.nn") is False     # real modules are left alone
    to_networkx = standin["utils"].to_networkx
    with pytest.raises(RuntimeError):
        to_networkx()

    class Dataset(standin["utils"].anything_else):                      # usable as a base class, as the reference's datasets do
        pass
    Dataset()
