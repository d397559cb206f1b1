"""Plain references of the row operators (csrc/aggregate.hip, csrc/encoders.hip and the per-edge operators of csrc/edgeops.hip), written
from the formulas of include/gsat_hip.h with index_add_ and explicit indexing, no autograd; plus the graphs and the two input recipes
the row-operator tests share.  CPU only.  Every function casts its inputs to ``dtype`` first: float64 is the reference, float32 "the
same formula in fp32" whose own error the tests grant as slack.

The exact recipe.  x, dout, edge_emb and the tables W are integers in [-4, 4], edge and node attention are in {0, 1/4, ..., 2} and
self_coef is 0, 1 or 1.5.  Every message relu(x + e) is then an integer in [0, 8], every product a multiple of 1/8 of magnitude <= 32,
and a sum of at most 2600 edge terms (or of 2048 columns) is a multiple of 1/8 below 2^17: all partial sums fit the 24-bit fp32
significand, so an fp32 sum in ANY order -- and with or without fused multiply-adds -- is the exact result.  The GPU tests therefore
compare bit for bit with the fp64 reference cast to fp32; tests/test_rowop_oracle_host.py checks that premise without a kernel.

The float recipe.  Seeded randn values and rand attention.  The bounds are derived, not tuned; with u = 2^-24:

- an entry of ``out`` or ``dx`` summed from n terms, c of them read back as chunk partials:
      |got - ref64| <= 2 (n + 4 + c) u abs_sum,      abs_sum = |self_coef s| + sum_k |w_k m_k|.
  Recursive summation of n terms in any order is off by at most (n - 1) u sum|terms| to first order; every term carries the rounding of
  its product (or none, fused), of relu(x + e)'s addition and of self_coef * s: 3 u more; each chunk partial is rounded once more when
  it is stored and added: c u.  That is (n + 2 + c) u abs_sum, (n + 4 + c) with the second-order terms granted generously, and the
  factor 2 is the margin over the first-order bound (n u < 1e-4 here, so the neglected n^2 u^2 terms are far below it).
- ``datt``: a dot product over H columns, |got - ref64| <= 2 (H + 2) u sum_c |m_c g_c|: H - 1 additions in any order (lane partials,
  then the lane-group reduction), the product and relu(x + e)'s addition.
- ``dedge_emb``: one product, |got - ref64| <= 2 u |ref64|.  The ReLU mask is the same in fp32 and fp64: the sign of a rounded sum of
  two fp32 numbers is the sign of the exact sum.
- an entry whose abs_sum is 0 must be exactly 0.
"""
from functools import lru_cache
from types import SimpleNamespace as NS

import torch

U = 2.0 ** -24
LONG_ROW = 256                                   # GSAT_LONG_ROW_EDGES
WIDTHS = (4, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048)       # both ends of every (LPR, NV) bucket
HUB_DEGREES = (255, 256, 257, 258, 259, 511, 512, 513, 1300)


def row_geom(H):
    """(LPR, NV) of csrc/aggregate.hip for width H."""
    q = H // 4
    for lpr in (4, 8, 16, 32, 64):
        if q <= lpr:
            return lpr, 1
    return 64, (2 if q <= 128 else 4 if q <= 256 else 8)


# ---- CSR -------------------------------------------------------------------------------------------------------------------------------
def csr(edge_index, N, by):
    """(rowptr, other end, edge id) per slot, rows = edge_index[by], edge-id order inside a row."""
    key, other = edge_index[by], edge_index[1 - by]
    eid = torch.sort(key, stable=True).indices
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(key, minlength=N), 0)
    return rowptr, other[eid], eid


def slot_rows(rowptr):
    rowptr = rowptr.long()
    return torch.repeat_interleave(torch.arange(rowptr.shape[0] - 1), rowptr[1:] - rowptr[:-1])


def _scatter(N, rows, terms, order):
    if order is not None:
        rows, terms = rows[order], terms[order]
    return torch.zeros(N, terms.shape[1], dtype=terms.dtype).index_add_(0, rows, terms)


# ---- sum aggregation -------------------------------------------------------------------------------------------------------------------
def aggr_sum(x, self_rows, att, edge_emb, rowptr, col, eid, self_coef, dtype=torch.float64, order=None):
    """out[i] = self_coef * self_rows[i] + sum_{k in row i} w_k m_k with m_k = x[col[k]] or relu(x[col[k]] + edge_emb[eid[k]]) and
    w_k = att[eid[k]] or 1; self_rows None -> x, not read when self_coef == 0.  Returns (out, abs_sum).  ``order``: a permutation of the
    slots, the order in which the terms are added."""
    col, rows = col.long(), slot_rows(rowptr)
    N = rowptr.shape[0] - 1
    m = x.to(dtype)[col]
    if edge_emb is not None:
        m = torch.relu(m + edge_emb.to(dtype)[eid.long()])
    if att is not None:
        m = m * att.to(dtype).reshape(-1)[eid.long()].view(-1, 1)
    out = _scatter(N, rows, m, order)
    abs_sum = _scatter(N, rows, m.abs(), order)
    if self_coef != 0:
        s = self_coef * (x if self_rows is None else self_rows).to(dtype)[:N]
        out, abs_sum = out + s, abs_sum + s.abs()
    return out, abs_sum


def aggr_sum_bwd(x, att, edge_emb, dout, rowptr_src, dst, eid, self_coef, dtype=torch.float64, order=None, col_order=None):
    """Backward over the by-source CSR.  Returns NS(dx, datt, dedge_emb, dx_abs, datt_abs): dx[j] = self_coef dout[j] + sum_{k in
    source row j} w_k dout[dst[k]] [pre_k > 0]; datt[eid[k]] = <m_k, dout[dst[k]]> (summed over H, in ``col_order``);
    dedge_emb[eid[k]] = w_k dout[dst[k]] [pre_k > 0] (None without edge_emb).  The ReLU slope is 0 at pre <= 0."""
    dst, eid, rows = dst.long(), eid.long(), slot_rows(rowptr_src)
    N, E = rowptr_src.shape[0] - 1, dst.shape[0]
    d = dout.to(dtype)
    g = d[dst]
    m = x.to(dtype)[rows]
    if edge_emb is not None:
        pre = m + edge_emb.to(dtype)[eid]
        m = torch.relu(pre)
        gm = g * (pre > 0).to(dtype)
    else:
        gm = g
    prod = m * g
    if col_order is not None:
        prod = prod[:, col_order]
    datt, datt_abs = torch.zeros(E, dtype=dtype), torch.zeros(E, dtype=dtype)
    if dtype == torch.float32:                       # a plain left-to-right fp32 sum over the columns
        acc, acc_abs = torch.zeros(E, dtype=dtype), torch.zeros(E, dtype=dtype)
        for c in range(prod.shape[1]):
            acc, acc_abs = acc + prod[:, c], acc_abs + prod[:, c].abs()
    else:
        acc, acc_abs = prod.sum(1), prod.abs().sum(1)
    datt[eid], datt_abs[eid] = acc, acc_abs
    if att is not None:
        gm = gm * att.to(dtype).reshape(-1)[eid].view(-1, 1)
    dedge = None
    if edge_emb is not None:
        dedge = torch.zeros(E, d.shape[1], dtype=dtype)
        dedge[eid] = gm
    s = self_coef * d[:N]
    return NS(dx=_scatter(N, rows, gm, order) + s, datt=datt, dedge_emb=dedge, dx_abs=_scatter(N, rows, gm.abs(), order) + s.abs(),
              datt_abs=datt_abs)


def sum_bound(rowptr, abs_sum, chunks=None):
    """2 (n + 4 + c) u abs_sum per entry: n = row length + 1 (the self term), c = chunk partials of the row."""
    rowptr = rowptr.long()
    n = (rowptr[1:] - rowptr[:-1] + 1).double()
    c = torch.zeros_like(n) if chunks is None else chunks.double()
    return 2.0 * (n + 4.0 + c).view(-1, 1) * U * abs_sum.double()


def chunk_counts(rowptr):
    """ceil(d / 256) chunks for a row of d > 256 entries, else none."""
    rowptr = rowptr.long()
    d = rowptr[1:] - rowptr[:-1]
    return torch.where(d > LONG_ROW, (d + LONG_ROW - 1) // LONG_ROW, torch.zeros_like(d))


# ---- segment pools ---------------------------------------------------------------------------------------------------------------------
def _seg_ids(ptr):
    return slot_rows(ptr)


def segment_pool(x, ptr, mean, dtype=torch.float64):
    ptr = ptr.long()
    G = ptr.shape[0] - 1
    out = torch.zeros(G, x.shape[1], dtype=dtype).index_add_(0, _seg_ids(ptr), x.to(dtype)[: int(ptr[-1])])
    if mean:
        out = out / (ptr[1:] - ptr[:-1]).clamp(min=1).to(dtype).view(-1, 1)
    return out


def segment_pool_bwd(dout, ptr, mean, dtype=torch.float64):
    ptr = ptr.long()
    d = dout.to(dtype)
    if mean:
        d = d / (ptr[1:] - ptr[:-1]).clamp(min=1).to(dtype).view(-1, 1)
    return d[_seg_ids(ptr)]


def pool_lengths(H):
    gpb = 256 // row_geom(H)[0]
    return (0, 1, 2, 0, 4 * gpb, 4 * gpb + 1, 37, 0)


# ---- encoders --------------------------------------------------------------------------------------------------------------------------
def _clamped_rows(x, dims):
    dims = torch.as_tensor(dims, dtype=torch.int64)
    off = torch.cumsum(dims, 0) - dims
    return torch.minimum(x.long().clamp(min=0), dims - 1) + off


def embsum(x, dims, W, dtype=torch.float64):
    """out[n] = sum_col W[offset(col) + clamp(x[n, col], 0, dims[col] - 1)]."""
    rows = _clamped_rows(x, dims)
    out = torch.zeros(x.shape[0], W.shape[1], dtype=dtype)
    for c in range(rows.shape[1]):
        out += W.to(dtype)[rows[:, c]]
    return out


def onehot_rows(x, dims, R_padded, dtype=torch.float32):
    rows = _clamped_rows(x, dims)
    O = torch.zeros(x.shape[0], R_padded, dtype=dtype)
    O[torch.arange(x.shape[0]).view(-1, 1).expand_as(rows), rows] = 1
    return O


def table_dims(ncol):
    return [(5, 3, 7, 2, 1, 11, 4)[c % 7] for c in range(ncol)]


# ---- per-edge operators ----------------------------------------------------------------------------------------------------------------
def lift(a, src, dst, dtype=torch.float64):
    a = a.to(dtype).reshape(-1)
    return a[src.long()] * a[dst.long()]


def lift_bwd(a, dedge, src, dst, dtype=torch.float64):
    """da[n] = sum_{e: src_e = n} d_e a[dst_e] + sum_{e: dst_e = n} d_e a[src_e]; a self loop counts on both sides."""
    a, d, src, dst = a.to(dtype).reshape(-1), dedge.to(dtype).reshape(-1), src.long(), dst.long()
    da = torch.zeros_like(a)
    da.index_add_(0, src, d * a[dst])
    da.index_add_(0, dst, d * a[src])
    return da


def symmetrise(att, rev, flag=None, dtype=torch.float64):
    a = att.to(dtype).reshape(-1)
    if flag is not None and int(flag) == 0:
        return a.clone()
    return (a + a[rev.long()]) / 2


def gather_clamped(table, index):
    return table[index.long().clamp(0, table.shape[0] - 1)]


def involution(E, seed, fixed):
    """A reverse-edge map on E entries: seeded random pairs, the last ``fixed`` (and an odd one out) paired with themselves."""
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(seed))
    rev = torch.arange(E)
    pairs = max(E - fixed, 0) // 2
    a, b = perm[:pairs], perm[pairs:2 * pairs]
    rev[a], rev[b] = b, a
    return rev


# ---- info loss -------------------------------------------------------------------------------------------------------------------------
def info_terms(att, r, dtype=torch.float64):
    """The two pieces of a log(a / r + 1e-6) + (1 - a) log((1 - a) / (1 - r + 1e-6) + 1e-6), per entry."""
    a = att.to(dtype).reshape(-1)
    r = r.to(dtype).reshape(-1) if torch.is_tensor(r) else torch.tensor(float(r), dtype=dtype)
    eps = torch.tensor(1e-6, dtype=dtype)
    return a * torch.log(a / r + eps), (1 - a) * torch.log((1 - a) / (1 - r + eps) + eps)


def info_dterm(att, r, dtype=torch.float64):
    a = att.to(dtype).reshape(-1)
    r = r.to(dtype).reshape(-1) if torch.is_tensor(r) else torch.tensor(float(r), dtype=dtype)
    eps = torch.tensor(1e-6, dtype=dtype)
    q = 1 - r + eps
    t1, t2 = a / r + eps, (1 - a) / q + eps
    return torch.log(t1) + a / (r * t1) - torch.log(t2) - (1 - a) / (q * t2)


def info_counted(m_valid, M):
    return M if m_valid is None else min(max(int(m_valid), 0), M)


def info_loss(att, r, m_valid=None, dtype=torch.float64):
    """(loss, sum(|piece1| + |piece2|) / max(m, 1)) over the first m = clamp(m_valid, 0, M) entries; the per-entry terms in ``dtype``,
    their sum in fp64."""
    m = info_counted(m_valid, att.numel())
    p1, p2 = info_terms(att, r, dtype)
    return (p1 + p2)[:m].double().sum() / max(m, 1), (p1.abs() + p2.abs())[:m].double().sum() / max(m, 1)


def info_loss_bwd(att, r, gout, m_valid=None, dtype=torch.float64):
    m = info_counted(m_valid, att.numel())
    inv = torch.tensor(1.0, dtype=dtype) / torch.tensor(float(max(m, 1)), dtype=dtype)
    d = torch.tensor(float(gout), dtype=dtype) * inv * info_dterm(att, r, dtype)
    d[m:] = 0
    return d


def info_att(M, m):
    """The attention of test_info_loss_counts_valid_entries_only: m entries in [0.02, 0.98], the rest at 0.5, next to 0 and 1, and at
    exactly 0 and 1."""
    g = torch.Generator().manual_seed(M + 31 * m)
    att = torch.rand(M, generator=g) * 0.96 + 0.02
    edge = torch.tensor([0.5, 1e-7, 1.0 - 1e-7, 0.0, 1.0]).repeat(M // 5 + 1)[:M]
    att[m:] = edge[m:]
    prior = torch.rand(M, generator=g) * 0.8 + 0.1
    return att, prior


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------
def _shuffled(edges, seed):
    ei = torch.tensor(edges, dtype=torch.int64).t().contiguous()
    return ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(seed))].contiguous()


@lru_cache(maxsize=None)
def small_graph(copies=1, num_nodes=None):
    """40 nodes, in- and out-degrees 0..5, two self loops, a duplicate edge, a node with a self loop only, an isolated node; edge ids
    shuffled.  ``copies``: that many disjoint copies; ``num_nodes``: isolated nodes up to that count."""
    base = []
    for i in range(36):
        for j in range(i % 6):
            base.append(((i * 5 + 7 * j + 1) % 36, i))
    base += [(3, 3), (10, 10), base[5], (37, 0), (37, 1), (2, 38), (39, 39)]          # node 36 stays isolated
    edges = [(s + 40 * c, d + 40 * c) for c in range(copies) for (s, d) in base]
    N = 40 * copies if num_nodes is None else num_nodes
    return _shuffled(edges, 11 + copies), N


@lru_cache(maxsize=None)
def hubs_graph():
    """One undirected batch of 1400 nodes: hubs 0..8 with HUB_DEGREES neighbours each among the 1300 leaves 9..1308 (distinct leaves
    per hub, windows that overlap between hubs), a path over the nodes 1309..1389, ten isolated nodes."""
    und = []
    for h, d in enumerate(HUB_DEGREES):
        und += [(h, 9 + (137 * h + j) % 1300) for j in range(d)]
    und += [(v, v + 1) for v in range(1309, 1389)]
    edges = und + [(b, a) for (a, b) in und]
    return _shuffled(edges, 5), 1400


@lru_cache(maxsize=None)
def star_graph(E, reverse=False):
    """A directed star of E leaves into node 0 (or out of it)."""
    edges = [(0, v) if reverse else (v, 0) for v in range(1, E + 1)]
    return _shuffled(edges, E), E + 1


@lru_cache(maxsize=None)
def ring_graph(N):
    """i -> i + 1 and i -> 7 i + 3 (mod N): E = 2 N, in- and out-degree 2 when gcd(7, N) = 1."""
    i = torch.arange(N)
    ei = torch.stack([torch.cat([i, i]), torch.cat([(i + 1) % N, (7 * i + 3) % N])])
    return ei[:, torch.randperm(2 * N, generator=torch.Generator().manual_seed(N))].contiguous(), N


GRAPHS = {
    "small": lambda: small_graph(),
    "small_x3": lambda: small_graph(3),
    "hubs": hubs_graph,
    "hub_in": lambda: star_graph(300),
    "hub_out": lambda: star_graph(300, True),
    "edge256": lambda: star_graph(256),
    "edge257": lambda: star_graph(257),
    "ring": lambda: ring_graph(65540),
}


# ---- input recipes ---------------------------------------------------------------------------------------------------------------------
def ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).float()


def quarters(g, *shape):
    return torch.randint(0, 9, shape, generator=g).float() / 4


@lru_cache(maxsize=4)
def rowop_inputs(N, E, H, recipe, seed=0):
    """fp32 inputs of one aggregation case (cached: treat as read-only): x, dout [N, H]; edge_emb, xe (an edge-row source) [E, H];
    att [E]; node_att [N]; dedge_att [E]."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 31 * E + H)
    if recipe == "exact":
        return NS(x=ints(g, N, H), dout=ints(g, N, H), edge_emb=ints(g, E, H), xe=ints(g, E, H), att=quarters(g, E),
                  node_att=quarters(g, N), dedge_att=ints(g, E))
    assert recipe == "float"
    r = lambda *s: torch.randn(*s, generator=g)
    return NS(x=r(N, H), dout=r(N, H), edge_emb=r(E, H), xe=r(E, H), att=torch.rand(E, generator=g),
              node_att=torch.rand(N, generator=g), dedge_att=r(E))
