"""A plain reference of the PNA multi-aggregation (csrc/pna.hip) and its analytic backward: explicit per-row loops in numpy, no autograd,
nothing shared with oracle/ops.py; plus the graphs and the two input recipes the PNA tests share.  CPU only.

For destination row i the in-edges are taken in edge order (the CSR build is stable, so this is the kernels' slot order) and the messages
are m_e = w_e * [x_i | x_src(e) | emb_e] with w_e = att_e (edge attention), na[dst] * na[src] (node attention) or 1.  The gradient of min
and max goes to the FIRST edge in edge order that attains the extremum (np.argmin / np.argmax: first occurrence, -0.0 == +0.0).

The exact recipe.  x and the edge embedding are k/4 with |k| <= 8, drawn from a pool of a few distinct rows, attention is in
{0, 1/4, 1/2, 3/4, 1}, dout is k/4 with |k| <= 8, zero on the std segments and, on rows whose in-degree is not a power of two, on the mean
segments.  Every message is then a multiple of 1/16 (1/64 with node attention) of magnitude <= 2, 1/n is a power of two wherever the mean is live, and every sum of
the forward and the backward stays inside the 24-bit fp32 significand: an fp32 evaluation in ANY order is the exact result, so the GPU
tests compare bit for bit with the float64 reference cast to fp32.  tests/test_pna_oracle_host.py checks that premise without a kernel
(float32 in forward, reverse and a random visiting order against float64).

The float recipe.  Seeded randn / rand values with ReLU zeros in x, as tests/test_gpu_pna.py draws them, and a full random dout."""
from functools import lru_cache
from types import SimpleNamespace as NS

import numpy as np
import torch

LONG_ROW = 256                                                   # GSAT_LONG_ROW_EDGES
AGG4 = ["mean", "min", "max", "std"]
AGG5 = ["mean", "min", "max", "std", "sum"]
AGG_STAGED = ["sum", "min", "max"]                               # generic kernel, gradient row staged in LDS (nseg <= 8)
AGG_ALL = ["mean", "min", "max", "std", "sum", "var"]
SCALERS3 = ["identity", "amplification", "attenuation"]
AGG_CODES = {"sum": 0, "mean": 1, "min": 2, "max": 3, "var": 4, "std": 5}
SCALER_CODES = {"identity": 0, "amplification": 1, "attenuation": 2, "linear": 3, "inverse_linear": 4}
ROW_DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17)
HUB_DEGREES = (256, 257, 512, 513, 1025)


def lpr(H):
    """Lanes per row of pna_lpr (each lane holds one float4)."""
    q = H // 4
    return 4 if q <= 4 else 8 if q <= 8 else 16 if q <= 16 else 20 if q <= 20 else 32 if q <= 32 else 64


def scaler_factor(name, deg, avg, dtype):
    """scaler_factor of csrc/pna.hip: the degree is the unweighted in-degree; attenuation and inverse_linear are 1 on an empty row."""
    deg, one = dtype(deg), dtype(1)
    if name == "identity":
        return one
    if name == "amplification":
        return np.log(deg + one) / dtype(avg["log"])
    if name == "attenuation":
        return one if deg == 0 else dtype(avg["log"]) / np.log(deg + one)
    if name == "linear":
        return deg / dtype(avg["lin"])
    if name == "inverse_linear":
        return one if deg == 0 else dtype(avg["lin"]) / deg
    raise ValueError(name)


def _seqsum(a):
    """Sum of the rows of a [d, F], strictly one after the other, in a's dtype."""
    if a.shape[0] == 0:
        return np.zeros(a.shape[1], dtype=a.dtype)
    return np.cumsum(a, axis=0, dtype=a.dtype)[-1]


def _visit(d, order, rng):
    if order is None:
        return np.arange(d)
    if order == "reverse":
        return np.arange(d)[::-1]
    return rng.permutation(d)


def pna_reference(x, ei, aggr, scalers, avg, att=None, node_att=None, edge_emb=None, dout=None, dtype=np.float64, order=None):
    """out [N, S*A*F] (layout [scaler][aggregator][x_i | x_j | emb][H]) and, with ``dout``, dx, datt [E] / dna [N], dedge [E, H].
    ``order``: None (edge order), "reverse" or an int seed: the order in which every sum visits its terms."""
    def arr(t):
        return None if t is None else np.ascontiguousarray(np.asarray(t, dtype=np.float64).astype(dtype))
    x, att, na, emb, dout = arr(x), arr(att), arr(node_att), arr(edge_emb), arr(dout)
    ei = np.asarray(ei)
    src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
    N, H = x.shape
    E = src.shape[0]
    P = 3 if emb is not None else 2
    F, A, S = P * H, len(aggr), len(scalers)
    if att is not None:
        w_all = att.reshape(-1)
    elif na is not None:
        na = na.reshape(-1)
        w_all = na[dst] * na[src]
    else:
        w_all = np.ones(E, dtype=dtype)
    rng = np.random.RandomState(order) if isinstance(order, int) else None
    by_row = np.argsort(dst, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))])
    out = np.zeros((N, S * A * F), dtype=dtype)
    eps, two, half = dtype(1e-5), dtype(2), dtype(0.5)
    dx = np.zeros((N, H), dtype=dtype)
    dmsg = np.zeros((E, H), dtype=dtype)
    dedge = np.zeros((E, H), dtype=dtype) if emb is not None else None
    dw = np.zeros(E, dtype=dtype)
    cols = np.arange(F)
    for i in range(N):
        es = by_row[ptr[i]:ptr[i + 1]]                           # ascending edge ids
        d = es.shape[0]
        fs = [scaler_factor(s, d, avg, dtype) for s in scalers]
        if d == 0:
            val = {"std": np.full(F, np.sqrt(eps), dtype=dtype)}
            zero = np.zeros(F, dtype=dtype)
            out[i] = np.concatenate([f * val.get(a, zero) for f in fs for a in aggr])
            continue
        U = np.concatenate([np.broadcast_to(x[i], (d, H)), x[src[es]]] + ([emb[es]] if emb is not None else []), axis=1)
        w = w_all[es]
        M = w[:, None] * U
        p = _visit(d, order, rng)
        n = dtype(d)
        mean = _seqsum(M[p]) / n
        var = _seqsum((M * M)[p]) / n - mean * mean
        jmin, jmax = M.argmin(axis=0), M.argmax(axis=0)
        val = {"sum": _seqsum(M[p]), "mean": mean, "min": M[jmin, cols], "max": M[jmax, cols], "var": var,
               "std": np.sqrt(np.maximum(var, dtype(0)) + eps)}
        out[i] = np.concatenate([f * val[a] for f in fs for a in aggr])
        if dout is None:
            continue
        g = dout[i].reshape(S, A, F)
        dM = np.zeros((d, F), dtype=dtype)
        hs = np.where(var > 0, half / np.sqrt(var + eps), dtype(0)).astype(dtype)      # relu'(0) = 0
        for si, f in enumerate(fs):
            for ai, a in enumerate(aggr):
                v = f * g[si, ai]
                if a == "sum":
                    dM += v
                elif a == "mean":
                    dM += v / n
                elif a == "min":
                    dM[jmin, cols] += v
                elif a == "max":
                    dM[jmax, cols] += v
                elif a == "var":
                    dM += (v * (two / n)) * (M - mean)
                else:
                    dM += (v * hs * (two / n)) * (M - mean)
        dw[es] = (dM * U).sum(axis=1, dtype=dtype)
        dU = w[:, None] * dM
        dx[i] += _seqsum(dU[p, :H])                              # dx_self
        dmsg[es] = dU[:, H:2 * H]
        if emb is not None:
            dedge[es] = dU[:, 2 * H:]
    res = NS(out=out, dx=None, datt=None, dna=None, dedge=None)
    if dout is None:
        return res
    ev = _visit(E, order, rng)
    np.add.at(dx, src[ev], dmsg[ev])                             # unbuffered: one term after the other
    res.dx, res.dedge = dx, dedge
    if att is not None:
        res.datt = dw
    elif na is not None:
        dna = np.zeros(N, dtype=dtype)
        np.add.at(dna, dst[ev], dw[ev] * na[src[ev]])
        np.add.at(dna, src[ev], dw[ev] * na[dst[ev]])
        res.dna = dna
    return res


# ---- graphs ------------------------------------------------------------------------------------------------------------------------------
def _edges_in_slot_order(rows, seed):
    """rows: [(dst, [src per slot])] -> edge_index whose edges are interleaved at random while every row keeps its slot order."""
    rng = np.random.RandomState(seed)
    label = rng.permutation(np.concatenate([np.full(len(s), r) for r, (_, s) in enumerate(rows)]).astype(np.int64))
    E = label.shape[0]
    src, dst = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
    for r, (d, s) in enumerate(rows):
        pos = np.nonzero(label == r)[0]
        src[pos], dst[pos] = np.asarray(s, dtype=np.int64), d
    return np.stack([src, dst])


@lru_cache(maxsize=None)
def row_length_graph():
    """Graph A: 60 nodes, node i has ROW_DEGREES[i % 11] in-edges (the last five none), sources drawn with repetition (duplicate edges),
    a self-loop on node 1, edges shuffled.  Returns (edge_index int64 [2, E], N)."""
    N = 60
    rng = np.random.RandomState(11)
    rows = []
    for i in range(55):
        d = ROW_DEGREES[i % len(ROW_DEGREES)]
        s = rng.randint(0, N, size=d)
        if d >= 2:
            s[-1] = s[0]                                         # a duplicate edge
        if i == 1:
            s[0] = 1                                             # a self-loop
        rows.append((i, s.tolist()))
    ei = _edges_in_slot_order([r for r in rows if r[1]], 12)
    deg = np.bincount(ei[1], minlength=N)
    assert set(deg.tolist()) == set(ROW_DEGREES)
    return torch.from_numpy(ei), N


HUB_EXT, HUB_LAST = 1099, 1098                                   # source nodes with prescribed feature rows (hub_exact_inputs)


@lru_cache(maxsize=None)
def hub_graph():
    """Graph C: 1100 nodes; rows 0..4 have HUB_DEGREES in-edges (256 is not long: the hub test is > 256), rows 5..12 are short.  In slot
    order a hub row has source HUB_EXT at slots 3 and 300 (200 in the 256-edge row): chunk 0 and a later chunk; and HUB_LAST at its last
    slot: the single edge of the last chunk of the 257-, 513- and 1025-edge rows.  Returns (edge_index, N, {row: slot list of edge ids})."""
    N = 1100
    rng = np.random.RandomState(21)
    rows = []
    for r, d in enumerate(HUB_DEGREES):
        s = rng.randint(5, HUB_LAST, size=d)
        s[3] = HUB_EXT
        s[300 if d > 300 else 200] = HUB_EXT
        s[-1] = HUB_LAST
        rows.append((r, s.tolist()))
    for r, d in zip(range(5, 13), (1, 3, 4, 5, 9, 2, 8, 16)):
        rows.append((r, rng.randint(0, N, size=d).tolist()))
    ei = _edges_in_slot_order(rows, 22)
    slots = {r: np.nonzero(ei[1] == r)[0] for r in range(len(HUB_DEGREES))}
    return torch.from_numpy(ei), N, slots


@lru_cache(maxsize=None)
def one_chunk_graph():
    """A batch of exactly 256 edges (no row can be long: the *_long entry points drop the chunk list): one row of 240 in-edges, short rows."""
    N = 40
    rng = np.random.RandomState(31)
    rows = [(0, rng.randint(1, N, size=240).tolist()), (1, rng.randint(0, N, size=9).tolist()), (2, rng.randint(0, N, size=5).tolist()),
            (5, rng.randint(0, N, size=2).tolist())]
    ei = _edges_in_slot_order(rows, 32)
    assert ei.shape[1] == LONG_ROW
    return torch.from_numpy(ei), N


STAR_CENTRE, STAR_LEAVES = 40, 40                                # window_graph: node 40 has 40 in-edges


@lru_cache(maxsize=None)
def window_graph():
    """Graph F: 80 nodes in block-diagonal graphs: five two-way rings of 6, isolated nodes 30..39, a star whose centre (node 40) has 40
    in-edges from leaves 41..79 (one of them twice) that send nothing else (the centre answers the first four), and one edge from node 2 to node 75: a source
    whose destination lies in another window.  Returns (edge_index, batch, N)."""
    src, dst, batch = [], [], []
    for g in range(5):
        for k in range(6):
            a, b = 6 * g + k, 6 * g + (k + 1) % 6
            src += [a, b]; dst += [b, a]
        batch += [g] * 6
    batch += list(range(5, 15))                                  # isolated nodes: one graph each
    N = STAR_CENTRE + 1 + STAR_LEAVES - 1
    leaves = list(range(STAR_CENTRE + 1, N))
    src += leaves + [leaves[0]]; dst += [STAR_CENTRE] * (len(leaves) + 1)       # a duplicate edge: 40 in-edges
    src += [STAR_CENTRE] * 4; dst += leaves[:4]
    batch += [15] * (N - STAR_CENTRE)
    src.append(2); dst.append(75)
    ei = np.stack([np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)])
    ei = ei[:, np.random.RandomState(41).permutation(ei.shape[1])]
    assert int(np.bincount(ei[1], minlength=N)[STAR_CENTRE]) == STAR_LEAVES
    return torch.from_numpy(ei), torch.tensor(batch, dtype=torch.int64), N


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def in_degree(ei, N):
    return np.bincount(np.asarray(ei)[1], minlength=N)


def exact_dout(ei, N, H, aggr, scalers, parts, seed):
    """k/4 with |k| <= 8; zero on the std (and var) segments and, on rows whose in-degree is not a power of two, on the mean segments."""
    rng = np.random.RandomState(seed)
    A, S = len(aggr), len(scalers)
    g = rng.randint(-8, 9, size=(N, S, A, parts * H)).astype(np.float64) / 4
    deg = in_degree(ei, N)
    pow2 = (deg > 0) & ((deg & (deg - 1)) == 0)
    for ai, a in enumerate(aggr):
        if a in ("std", "var"):
            g[:, :, ai] = 0
        if a == "mean":
            g[~pow2, :, ai] = 0
    return torch.from_numpy(g.reshape(N, -1)).float(), torch.from_numpy(pow2)


def exact_inputs(ei, N, H, seed, pool=3, edge_emb=False):
    """x [N, H] and emb [E, H] from ``pool`` distinct rows of k/4, |k| <= 8; att [E] and na [N] in {0, 1/4, 1/2, 3/4, 1} (na[::7] = 0);
    dx_add [N, H] and dna0 [N] on the same grid."""
    rng = np.random.RandomState(seed)
    E = np.asarray(ei).shape[1]
    rows = rng.randint(-8, 9, size=(pool, H)).astype(np.float64) / 4
    x = rows[rng.randint(0, pool, size=N)]
    erows = rng.randint(-8, 9, size=(pool, H)).astype(np.float64) / 4
    emb = erows[rng.randint(0, pool, size=E)] if edge_emb else None
    att = rng.randint(0, 5, size=E).astype(np.float64) / 4
    na = rng.randint(1, 5, size=N).astype(np.float64) / 4
    na[::7] = 0
    dx_add = rng.randint(-8, 9, size=(N, H)).astype(np.float64) / 4
    dna0 = rng.randint(-8, 9, size=N).astype(np.float64) / 4
    f = lambda a: None if a is None else torch.from_numpy(a).float()
    return NS(x=f(x), emb=f(emb), att=f(att), na=f(na), dx_add=f(dx_add), dna0=f(dna0))


def float_inputs(ei, N, H, seed, edge_emb=False):
    """randn x with ReLU zeros on every fifth row, rand attention (na[::7] = 0), randn embedding, as tests/test_gpu_pna.py."""
    g = torch.Generator().manual_seed(seed)
    E = np.asarray(ei).shape[1]
    x = torch.randn(N, H, generator=g)
    x[::5] = x[::5].relu()
    att = torch.rand(E, generator=g)
    na = torch.rand(N, generator=g)
    na[::7] = 0.0
    emb = torch.randn(E, H, generator=g) if edge_emb else None
    return NS(x=x, emb=emb, att=att, na=na, dx_add=torch.randn(N, H, generator=g), dna0=torch.randn(N, generator=g))


def float_dout(N, H, aggr, scalers, parts, seed):
    return torch.randn(N, len(scalers) * len(aggr) * parts * H, generator=torch.Generator().manual_seed(seed))


def self_part_inputs(ei, N, H, seed):
    """Case B: exact-recipe inputs whose x rows carry the sign patterns > 0, < 0, +0, -0 per channel (channel c of row i: pattern
    (c + i) % 4) and whose attention attains both its minimum and its maximum twice in every row of two or more in-edges (slots 0 and 1
    the maximum or the minimum in turn, the other extreme on slots 2 and 3 where the row has them)."""
    inp = exact_inputs(ei, N, H, seed)
    rng = np.random.RandomState(seed + 1)
    mag = rng.randint(1, 9, size=(N, H)).astype(np.float64) / 4
    pat = (np.arange(H)[None, :] + np.arange(N)[:, None]) % 4
    x = np.where(pat == 0, mag, np.where(pat == 1, -mag, np.where(pat == 2, 0.0, -0.0)))
    x[pat == 3] = -0.0
    ei = np.asarray(ei)
    att = rng.randint(1, 4, size=ei.shape[1]).astype(np.float64) / 4          # 1/4 .. 3/4 inside
    for i in range(N):
        es = np.nonzero(ei[1] == i)[0]
        lo, hi = (0.0, 1.0) if i % 2 else (1.0, 0.0)
        att[es[:2]] = hi
        att[es[2:4]] = lo
    inp.x, inp.att = torch.from_numpy(x).float(), torch.from_numpy(att).float()
    return inp


def hub_exact_inputs(H, seed, edge_emb=False):
    """Case C, exact recipe on hub_graph().  Ordinary nodes and edges carry pool rows with |value| <= 1 and attention in {1/4 .. 1}.
    Per channel group (c % 3):
      0  the extremum (+-2, the sign alternates with c) is attained by HUB_EXT, at slot 3 and again in a later chunk: chunk 0 must win;
      1  the extremum is attained only by HUB_LAST, at the row's last slot: the single edge of the last chunk of rows 257, 513, 1025;
      2  pool values only: ties everywhere.
    Both carry attention 1 there; attention 0 (the row's att minimum, a -0.0 / +0.0 message) sits at slots 10 and 270 (150 in the
    256-edge row): repeated across chunks.  The edge embedding follows the same plan per slot."""
    ei, N, slots = hub_graph()
    rng = np.random.RandomState(seed)
    E = ei.shape[1]
    c = np.arange(H)
    sign = np.where(c % 2 == 0, 1.0, -1.0)
    pool = rng.randint(-4, 5, size=(3, H)).astype(np.float64) / 4
    ext = np.where(c % 3 == 0, 2.0 * sign, pool[0])
    last = np.where(c % 3 == 1, -2.0 * sign, pool[1])
    x = pool[rng.randint(0, 3, size=N)]
    x[HUB_EXT], x[HUB_LAST] = ext, last
    att = rng.randint(1, 5, size=E).astype(np.float64) / 4
    emb = None
    if edge_emb:
        epool = rng.randint(-4, 5, size=(3, H)).astype(np.float64) / 4
        emb = epool[rng.randint(0, 3, size=E)]
    for r, sl in slots.items():
        d = len(sl)
        again = 300 if d > 300 else 200
        zero2 = 270 if d > 270 else 150
        att[sl[[3, again, d - 1]]] = 1.0
        att[sl[[10, zero2]]] = 0.0
        if edge_emb:
            emb[sl[3]] = emb[sl[again]] = np.where(c % 3 == 0, -2.0 * sign, epool[0])
            emb[sl[d - 1]] = np.where(c % 3 == 1, 2.0 * sign, epool[1])
    f = lambda a: None if a is None else torch.from_numpy(a).float()
    return NS(x=f(x), emb=f(emb), att=f(att), na=None, dx_add=None, dna0=None)
