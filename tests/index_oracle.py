"""The per-batch integer index restated in plain numpy (int64), and the table of cases the index builders are run on.

Every kernel of the library reads this index (the two CSRs, the slot map, the hub chunk lists, the reverse permutation, the segment
pointers, the edges-by-graph order), so the comparisons built on this file are all ``array_equal``: no tolerance anywhere.  The
restatements follow the documented rules of include/gsat_hip.h and the comments of bookkeeping.hip, not its code: a stable argsort,
a bincount, a searchsorted.  The dual graphs stay with oracle/bookkeeping.py.

The case builders are seeded and place every boundary by construction; tests/test_index_oracle_host.py asserts from the generated
arrays that each boundary is really there, so an edit that loses one fails on the CPU.
"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- constants: one place each -----------------------------------------------------------------------------------------------------
def long_row_edges() -> int:
    """GSAT_LONG_ROW_EDGES of include/gsat_hip.h: rows above it are split into hub chunks of that many slots."""
    txt = open(os.path.join(ROOT, "include", "gsat_hip.h")).read()
    return int(re.search(r"#define\s+GSAT_LONG_ROW_EDGES\s+(\d+)", txt).group(1))


def counting_limits():
    """(row limit, chunk, key limit) of the counting build, from the library (gsat_csr_counting_limits: host only, needs no GPU)."""
    from dp_gsat_amd import _lib
    out = (ctypes.c_int64 * 3)()
    _lib.load().gsat_csr_counting_limits(out)
    return int(out[0]), int(out[1]), int(out[2])


def csr_counts(keys: int) -> int:
    """1 when a build of ``keys`` keys counts, 0 when it sorts (gsat_csr_counts; sees GSAT_CSR_COUNTING of this process)."""
    from dp_gsat_amd import _lib
    return int(_lib.load().gsat_csr_counts(int(keys)))


# ---- restatements ---------------------------------------------------------------------------------------------------------------------
def clamp_ids(v, n: int):
    """(ids with everything outside [0, n) replaced by n - 1, number of replaced ids): the documented treatment of bad ids."""
    v = np.asarray(v, dtype=np.int64)
    bad = (v < 0) | (v >= n)
    return np.where(bad, n - 1, v), int(bad.sum())


def csr(rows, other, R: int):
    """(rowptr[R+1], perm, other[perm]) of gsat_build_csr: perm = edge ids by (row, edge id); bad rows are clamped to R - 1 first."""
    rows, _ = clamp_ids(rows, R)
    perm = np.argsort(rows, kind="stable").astype(np.int64)
    rowptr = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=R)[:R], out=rowptr[1:])
    return rowptr, perm, (None if other is None else np.asarray(other, dtype=np.int64)[perm])


def chunk_ptr(rowptr, L: int):
    """Exclusive scan, len(rowptr) entries, of ``deg > L ? ceil(deg / L) : 0``."""
    deg = np.diff(rowptr)
    chunks = np.where(deg > L, (deg + L - 1) // L, 0)
    out = np.zeros(rowptr.shape[0], dtype=np.int64)
    np.cumsum(chunks, out=out[1:])
    return out


PAIR_OUTPUTS = ("rowptr_dst", "src_by_dst", "eid_by_dst", "rowptr_src", "dst_by_src", "eid_by_src", "slot_dst_of_srcslot",
                "chunk_ptr_dst", "chunk_ptr_src", "src32", "dst32")


def pair(ei, N: int, L: int | None = None):
    """The eleven outputs of gsat_build_csr_pair and its four status words, by name."""
    L = long_row_edges() if L is None else L
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    E = ei.shape[1]
    if E == 0:
        z, e = np.zeros(N + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)
        out = {k: (z.copy() if k.startswith(("rowptr", "chunk")) else e.copy()) for k in PAIR_OUTPUTS}
        out["status"] = np.zeros(4, dtype=np.int64)
        return out
    src, bad_s = clamp_ids(ei[0], N)
    dst, bad_d = clamp_ids(ei[1], N)
    rowptr_dst, eid_by_dst, src_by_dst = csr(dst, src, N)
    rowptr_src, eid_by_src, dst_by_src = csr(src, dst, N)
    inv = np.empty(E, dtype=np.int64)
    inv[eid_by_dst] = np.arange(E)
    cd, cs = chunk_ptr(rowptr_dst, L), chunk_ptr(rowptr_src, L)
    return dict(rowptr_dst=rowptr_dst, src_by_dst=src_by_dst, eid_by_dst=eid_by_dst, rowptr_src=rowptr_src, dst_by_src=dst_by_src,
                eid_by_src=eid_by_src, slot_dst_of_srcslot=inv[eid_by_src], chunk_ptr_dst=cd, chunk_ptr_src=cs, src32=src, dst32=dst,
                status=np.array([bad_s + bad_d, cd[-1], cs[-1], 0], dtype=np.int64))


def edge_keys_u64(ei, N: int, transposed: bool = False):
    """src * N + dst as uint64 (exact up to N = 2^31 - 1, where the product needs 62 bits)."""
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    a, b = (ei[1], ei[0]) if transposed else (ei[0], ei[1])
    return a.astype(np.uint64) * np.uint64(N) + b.astype(np.uint64)


def rev_key_bits(N: int) -> int:
    """Bits of the largest edge key N * N - 1; the sort entry point puts its half bit right above them."""
    return max(int(N * N - 1).bit_length(), 1)


def reverse_perm(ei, N: int):
    """(rev, unmatched): the i-th smallest (key, edge id) pairs with the i-th smallest (transposed key, edge id), so the k-th copy of
    (s, d) meets the k-th copy of (d, s) and a self loop meets itself.  ``unmatched`` counts the sorted positions whose two keys differ
    (k_pair_reverse2's flags[1]); rev is a permutation whether or not it is 0."""
    k, kt = edge_keys_u64(ei, N), edge_keys_u64(ei, N, transposed=True)
    p, q = np.argsort(k, kind="stable"), np.argsort(kt, kind="stable")
    rev = np.empty(k.shape[0], dtype=np.int64)
    rev[q] = p
    return rev, int((k[p] != kt[q]).sum())


def copy_index(ei, N: int):
    """k of every edge: the number of earlier edges (by edge id) with the same (src, dst)."""
    key = edge_keys_u64(ei, N)
    order = np.argsort(key, kind="stable")
    k = np.empty(key.shape[0], dtype=np.int64)
    if key.size:
        first = np.concatenate([[True], key[order][1:] != key[order][:-1]])          # first copy of its (src, dst) in sorted order
        k[order] = np.arange(key.shape[0]) - np.flatnonzero(first)[np.cumsum(first) - 1]
    return k


def rev_branches(ei, N: int):
    """Per edge, the two "shorter row" choices of k_rev_from_csr: (counts its copy index in the out-row of s, walks the in-row of s)."""
    ei = np.asarray(ei, dtype=np.int64)
    out_deg, in_deg = np.bincount(ei[0], minlength=N), np.bincount(ei[1], minlength=N)
    s, d = ei[0], ei[1]
    return out_deg[s] <= in_deg[d], in_deg[s] <= out_deg[d]


def segments(ids, G: int):
    """(ptr[G+1] by searchsorted, ids clamped to [0, G), bad count by k_segments' rule).  The pointers mean something only when the
    bad count is 0: a binary search over an unsorted vector is whatever its probe sequence makes it."""
    ids = np.asarray(ids, dtype=np.int64)
    ptr = np.searchsorted(ids, np.arange(G + 1), side="left").astype(np.int64)
    bad = (ids < 0) | (ids >= G)
    bad[1:] |= ids[:-1] > ids[1:]
    return ptr, np.clip(ids, 0, max(G - 1, 0)), int(bad.sum())


def edge_segments(ei, batch, G: int):
    """(edge_ptr[G+1], edge_order, edge_graph) of GraphSegments.edge_segments: edges grouped by the graph of their source node, in edge
    order inside a graph."""
    ei = np.asarray(ei, dtype=np.int64)
    batch = np.asarray(batch, dtype=np.int64)
    eg = batch[clamp_ids(ei[0], batch.shape[0])[0]]
    eptr, order, _ = csr(eg, None, G)
    return eptr, order, eg


def und_of_edge(ei, und_index):
    """Dual node of every directed edge under the undirected rule: index of (min, max) in und_index, -1 for a self loop."""
    ei = np.asarray(ei, dtype=np.int64)
    where = {(int(a), int(b)): i for i, (a, b) in enumerate(np.asarray(und_index).T)}
    return np.array([-1 if s == d else where[(min(s, d), max(s, d))] for s, d in ei.T.tolist()], dtype=np.int64)


def run_lengths(keys):
    """(start, length, key) of every maximal run of equal adjacent keys."""
    keys = np.asarray(keys, dtype=np.int64)
    if keys.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    start = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return start, np.diff(np.concatenate([start, [keys.size]])), keys[start]


# ---- case builders --------------------------------------------------------------------------------------------------------------------
BAD_IDS = (-1, None, 2 ** 31 + 5, -2 ** 40)          # None stands for N (or R): the first id past the range


def _bad(values, n):
    return [n if v is None else v for v in values]


def tiny_cases():
    """[(name, ei, N)]: E around the wave (64) and the block (256), N down to a single node; self loops and repeated edges wherever E allows."""
    out = []
    for N in (1, 2, 50):
        for E in (0, 1, 2, 63, 64, 65, 255, 256, 257):
            rng = np.random.default_rng(1000 * N + E)
            ei = rng.integers(0, N, size=(2, E), dtype=np.int64)
            if E >= 1:
                ei[1, 0] = ei[0, 0]                       # a self loop
            if E >= 2:
                ei[:, E - 1] = ei[:, (E - 1) // 2]        # a repeated edge; its second copy is the last edge
            out.append((f"tiny_E{E}_N{N}", ei, N))
    return out


def rows_degrees():
    """The in-degrees the `rows` batch contains exactly: either side of every limit a row length is compared with."""
    L = long_row_edges()
    row, chunk, _ = counting_limits()
    return [L - 1, L, L + 1, 2 * L, 2 * L + 1, row - 1, row, row + 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1]


def rows_case(seed: int = 7, N: int = 300, extra: int = 3000):
    """(ei, N): node i < 13 receives exactly rows_degrees()[i] edges from random sources; ``extra`` random edges among the other nodes;
    the whole list shuffled, so a hub's edge ids are scattered.  ei[::-1] is the by-source counterpart."""
    rng = np.random.default_rng(seed)
    degs = rows_degrees()
    dst = np.concatenate([np.full(d, i, dtype=np.int64) for i, d in enumerate(degs)] + [rng.integers(len(degs), N, extra)])
    src = rng.integers(0, N, dst.shape[0])
    perm = rng.permutation(dst.shape[0])
    return np.stack([src[perm], dst[perm]]).astype(np.int64), N


def short_rows_case(seed: int = 5, N: int = 400, E: int = 1200):
    """(ei, N): a molecule-like symmetric batch, degrees far below the long-row limit."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, N, E // 2), rng.integers(0, N, E // 2)
    ei = np.stack([np.concatenate([a, b]), np.concatenate([b, a])]).astype(np.int64)
    return ei[:, rng.permutation(E)], N


def bad_ids_case(seed: int = 11, N: int = 300, E: int = 2000):
    """(ei, N, planted): -1, N, 2^31 + 5 and -2^40 in either row, one edge with both ends bad, and bad ids in the last partial wave
    (E = 2000 = 31 * 64 + 16: edges 1984..1999).  ``planted`` = [(row, edge, value)]."""
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, N, size=(2, E), dtype=np.int64)
    vals = _bad(BAD_IDS, N)
    planted = [(0, 3, vals[0]), (0, 64, vals[1]), (0, 700, vals[2]), (0, 1023, vals[3]),
               (1, 5, vals[1]), (1, 63, vals[0]), (1, 256, vals[3]), (1, 1500, vals[2]),
               (0, 900, vals[2]), (1, 900, vals[0]),                                       # both ends of edge 900
               (0, 1990, vals[1]), (1, 1999, vals[3])]                                     # the last partial wave
    for r, e, v in planted:
        ei[r, e] = v
    return ei, N, planted


def runs_case(seed: int = 3, R: int = 40):
    """(keys, R, other, marks): one key column for gsat_build_csr made of runs laid at known positions; ``marks`` names the start of each
    run the host test looks for.  Keys of neighbouring runs differ, so every run is maximal."""
    rng = np.random.default_rng(seed)
    parts, marks, pos = [], {}, 0

    def put(name, key, n):
        nonlocal pos
        if name:
            marks[name] = (pos, n)
        parts.append(np.full(n, key, dtype=np.int64))
        pos += n

    put("len64_lane0", 5, 64)                       # [0, 64)
    put("len63_lane0", 6, 63)                       # [64, 127)
    put("len1_lane63", 7, 1)                        # [127, 128)
    put("len65_lane0", 8, 65)                       # [128, 193)
    put("aba", 9, 1); put(None, 10, 1); put(None, 9, 1)
    k = 11
    while pos < 250:                                # single keys up to the next mark
        put(None, k, 1)
        k = 11 + (k - 10) % 8
    put("len128_block_edge", 20, 128)               # [250, 378): over thread 255 | 256
    k = 11
    while pos % 64 != 63:
        put(None, k, 1)
        k = 11 + (k - 10) % 8
    put("len300_lane63", 21, 300)                   # [383, 683): begins on the last lane of a wave, spans a block edge
    put("clamped_run", R - 1, 10)                   # natural R - 1, then bad keys that clamp to R - 1, then natural again: ONE run
    for v in _bad(BAD_IDS, R) + [R + 3, -7, 2 ** 40]:
        put(None, v, 1)
    put(None, R - 1, 5)
    marks["clamped_run"] = (marks["clamped_run"][0], 22)
    tail = 64 + (1 - (pos + 64)) % 64               # random keys up to a count of 64 k + 1
    parts.append(rng.integers(0, R - 1, tail))
    pos += tail
    keys = np.concatenate(parts).astype(np.int64)
    other = rng.integers(0, 10 ** 6, keys.shape[0]).astype(np.int64)
    return keys, R, other, marks


def runs_single_row_case():
    """(keys, 1, other): R = 1 -- every key is row 0, the bad ones after clamping; 130 keys = two waves and two lanes."""
    keys = np.zeros(130, dtype=np.int64)
    keys[[0, 63, 64, 100, 129]] = [1, -1, 2 ** 31 + 5, -2 ** 40, 7]
    return keys, 1, np.arange(130, dtype=np.int64)[::-1].copy()


SWITCH_N, SWITCH_HUB = 5000, 300


def switch_pair_sizes():
    """[last E at which the pair build counts, first E at which it sorts]."""
    limit = counting_limits()[2]
    return [limit // 2, limit // 2 + 1]


def switch_csr_sizes():
    """[last, first] key counts for gsat_build_csr: it compares 2 * (keys / 2) with the limit, so an odd count one above it still counts."""
    limit = counting_limits()[2]
    return [limit + 1, limit + 2]


def switch_pair_case(E: int, seed: int = 21):
    """(ei, N): E edges over 5000 nodes; node 0 receives exactly 300 (the only row with hub chunks), scattered by a permutation."""
    rng = np.random.default_rng(seed)
    dst = np.concatenate([np.zeros(SWITCH_HUB, dtype=np.int64), rng.integers(1, SWITCH_N, E - SWITCH_HUB)])
    src = rng.integers(0, SWITCH_N, E)
    perm = rng.permutation(E)
    return np.stack([src[perm], dst[perm]]).astype(np.int64), SWITCH_N


def switch_csr_case(n: int, seed: int = 22):
    """(keys, R, other) for gsat_build_csr at n keys."""
    rng = np.random.default_rng(seed)
    keys = np.concatenate([np.zeros(SWITCH_HUB, dtype=np.int64), rng.integers(1, SWITCH_N, n - SWITCH_HUB)])[rng.permutation(n)]
    return keys.astype(np.int64), SWITCH_N, rng.integers(0, 2 ** 31 - 1, n).astype(np.int64)


def _both_ways(pairs, mult):
    src, dst = [], []
    for (u, v), m in zip(pairs, mult):
        src += [u] * m + ([v] * m if u != v else [])
        dst += [v] * m + ([u] * m if u != v else [])
    return np.array([src, dst], dtype=np.int64).reshape(2, -1)


def rev_multigraph_case(seed: int = 31, N: int = 200):
    """(a) (ei, N): symmetric multigraph, one to three copies of every edge, self loops (some twice), node 0 a hub of 150 neighbours."""
    rng = np.random.default_rng(seed)
    pairs = {(int(min(u, v)), int(max(u, v))) for u, v in rng.integers(1, N, size=(300, 2)) if u != v}
    pairs |= {(0, int(v)) for v in rng.permutation(np.arange(1, N))[:150]}
    pairs |= {(int(v), int(v)) for v in rng.permutation(N)[:12]}
    pairs = sorted(pairs)
    ei = _both_ways(pairs, rng.integers(1, 4, len(pairs)).tolist())
    return ei[:, rng.permutation(ei.shape[1])], N


def rev_asymmetric_case():
    """(b) (ei, N, removed): (a) without one non-loop edge."""
    ei, N = rev_multigraph_case()
    e = int(np.flatnonzero(ei[0] != ei[1])[17])
    return np.delete(ei, e, axis=1), N, e


REV_BRANCH_KINDS = ("hub_to_leaf", "leaf_to_hub", "hub_to_hub", "equal")


def rev_branch_case(seed: int = 33):
    """(c) (ei, N, kind): every edge twice or three times, so every kind of edge meets a copy index k >= 1.  Hubs 0 (40 leaves), 1 (30
    leaves), 2 and 3 (25 leaves each: equal lengths); hub-hub edges 0-1 (unequal) and 2-3 (equal); isolated pairs of equal degree.
    ``kind[e]`` names the edge: index into REV_BRANCH_KINDS.  The edge set is symmetric, so out-degree = in-degree at every node and the
    two choices of k_rev_from_csr always agree; the two mixed combinations need an asymmetric input, where rev is not specified."""
    rng = np.random.default_rng(seed)
    pairs, mult, leaf = [], [], 4
    for hub, n in ((0, 40), (1, 30), (2, 25), (3, 25)):
        pairs += [(hub, leaf + i) for i in range(n)]
        mult += [2 + (i % 2) for i in range(n)]
        leaf += n
    pairs += [(0, 1), (2, 3)]
    pairs += [(leaf + 2 * i, leaf + 2 * i + 1) for i in range(6)]
    N = leaf + 12
    mult += [3, 2] + [2] * 6
    ei = _both_ways(pairs, mult)
    ei = ei[:, rng.permutation(ei.shape[1])]
    hub = ei < 4
    deg = np.bincount(ei[0], minlength=N)
    kind = np.where(hub[0] & hub[1], 2, np.where(hub[0], 0, np.where(hub[1], 1, 3)))
    kind = np.where(deg[ei[0]] == deg[ei[1]], 3, kind)
    return ei, N, kind


def rev_wide_case(seed: int = 35):
    """(d) (ei, N): N = 2^31 - 1 with ids from {0, 1, N - 2, N - 1} -- the largest keys the sort entry point accepts (62 key bits, its half
    bit on bit 62).  A symmetric multigraph with loops; nothing of size N exists anywhere."""
    rng = np.random.default_rng(seed)
    N = 2 ** 31 - 1
    ids = [0, 1, N - 2, N - 1]
    pairs = [(ids[i], ids[j]) for i in range(4) for j in range(i, 4)]          # loops included
    ei = _both_ways(pairs, rng.integers(1, 4, len(pairs)).tolist())
    return ei[:, rng.permutation(ei.shape[1])], N


def segments_cases():
    """[(name, ids, G, valid)]"""
    rng = np.random.default_rng(41)
    out = []
    for n in (0, 1, 255, 256, 257):
        G = 9
        out.append((f"n{n}", np.sort(rng.integers(0, G, n)).astype(np.int64), G, True))
    out.append(("G_far_above_n", np.array([5, 5, 699], dtype=np.int64), 700, True))
    out.append(("empty_first_middle_last", np.sort(rng.choice([2, 3, 6, 7], 40)).astype(np.int64), 10, True))
    out.append(("G0", np.zeros(0, dtype=np.int64), 0, True))
    # two descents (3 -> 2, 4 -> 3), a -1 in front and a G at the end: four bad elements.  The pointers of an unsorted vector are not
    # specified (rule: they stay in [0, n]); the clamped ids and the bad count are
    out.append(("invalid", np.array([-1, 0, 1, 3, 2, 2, 4, 3, 5, 5, 6], dtype=np.int64), 6, False))
    return out


def edge_segments_case(seed: int = 43):
    """(ei, batch, G, N): 8 graphs of 6 nodes; graphs 0, 4 and 7 (first, a middle one, last) have no edge; edges stay inside a graph but
    their order is shuffled."""
    rng = np.random.default_rng(seed)
    G, n = 8, 6
    batch = np.repeat(np.arange(G), n).astype(np.int64)
    cols = []
    for g in (1, 2, 3, 5, 6):
        m = int(rng.integers(3, 40))
        cols.append(rng.integers(g * n, (g + 1) * n, size=(2, m)))
    ei = np.concatenate(cols, axis=1).astype(np.int64)
    return ei[:, rng.permutation(ei.shape[1])], batch, G, G * n


DUAL_OUT_DEGREES = (0, 1, 2, 0, 1, 3, 4, 300, 2, 0, 3, 1, 0)


def dual_by_source_case(seed: int = 51):
    """(ei, N, batch): source-sorted edges with the out-degrees above: degree 0 and 1 at the very front, at the very end, and between two
    rows that have pairs (nodes 3, 4 and node 9).  Three graphs by node range, for the dual batch vector."""
    rng = np.random.default_rng(seed)
    N = len(DUAL_OUT_DEGREES)
    src = np.repeat(np.arange(N), DUAL_OUT_DEGREES)
    ei = np.stack([src, rng.integers(0, N, src.shape[0])]).astype(np.int64)
    batch = np.array([0] * 5 + [1] * 4 + [2] * 4, dtype=np.int64)
    return ei, N, batch


def dual_undirected_case(seed: int = 53, leaves: int = 300):
    """(ei, N, batch, ei_without_loop): graph 0 a star of ``leaves`` leaves round node 0, graph 1 a triangle with a tail; five directed
    edges duplicated and one self loop, shuffled.  The loop is the last column of ei."""
    rng = np.random.default_rng(seed)
    b = leaves + 1
    und = [(0, i) for i in range(1, leaves + 1)] + [(b, b + 1), (b + 1, b + 2), (b, b + 2), (b + 2, b + 3), (b + 3, b + 4)]
    ei = _both_ways(und, [1] * len(und))
    ei = np.concatenate([ei, ei[:, [0, 7, leaves + 5, ei.shape[1] - 1, ei.shape[1] - 4]]], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    N = b + 5
    batch = np.array([0] * b + [1] * 5, dtype=np.int64)
    loop = np.array([[b + 1], [b + 1]], dtype=np.int64)
    return np.concatenate([ei, loop], axis=1), N, batch, ei
