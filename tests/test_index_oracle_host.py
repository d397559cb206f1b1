"""CPU: the numpy restatements of tests/index_oracle.py agree with the independent ones of oracle/bookkeeping.py, and every boundary
its case table claims is present in the generated arrays -- asserted here, so that a later edit of a builder that loses a boundary
fails on a machine without a GPU instead of quietly testing less on one."""
import os

import numpy as np
import pytest

from oracle import bookkeeping as obk
from tests import index_oracle as io


# ---- constants ------------------------------------------------------------------------------------------------------------------------
def test_constants_come_from_the_header_and_the_library():
    assert io.long_row_edges() == 256
    assert io.counting_limits() == (1024, 4096, 1 << 20)
    assert io.rows_degrees() == [255, 256, 257, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193]
    assert io.switch_pair_sizes() == [524288, 524289] and io.switch_csr_sizes() == [(1 << 20) + 1, (1 << 20) + 2]
    env = os.environ.get("GSAT_CSR_COUNTING")
    if env is None:             # the default of the process: counting up to the limit.  (The library reads the switch once.)
        assert [io.csr_counts(2 * e) for e in io.switch_pair_sizes()] == [1, 0]
        assert [io.csr_counts(n) for n in io.switch_csr_sizes()] == [1, 0]
        assert io.csr_counts(0) == 1 and io.csr_counts(2) == 1
    elif env == "0":
        assert io.csr_counts(2) == 0


# ---- the restatements against oracle/bookkeeping.py ---------------------------------------------------------------------------------------
def _valid_pair_cases():
    cases = [(name, ei, N) for name, ei, N in io.tiny_cases()]
    ei, N = io.rows_case()
    cases += [("rows", ei, N), ("rows_T", ei[::-1].copy(), N)]
    cases.append(("short",) + io.short_rows_case())
    cases += [(f"switch_{E}", *io.switch_pair_case(E)) for E in io.switch_pair_sizes()]
    for name, c in (("rev_a", io.rev_multigraph_case()), ("rev_b", io.rev_asymmetric_case()[:2]), ("rev_c", io.rev_branch_case()[:2])):
        cases.append((name, c[0], c[1]))
    return cases


def test_csr_and_pair_agree_with_csr_by():
    for name, ei, N in _valid_pair_cases():
        p = io.pair(ei, N)
        E = ei.shape[1]
        if E == 0:
            assert not p["rowptr_dst"].any() and not p["rowptr_src"].any() and not p["status"].any(), name
            continue
        for rows, other, rp, eid, oth in ((ei[1], ei[0], "rowptr_dst", "eid_by_dst", "src_by_dst"),
                                          (ei[0], ei[1], "rowptr_src", "eid_by_src", "dst_by_src")):
            rowptr, perm = obk.csr_by(rows, N)
            assert np.array_equal(p[rp], rowptr) and np.array_equal(p[eid], perm) and np.array_equal(p[oth], other[perm]), name
            r2, p2, o2 = io.csr(rows, other, N)
            assert np.array_equal(r2, rowptr) and np.array_equal(p2, perm) and np.array_equal(o2, other[perm]), name
        # the slot map sends slot k of the by-source CSR to the slot of the same edge in the by-destination CSR
        assert np.array_equal(p["eid_by_dst"][p["slot_dst_of_srcslot"]], p["eid_by_src"]), name
        assert np.array_equal(p["src32"], ei[0]) and np.array_equal(p["dst32"], ei[1]) and p["status"][0] == 0, name
        # chunk pointers, restated once more without a scan: row r owns ceil(deg / L) chunks iff deg > L
        L = io.long_row_edges()
        for rp, cp, word in (("rowptr_dst", "chunk_ptr_dst", 1), ("rowptr_src", "chunk_ptr_src", 2)):
            deg = np.diff(p[rp]).tolist()
            want = [0]
            for d in deg:
                want.append(want[-1] + (-(-d // L) if d > L else 0))
            assert p[cp].tolist() == want and p["status"][word] == want[-1] and p["status"][3] == 0, name


def test_bad_ids_are_clamped_before_everything_else():
    """csr / pair on raw ids = csr_by on the ids clamped to the last row (the documented rule), for the key column and the edge list."""
    for keys, R, other in (io.runs_case()[:3], io.runs_single_row_case(), io.switch_csr_case(io.switch_csr_sizes()[0])):
        clamped, _ = io.clamp_ids(keys, R)
        rowptr, perm = obk.csr_by(clamped, R)
        r2, p2, o2 = io.csr(keys, other, R)
        assert np.array_equal(r2, rowptr) and np.array_equal(p2, perm) and np.array_equal(o2, other[perm]) and r2[-1] == keys.shape[0]
    ei, N, _ = io.bad_ids_case()
    ec = np.stack([io.clamp_ids(ei[0], N)[0], io.clamp_ids(ei[1], N)[0]])
    p, pc = io.pair(ei, N), io.pair(ec, N)
    for k in io.PAIR_OUTPUTS:
        assert np.array_equal(p[k], pc[k]), k
    assert p["status"][0] == 12 and pc["status"][0] == 0 and np.array_equal(p["eid_by_dst"], obk.csr_by(ec[1], N)[1])


def test_reverse_perm_agrees_with_reverse_edge_perm_and_is_undirected():
    cases = [(n, ei, N) for n, ei, N in _valid_pair_cases() if not n.startswith("switch")]
    cases.append(("rev_d",) + io.rev_wide_case())
    seen = set()
    for name, ei, N in cases:
        rev, unmatched = io.reverse_perm(ei, N)
        und = obk.is_undirected(ei, N)
        assert (unmatched == 0) == und, name
        seen.add(und)
        assert np.array_equal(np.sort(rev), np.arange(ei.shape[1])), name          # a permutation either way
        if und:
            assert np.array_equal(rev, obk.reverse_edge_perm(ei, N)), name
            assert np.array_equal(ei[:, rev], ei[::-1]) and np.array_equal(rev[rev], np.arange(ei.shape[1])), name
            assert np.array_equal(io.copy_index(ei, N)[rev], io.copy_index(ei, N)), name          # k-th copy meets k-th copy
        else:
            with pytest.raises(ValueError):
                obk.reverse_edge_perm(ei, N)
    assert seen == {True, False}


def test_segments_and_edge_segments_agree_with_graph_ptr():
    for name, ids, G, valid in io.segments_cases():
        ptr, clamped, bad = io.segments(ids, G)
        assert (bad == 0) == valid, name
        if valid:
            assert np.array_equal(ptr, obk.graph_ptr(ids, G)) and np.array_equal(clamped, ids), name
    ei, batch, G, N = io.edge_segments_case()
    eptr, order, eg = io.edge_segments(ei, batch, G)
    rowptr, perm = obk.csr_by(batch[ei[0]], G)
    assert np.array_equal(eptr, rowptr) and np.array_equal(order, perm) and np.array_equal(eg, batch[ei[0]])
    assert np.array_equal(eptr, obk.graph_ptr(np.sort(eg), G))


# ---- every boundary the case table claims ---------------------------------------------------------------------------------------------------
def test_tiny_cases_cover_the_sizes_with_loops_and_repeats():
    cases = io.tiny_cases()
    assert {(ei.shape[1], N) for _, ei, N in cases} == {(E, N) for E in (0, 1, 2, 63, 64, 65, 255, 256, 257) for N in (1, 2, 50)}
    for name, ei, N in cases:
        E = ei.shape[1]
        assert ei.dtype == np.int64 and (E == 0 or (ei.min() >= 0 and ei.max() < N)), name
        if E >= 1:
            assert (ei[0] == ei[1]).any(), name
        if E >= 2:
            assert (io.copy_index(ei, N) >= 1).any(), name


def test_rows_case_has_exactly_the_listed_degrees():
    ei, N = io.rows_case()
    want = io.rows_degrees()
    indeg = np.bincount(ei[1], minlength=N)
    assert indeg[:len(want)].tolist() == want
    assert indeg[len(want):].max() < io.long_row_edges() - 1             # nothing else comes near a limit
    assert np.bincount(ei[0], minlength=N).max() < io.long_row_edges() - 1
    assert ei.shape[1] == sum(want) + 3000 and 36000 < ei.shape[1] < 38000
    outdeg_T = np.bincount(ei[::-1][0], minlength=N)                      # the transposed batch puts the same rows on the by-source side
    assert outdeg_T[:len(want)].tolist() == want
    # scattered: the edge ids of the longest row span the whole list and are not one block
    ids = np.flatnonzero(ei[1] == len(want) - 1)
    assert ids[0] < 100 and ids[-1] > ei.shape[1] - 100 and (np.diff(ids) > 1).sum() > 1000
    assert (io.copy_index(ei, N) >= 1).any()                              # multi-edges
    L = io.long_row_edges()
    p = io.pair(ei, N)
    assert np.diff(p["chunk_ptr_dst"])[:len(want)].tolist() == [0, 0, 2, 2, 3, 4, 4, 5, 16, 16, 17, 32, 33] and L == 256
    assert p["status"].tolist() == [0, 134, 0, 0]
    ei2, N2 = io.short_rows_case()
    assert max(np.bincount(ei2[0], minlength=N2).max(), np.bincount(ei2[1], minlength=N2).max()) < 32
    assert obk.is_undirected(ei2, N2)


def test_bad_ids_case_plants_every_kind_in_either_row():
    ei, N, planted = io.bad_ids_case()
    E = ei.shape[1]
    assert E == 2000 and E % 64 == 16
    bad = (ei < 0) | (ei >= N)
    assert int(bad.sum()) == len(planted) == 12
    for row in (0, 1):
        assert {-1, N, 2 ** 31 + 5, -2 ** 40} <= set(ei[row][bad[row]].tolist())
    assert int((bad[0] & bad[1]).sum()) == 1                              # one edge with both ends bad: it counts 2
    last_wave = np.arange(E) >= E - E % 64
    assert (bad[0] & last_wave).any() and (bad[1] & last_wave).any() and bad[1, E - 1]
    p = io.pair(ei, N)
    assert p["status"][0] == 12
    assert p["src32"].max() == N - 1 and p["src32"].min() >= 0 and p["dst32"].max() == N - 1 and p["dst32"].min() >= 0
    assert np.array_equal(p["src32"][~bad[0]], ei[0][~bad[0]]) and (p["src32"][bad[0]] == N - 1).all()
    assert np.diff(p["rowptr_dst"])[N - 1] >= int(bad[1].sum()) and np.diff(p["rowptr_src"])[N - 1] >= int(bad[0].sum())


def test_runs_case_places_its_runs_on_the_lanes_it_names():
    keys, R, other, marks = io.runs_case()
    n = keys.shape[0]
    assert n % 64 == 1 and other.shape == keys.shape
    clamped, nbad = io.clamp_ids(keys, R)
    assert nbad == 7
    start, length, key = io.run_lengths(clamped)
    runs = {int(s): (int(l), int(k)) for s, l, k in zip(start, length, key)}
    want = {"len64_lane0": (64, 0), "len63_lane0": (63, 0), "len1_lane63": (1, 63), "len65_lane0": (65, 0), "aba": (1, None),
            "len128_block_edge": (128, None), "len300_lane63": (300, 63), "clamped_run": (22, None)}
    assert set(marks) == set(want)
    for name, (ln, lane) in want.items():
        s, l = marks[name]
        assert l == ln and s in runs and runs[s][0] == ln, name              # a maximal run of exactly that length begins there
        assert lane is None or s % 64 == lane, name
    assert {1, 63, 64, 65, 128, 300} <= set(length.tolist())
    s, l = marks["len128_block_edge"]
    assert s // 256 != (s + l - 1) // 256 and s % 256 != 0                 # it straddles thread 255 | 256
    s, l = marks["len300_lane63"]
    assert (s + l - 1) // 256 - s // 256 == 1 and (s + l - 1) // 64 - s // 64 == 5          # over a block edge and five wave edges
    s, _ = marks["aba"]
    assert keys[s] == keys[s + 2] != keys[s + 1] and runs[s + 1][0] == 1 and runs[s + 2][0] == 1
    s, l = marks["clamped_run"]
    raw = keys[s:s + l]
    inside = (raw >= 0) & (raw < R)
    assert (raw[inside] == R - 1).all() and inside[0] and inside[-1] and int((~inside).sum()) == 7 and (clamped[s:s + l] == R - 1).all()
    assert s // 64 != (s + l - 1) // 64                                       # and it crosses a wave
    k1, R1, o1 = io.runs_single_row_case()
    assert R1 == 1 and io.clamp_ids(k1, 1)[1] == 5 and k1.shape[0] == 130 and not io.clamp_ids(k1, 1)[0].any()


def test_switch_cases_sit_on_either_side_of_the_key_limit():
    limit = io.counting_limits()[2]
    lo, hi = io.switch_pair_sizes()
    assert 2 * lo == limit and 2 * hi == limit + 2
    ei, N = io.switch_pair_case(lo)
    indeg, outdeg = np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)
    assert N == 5000 and ei.shape == (2, lo) and indeg[0] == 300 and indeg[1:].max() <= io.long_row_edges() and outdeg.max() <= io.long_row_edges()
    assert io.pair(ei, N)["status"].tolist() == [0, 2, 0, 0]
    ids = np.flatnonzero(ei[1] == 0)
    assert ids[-1] - ids[0] > lo // 2                                         # the hub's edges are scattered
    keys, R, other = io.switch_csr_case(io.switch_csr_sizes()[0])
    assert keys.shape[0] == limit + 1 and R == 5000 and keys.min() == 0 and keys.max() == R - 1 and other.shape == keys.shape


def test_rev_cases_take_the_branches_they_name():
    ei, N = io.rev_multigraph_case()
    k = io.copy_index(ei, N)
    loops = ei[0] == ei[1]
    assert obk.is_undirected(ei, N) and k.max() == 2 and (k[loops] >= 1).any() and loops.sum() >= 12
    assert np.bincount(ei[0], minlength=N)[0] >= 150 and np.bincount(ei[0], minlength=N)[1:].max() < 40
    assert (np.diff(np.flatnonzero(ei[0] == 0)) > 1).any()                    # shuffled
    eib, Nb, removed = io.rev_asymmetric_case()
    assert eib.shape[1] == ei.shape[1] - 1 and ei[0, removed] != ei[1, removed] and not obk.is_undirected(eib, Nb)
    assert io.reverse_perm(eib, Nb)[1] > 0
    # (c): the two choices per edge, and a copy index k >= 1 under each kind of edge
    eic, Nc, kind = io.rev_branch_case()
    assert obk.is_undirected(eic, Nc)
    c1, c2 = io.rev_branches(eic, Nc)
    assert np.array_equal(c1, c2)                    # a symmetric edge set has out-degree = in-degree: the mixed combinations cannot occur
    kc = io.copy_index(eic, Nc)
    deg = np.bincount(eic[0], minlength=Nc)
    ds, dd = deg[eic[0]], deg[eic[1]]
    for i, name in enumerate(io.REV_BRANCH_KINDS):
        sel = kind == i
        assert sel.any() and (kc[sel] >= 1).any(), name
    assert (ds[kind == 0] > dd[kind == 0]).all() and not c1[kind == 0].any() and not c2[kind == 0].any()          # hub -> leaf: both walk d's rows
    assert (ds[kind == 1] < dd[kind == 1]).all() and c1[kind == 1].all() and c2[kind == 1].all()                  # leaf -> hub: both walk s's rows
    hh = kind == 2
    assert (ds[hh] > 50).all() and (dd[hh] > 50).all() and (ds[hh] != dd[hh]).all()
    assert (kc[hh & c1] >= 1).any() and (kc[hh & ~c1] >= 1).any()                                                 # hub -> hub, each way round
    eq = kind == 3
    assert (ds[eq] == dd[eq]).all() and c1[eq].all() and c2[eq].all() and (ds[eq] > 50).any() and (ds[eq] < 5).any()
    # (d): the widest keys
    eid, Nd = io.rev_wide_case()
    assert Nd == 2 ** 31 - 1 and io.rev_key_bits(Nd) == 62 and set(np.unique(eid).tolist()) == {0, 1, Nd - 2, Nd - 1}
    assert int(io.edge_keys_u64(eid, Nd).max()) == Nd * Nd - 1 and int(io.edge_keys_u64(eid, Nd).max()) >> 61 == 1
    assert io.reverse_perm(eid, Nd)[1] == 0 and io.copy_index(eid, Nd).max() >= 1 and (eid[0] == eid[1]).any()


def test_segments_cases_have_the_shapes_they_name():
    cases = {name: (ids, G, valid) for name, ids, G, valid in io.segments_cases()}
    assert [cases[f"n{n}"][0].shape[0] for n in (0, 1, 255, 256, 257)] == [0, 1, 255, 256, 257]
    ids, G, _ = cases["G_far_above_n"]
    assert ids.shape[0] == 3 and G == 700 and ids[-1] == G - 1
    ids, G, _ = cases["empty_first_middle_last"]
    cnt = np.bincount(ids, minlength=G)
    assert cnt[0] == 0 and cnt[1] == 0 and cnt[4] == 0 and cnt[5] == 0 and cnt[8] == 0 and cnt[9] == 0 and (cnt[[2, 3, 6, 7]] > 0).all()
    ids, G, valid = cases["invalid"]
    desc = ids[:-1] > ids[1:]
    assert not valid and int(desc.sum()) == 2 and ids[0] == -1 and ids[-1] == G and io.segments(ids, G)[2] == 4
    assert io.segments(ids, G)[1].tolist() == [0, 0, 1, 3, 2, 2, 4, 3, 5, 5, 5]
    ei, batch, G, N = io.edge_segments_case()
    per_graph = np.bincount(batch[ei[0]], minlength=G)
    assert per_graph[0] == 0 and per_graph[4] == 0 and per_graph[G - 1] == 0 and (per_graph[[1, 2, 3, 5, 6]] > 0).all()
    assert (np.diff(batch[ei[0]]) < 0).any() and np.array_equal(batch[ei[0]], batch[ei[1]])


def test_dual_cases_have_the_degrees_they_name():
    ei, N, batch = io.dual_by_source_case()
    deg = np.bincount(ei[0], minlength=N).tolist()
    assert deg == list(io.DUAL_OUT_DEGREES) and {0, 1, 2, 3, 4, 300} == set(deg)
    assert (np.diff(ei[0]) >= 0).all()                                        # source-sorted: the oracle's group order is the kernel's
    assert deg[:2] == [0, 1] and deg[-2:] == [1, 0] and deg[2] > 1 and deg[3:5] == [0, 1] and deg[5] > 1 and deg[8] > 1 and deg[9] == 0 and deg[10] > 1
    assert batch.shape[0] == N and (np.diff(batch) >= 0).all()
    eu, Nu, bu, eu_no_loop = io.dual_undirected_case()
    directed = set(map(tuple, eu.T.tolist()))
    assert directed == {(d, s) for s, d in directed}                         # symmetric as a SET: the duplicates are of one direction only
    assert eu[0, -1] == eu[1, -1] and int((eu[0] == eu[1]).sum()) == 1
    assert np.array_equal(eu[:, :-1], eu_no_loop)
    assert len({(min(s, d), max(s, d)) for s, d in eu_no_loop.T.tolist()}) == 305 and eu_no_loop.shape[1] == 2 * 305 + 5
    assert int((io.copy_index(eu, Nu) >= 1).sum()) == 5
    assert np.bincount(eu[0], minlength=Nu)[0] >= 300 and (np.diff(np.flatnonzero(eu[0] == 0)) > 1).any()
    b = 301
    tri = {(b, b + 1), (b + 1, b + 2), (b, b + 2)}
    assert tri <= {(min(s, d), max(s, d)) for s, d in eu.T.tolist()} and bu[b] == 1 and bu[b - 1] == 0
