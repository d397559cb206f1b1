"""-m gpu: the index builders on every build path against the numpy restatements of tests/index_oracle.py -- the counting builds and
the rocPRIM sort builds of gsat_build_csr_pair / gsat_build_csr (the sort builds at small sizes in one child process started with
GSAT_CSR_COUNTING=0, and on either side of the key limit in both), gsat_row_chunks and the GSAT_CSR_PAIR=0 two-call build, both
reverse-permutation entry points, both segment-pointer entry points, edge_segments and the two line graphs.

Everything is an exact integer comparison.  Calls through the C ABI write into views of larger buffers prefilled with a sentinel no
valid index equals, with a workspace of exactly the advertised size and guard words round everything; every call is made twice, since
the counting build fills its rows in atomic order and the result must not depend on it.  Which build ran is asked of the library
(gsat_csr_counts), in the parent and in the child.  The guards are passive: no case asks a kernel to step outside its buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import bookkeeping as obk
from tests import index_oracle as io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -0x5A5A5A5B          # no row pointer, edge id, node id, slot, chunk count or status word is negative (und_of_edge's -1 aside)
GUARD = 64                  # int32 words in front of and behind every output
WS_GUARD = 256              # bytes in front of and behind the workspace
_IN_CHILD = False


def _stop(msg):
    """A HIP error ends the run: nothing more is started on a device that has faulted."""
    if _IN_CHILD:
        print("HIP ERROR " + msg, flush=True)
        sys.exit(3)
    pytest.exit("HIP error, stopping the run: " + msg, returncode=3)


def _call(name, *args):
    from dp_gsat_amd import _lib
    try:
        _lib.call(name, *args)
    except _lib.GsatHipError as exc:
        if "(code -1)" in str(exc):
            _stop(str(exc))
        raise


def _sync():
    try:
        torch.cuda.synchronize()
    except Exception as exc:          # noqa: BLE001  (whatever the runtime raises)
        _stop(repr(exc))


def _size(name, *args):
    from dp_gsat_amd import _lib
    return int(getattr(_lib.load(), name)(*args))


def _stream():
    from dp_gsat_amd import _lib
    return _lib.stream()


class Out:
    """int32[n] output: a view into a buffer of sentinels."""

    def __init__(self, n, dev, fill=None):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        if fill is not None:
            self.buf[GUARD:GUARD + self.n] = fill
        self.p = self.buf.data_ptr() + 4 * GUARD

    def get(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == SENT).all() and (b[GUARD + self.n:] == SENT).all(), f"{what}: guard words overwritten"
        v = b[GUARD:GUARD + self.n]
        assert not (v == SENT).any(), f"{what}: {int((v == SENT).sum())} of {self.n} words never written"
        return v.astype(np.int64)


class Work:
    """Workspace of exactly n bytes with guard bytes round it."""

    def __init__(self, n, dev):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * WS_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.p = self.buf.data_ptr() + WS_GUARD

    def check(self, what):
        assert bool((self.buf[:WS_GUARD] == 0xA5).all()) and bool((self.buf[WS_GUARD + self.n:] == 0xA5).all()), f"{what}: wrote past its workspace"


def _dev_i64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def _dev_i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(dev)


def _p(t):
    return t.data_ptr() if t is not None and t.numel() else None


# ---- the two CSR entry points through the C ABI -------------------------------------------------------------------------------------------
def run_pair(dev, name, ei, N, counts):
    """gsat_build_csr_pair twice on (ei, N): all eleven outputs and status[0:4] equal numpy both times; the build that ran is ``counts``."""
    E = int(ei.shape[1])
    assert io.csr_counts(2 * E) == counts, f"{name}: expected the {'counting' if counts else 'sort'} build"
    want = io.pair(ei, N)
    ei_d = _dev_i64(ei, dev)
    nbytes = _size("gsat_csr_pair_workspace_bytes", E, N)
    got = None
    for rep in range(2):
        outs = {k: Out(N + 1 if k.startswith(("rowptr", "chunk")) else E, dev) for k in io.PAIR_OUTPUTS}
        status, ws = Out(4, dev), Work(nbytes, dev)
        _call("gsat_build_csr_pair", _p(ei_d), E, N, *[outs[k].p for k in io.PAIR_OUTPUTS], status.p, ws.p, nbytes, _stream())
        _sync()
        ws.check(name)
        got = {k: outs[k].get(f"{name}.{k}") for k in io.PAIR_OUTPUTS}
        got["status"] = status.get(f"{name}.status")
        for k in io.PAIR_OUTPUTS + ("status",):
            assert np.array_equal(got[k], want[k]), f"{name} (call {rep}): {k} differs at {np.flatnonzero(got[k] != want[k])[:8].tolist()}"
    return got


def run_csr(dev, name, keys, R, other, counts):
    """gsat_build_csr twice on one key column, with other / other_sorted or with both NULL."""
    n = int(keys.shape[0])
    assert io.csr_counts(n) == counts, f"{name}: expected the {'counting' if counts else 'sort'} build"
    rowptr, perm, other_sorted = io.csr(keys, other, R)
    nbad = io.clamp_ids(keys, R)[1]
    keys_d = _dev_i64(keys, dev)
    other_d = None if other is None else _dev_i64(other, dev)
    nbytes = _size("gsat_csr_workspace_bytes", n, R)
    for rep in range(2):
        o_rowptr, o_perm, o_err, ws = Out(R + 1, dev), Out(n, dev), Out(1, dev, fill=0), Work(nbytes, dev)          # err_flag is caller-zeroed
        o_other = None if other is None else Out(n, dev)
        _call("gsat_build_csr", _p(keys_d), _p(other_d), n, R, o_rowptr.p, None if other is None else o_other.p, o_perm.p, o_err.p, ws.p,
              nbytes, _stream())
        _sync()
        ws.check(name)
        what = f"{name} (call {rep})"
        assert np.array_equal(o_rowptr.get(name + ".rowptr"), rowptr), what
        got = o_perm.get(name + ".perm")
        assert np.array_equal(got, perm), f"{what}: perm differs at {np.flatnonzero(got != perm)[:8].tolist()}"
        assert o_err.get(name + ".err").tolist() == [nbad], what
        if other is not None:
            assert np.array_equal(o_other.get(name + ".other_sorted"), other_sorted), what


def _small_build_cases():
    """[(name, kind, args)] of everything both build paths run below the key limit."""
    cases = [(name, "pair", (ei, N)) for name, ei, N in io.tiny_cases()]
    ei, N = io.rows_case()
    cases += [("rows", "pair", (ei, N)), ("rows_T", "pair", (ei[::-1].copy(), N))]
    ei, N, _ = io.bad_ids_case()
    cases.append(("bad_ids", "pair", (ei, N)))
    keys, R, other, _ = io.runs_case()
    cases += [("runs_other", "csr", (keys, R, other)), ("runs_null", "csr", (keys, R, None))]
    keys, R, other = io.runs_single_row_case()
    cases += [("runs_R1_other", "csr", (keys, R, other)), ("runs_R1_null", "csr", (keys, R, None))]
    return cases


def _switch_cases():
    """[(name, kind, builder)]: the four large cases, built only when they run."""
    cases = [(f"switch_pair_{E}", "pair", lambda E=E: io.switch_pair_case(E)) for E in io.switch_pair_sizes()]
    cases += [(f"switch_csr_{n}", "csr", lambda n=n: io.switch_csr_case(n)) for n in io.switch_csr_sizes()]
    return cases


def _run(dev, name, kind, args, counts):
    if callable(args):
        args = args()
    if kind == "pair":
        run_pair(dev, name, args[0], args[1], counts)
    else:
        run_csr(dev, name, args[0], args[1], args[2], counts)


def test_library_agrees_with_the_constants_of_the_case_table(dev):
    assert io.long_row_edges() == 256 and io.counting_limits() == (1024, 4096, 1 << 20)
    lo, hi = io.switch_pair_sizes()
    assert io.csr_counts(2 * lo) == 1 and io.csr_counts(2 * hi) == 0          # this process counts up to the key limit


def test_counting_pair_build_tiny(dev):
    for name, ei, N in io.tiny_cases():
        run_pair(dev, name, ei, N, counts=1)


@pytest.mark.parametrize("name", ["rows", "rows_T", "bad_ids"])
def test_counting_pair_build(dev, name):
    kind, args = {n: (k, a) for n, k, a in _small_build_cases()}[name]
    _run(dev, name, kind, args, counts=1)


@pytest.mark.parametrize("name", ["runs_other", "runs_null", "runs_R1_other", "runs_R1_null"])
def test_counting_single_csr_build_on_runs(dev, name):
    kind, args = {n: (k, a) for n, k, a in _small_build_cases()}[name]
    _run(dev, name, kind, args, counts=1)


@pytest.mark.parametrize("side", [0, 1])
def test_pair_build_on_either_side_of_the_key_limit(dev, side):
    """E = 524 288 is the last size that counts, 524 289 the first that sorts: the same arrays either way."""
    name, kind, args = _switch_cases()[side]
    _run(dev, name, kind, args, counts=1 - side)


@pytest.mark.parametrize("side", [0, 1])
def test_single_csr_build_on_either_side_of_the_key_limit(dev, side):
    """gsat_build_csr counts up to 2^20 + 1 keys (it halves the key count first) and sorts from 2^20 + 2."""
    name, kind, args = _switch_cases()[2 + side]
    _run(dev, name, kind, args, counts=1 - side)


def run_sort_cases():
    """Body of the child process (GSAT_CSR_COUNTING=0): every small case and both sides of the switch on the sort builds."""
    global _IN_CHILD
    _IN_CHILD = True
    assert os.environ.get("GSAT_CSR_COUNTING") == "0"
    dev = torch.device("cuda:0")
    assert io.csr_counts(2) == 0 and io.csr_counts(0) == 0
    for name, kind, args in _small_build_cases() + _switch_cases():
        _run(dev, name, kind, args, counts=0)
        print(f"sort-build {name} ok", flush=True)
    print("sort-build all ok", flush=True)


def test_sort_builds_in_a_fresh_process(dev):
    """GSAT_CSR_COUNTING is read once per process, so the sort builds of the small cases run in one child started with it set to 0; the
    child compares against numpy itself and reports one line per case."""
    env = dict(os.environ, GSAT_CSR_COUNTING="0")
    try:
        out = subprocess.run([sys.executable, "-c", "from tests.test_gpu_index_paths import run_sort_cases; run_sort_cases()"],
                             capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    except subprocess.TimeoutExpired as exc:
        _stop(f"the sort-build child hung: {exc}")
    tail = (out.stdout + out.stderr)[-3000:]
    if out.returncode < 0 or out.returncode in (3, 134, 139):          # killed by a signal, or it reported a HIP error itself
        _stop("the sort-build child died: " + tail)
    assert out.returncode == 0, tail
    lines = out.stdout.splitlines()
    for name, _, _ in _small_build_cases() + _switch_cases():
        assert f"sort-build {name} ok" in lines, (name, tail)
    assert lines[-1] == "sort-build all ok", tail


# ---- gsat_row_chunks and the two-call build -----------------------------------------------------------------------------------------------
def test_row_chunks_against_numpy_and_the_pair_build(dev):
    L = io.long_row_edges()
    ei, N = io.rows_case()
    ei2, N2 = io.short_rows_case()
    pair_rows = run_pair(dev, "rows", ei, N, counts=1)
    pair_short = run_pair(dev, "short", ei2, N2, counts=1)
    cases = [("rows_dst", io.pair(ei, N)["rowptr_dst"], pair_rows["chunk_ptr_dst"]), ("rows_src", io.pair(ei, N)["rowptr_src"], pair_rows["chunk_ptr_src"]),
             ("rows_T_src", io.pair(ei[::-1], N)["rowptr_src"], pair_rows["chunk_ptr_dst"]),
             ("short", io.pair(ei2, N2)["rowptr_dst"], pair_short["chunk_ptr_dst"]), ("no_rows", np.zeros(1, dtype=np.int64), None)]
    for name, rowptr, from_pair in cases:
        R = rowptr.shape[0] - 1
        want = io.chunk_ptr(rowptr, L)
        rp_d = _dev_i32(rowptr, dev)
        nbytes = _size("gsat_row_chunks_workspace_bytes", R)
        for rep in range(2):
            out, ws = Out(R + 1, dev), Work(nbytes, dev)
            _call("gsat_row_chunks", rp_d.data_ptr(), R, out.p, ws.p, nbytes, _stream())
            _sync()
            ws.check(name)
            got = out.get(name)
            assert np.array_equal(got, want), (name, rep)
            assert from_pair is None or np.array_equal(got, from_pair), (name, rep)
    assert not pair_short["chunk_ptr_dst"].any() and pair_rows["chunk_ptr_dst"][-1] == 134


INDEX_TENSORS = ("rowptr_dst", "src_by_dst", "eid_by_dst", "rowptr_src", "dst_by_src", "eid_by_src", "slot_dst_of_srcslot", "chunk_ptr_dst",
                 "chunk_ptr_src", "src32", "dst32")


def _index_facts(ix):
    facts = {k: getattr(ix, k).cpu().numpy().astype(np.int64) for k in INDEX_TENSORS}
    facts["long_rows"] = tuple(None if t is None else t.cpu().numpy().astype(np.int64) for t in ix.long_rows)
    rev = ix.rev
    facts["rev"] = None if rev is None else rev.cpu().numpy().astype(np.int64)
    return facts


@pytest.mark.parametrize("case", ["rows", "short"])
def test_two_call_build_equals_the_pair_build(dev, monkeypatch, case):
    """GSAT_CSR_PAIR=0 (read per construction): two gsat_build_csr calls, two gsat_row_chunks calls and a sorted reverse permutation give
    the index of the default build bit for bit.  (bad ids are not run here: src32 of this build is narrowed, not clamped.)"""
    from dp_gsat_amd.graph_index import BatchIndex
    ei, N = io.rows_case() if case == "rows" else io.short_rows_case()
    want = io.pair(ei, N)
    ei_d = _dev_i64(ei, dev)
    monkeypatch.delenv("GSAT_CSR_PAIR", raising=False)
    default = _index_facts(BatchIndex(ei_d, N))
    monkeypatch.setenv("GSAT_CSR_PAIR", "0")
    two_call = _index_facts(BatchIndex(ei_d, N))
    _sync()
    for k in INDEX_TENSORS:
        assert np.array_equal(two_call[k], default[k]) and np.array_equal(default[k], want[k]), k
    for a, b, k in zip(two_call["long_rows"], default["long_rows"], ("chunk_ptr_dst", "chunk_ptr_src")):
        assert (a is None) == (b is None) == (want[k][-1] == 0), k
        assert a is None or (np.array_equal(a, b) and np.array_equal(a, want[k])), k
    rev, unmatched = io.reverse_perm(ei, N)
    if unmatched:          # not symmetric: both builds answer None
        assert two_call["rev"] is None and default["rev"] is None
    else:
        assert np.array_equal(two_call["rev"], rev) and np.array_equal(default["rev"], rev)


# ---- reverse permutation --------------------------------------------------------------------------------------------------------------------
def run_rev_sort(dev, name, ei, N):
    """gsat_reverse_edge_perm (the 2E-key sort) twice; returns (rev, flags) of the second call, the first having been equal."""
    E = int(ei.shape[1])
    ei_d = _dev_i64(ei, dev)
    nbytes = _size("gsat_rev_workspace_bytes", E)
    seen = []
    for rep in range(2):
        rev, flags, ws = Out(E, dev), Out(2, dev), Work(nbytes, dev)
        _call("gsat_reverse_edge_perm", _p(ei_d), E, N, rev.p, flags.p, ws.p, nbytes, _stream())
        _sync()
        ws.check(name)
        seen.append((rev.get(name + ".rev"), flags.get(name + ".flags")))
    assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1]), name
    return seen[1]


def run_rev_csr(dev, name, ei, N):
    """gsat_reverse_edge_perm_csr twice, on the CSRs of the numpy restatement (so the call is judged on its own)."""
    E = int(ei.shape[1])
    p = io.pair(ei, N)
    d = {k: _dev_i32(p[k], dev) for k in ("src32", "dst32", "rowptr_dst", "src_by_dst", "eid_by_dst", "rowptr_src", "dst_by_src", "eid_by_src")}
    seen = []
    for rep in range(2):
        rev, flags = Out(E, dev), Out(2, dev)
        _call("gsat_reverse_edge_perm_csr", _p(d["src32"]), _p(d["dst32"]), _p(d["rowptr_dst"]), _p(d["src_by_dst"]), _p(d["eid_by_dst"]),
              _p(d["rowptr_src"]), _p(d["dst_by_src"]), _p(d["eid_by_src"]), E, N, rev.p, flags.p, _stream())
        _sync()
        seen.append((rev.get(name + ".rev"), flags.get(name + ".flags")))
    assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1]), name
    return seen[1]


@pytest.mark.parametrize("case", ["a", "c"])
def test_reverse_permutation_of_symmetric_multigraphs(dev, monkeypatch, case):
    """Both entry points pair the k-th copy of (s, d) with the k-th copy of (d, s) -- (c) with k >= 1 under each of k_rev_from_csr's row
    choices -- through the C ABI and through BatchIndex with and without GSAT_REV_CSR=0."""
    from dp_gsat_amd.graph_index import BatchIndex
    ei, N = io.rev_multigraph_case() if case == "a" else io.rev_branch_case()[:2]
    want, unmatched = io.reverse_perm(ei, N)
    assert unmatched == 0
    for run in (run_rev_csr, run_rev_sort):
        rev, flags = run(dev, f"rev_{case}", ei, N)
        assert np.array_equal(rev, want), (run.__name__, np.flatnonzero(rev != want)[:8].tolist())
        assert flags.tolist() == [1, 0], run.__name__
    ei_d = _dev_i64(ei, dev)
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("GSAT_REV_CSR", raising=False)
        else:
            monkeypatch.setenv("GSAT_REV_CSR", env)
        ix = BatchIndex(ei_d, N)
        assert ix.is_undirected and np.array_equal(ix.rev.cpu().numpy().astype(np.int64), want), env
        rev_d, flags_d = ix.rev_and_flag
        assert flags_d.tolist() == [1, 0], env


def test_reverse_permutation_of_an_asymmetric_multigraph(dev, monkeypatch):
    """(b): one edge has lost its partner.  Both entry points clear flags[0], count in flags[1] and keep rev inside [0, E).  The sort's rev
    and count are the restated ones; the CSR path's rev is only required to stay in bounds (rule: no value asserted)."""
    from dp_gsat_amd.graph_index import BatchIndex
    ei, N, _ = io.rev_asymmetric_case()
    E = ei.shape[1]
    want, unmatched = io.reverse_perm(ei, N)
    assert unmatched > 0
    rev, flags = run_rev_sort(dev, "rev_b", ei, N)
    assert flags.tolist() == [0, unmatched] and rev.min() >= 0 and rev.max() < E and np.array_equal(rev, want)
    rev, flags = run_rev_csr(dev, "rev_b", ei, N)
    assert flags[0] == 0 and flags[1] > 0 and rev.min() >= 0 and rev.max() < E
    ei_d = _dev_i64(ei, dev)
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("GSAT_REV_CSR", raising=False)
        else:
            monkeypatch.setenv("GSAT_REV_CSR", env)
        ix = BatchIndex(ei_d, N)
        assert not ix.is_undirected and ix.rev is None, env


def test_sorted_reverse_permutation_with_the_widest_keys_and_no_edges(dev):
    """(d): N = 2^31 - 1, keys of 62 bits with the half bit on bit 62 -- the sort entry point only, nothing of size N is allocated.
    E = 0 gives flags [1, 0] from both entry points."""
    ei, N = io.rev_wide_case()
    want, unmatched = io.reverse_perm(ei, N)
    rev, flags = run_rev_sort(dev, "rev_d", ei, N)
    assert unmatched == 0 and np.array_equal(rev, want) and flags.tolist() == [1, 0]
    empty = np.zeros((2, 0), dtype=np.int64)
    for run in (run_rev_sort, run_rev_csr):
        rev, flags = run(dev, "rev_E0", empty, 5)
        assert rev.shape == (0,) and flags.tolist() == [1, 0], run.__name__


# ---- segment pointers -------------------------------------------------------------------------------------------------------------------------
def test_segment_pointers_of_both_entry_points(dev):
    for name, ids, G, valid in io.segments_cases():
        n = int(ids.shape[0])
        ptr, clamped, bad = io.segments(ids, G)
        ids_d = _dev_i64(ids, dev)
        for rep in range(2):
            o_ptr, o_flag = Out(G + 1, dev), Out(1, dev)                       # gsat_segment_ptr zeroes its flag itself
            _call("gsat_segment_ptr", _p(ids_d), n, G, o_ptr.p, o_flag.p, _stream())
            o_ptr32, o_ids32, o_flag32 = Out(G + 1, dev), Out(n, dev), Out(1, dev, fill=5)          # gsat_segment_ptr32 adds to what the word held
            _call("gsat_segment_ptr32", _p(ids_d), n, G, o_ptr32.p, o_ids32.p, o_flag32.p, _stream())
            _sync()
            got, got32 = o_ptr.get(name + ".ptr"), o_ptr32.get(name + ".ptr32")
            if valid:
                assert np.array_equal(got, ptr) and np.array_equal(got32, ptr), name
            else:          # rule: the pointers of an unsorted vector are unspecified beyond staying in [0, n]
                assert got.min() >= 0 and got.max() <= n and got32.min() >= 0 and got32.max() <= n, name
            assert o_flag.get(name + ".flag").tolist() == [bad] and o_flag32.get(name + ".flag32").tolist() == [5 + bad], name
            assert np.array_equal(o_ids32.get(name + ".ids32"), clamped), name


def test_edge_segments_with_empty_graphs(dev):
    from dp_gsat_amd.graph_index import BatchIndex
    ei, batch, G, N = io.edge_segments_case()
    eptr, order, eg = io.edge_segments(ei, batch, G)
    for rep in range(2):
        seg = BatchIndex(_dev_i64(ei, dev), N).graphs(_dev_i64(batch, dev), G)
        got_ptr, got_order, got_eg, got_eg32 = seg.edge_segments
        _sync()
        assert np.array_equal(got_ptr.cpu().numpy(), eptr) and np.array_equal(got_order.cpu().numpy(), order)
        assert np.array_equal(got_eg.cpu().numpy(), eg) and np.array_equal(got_eg32.cpu().numpy(), eg)
        assert np.array_equal(seg.node_ptr.cpu().numpy(), io.segments(batch, G)[0]) and np.array_equal(seg.node_seg32.cpu().numpy(), batch)
        assert eptr[1] == 0 and eptr[4] == eptr[5] and eptr[G - 1] == eptr[G] == ei.shape[1]          # first, a middle and the last graph empty
        seg.check()


# ---- line graphs ----------------------------------------------------------------------------------------------------------------------------
def test_line_graph_by_source_with_a_hub_and_pairless_nodes(dev):
    """k_line_graph's search over the triangle prefix at out-degree 300, and its search over the pair pointers past nodes of degree 0
    and 1 at the front, at the end and between two rows with pairs."""
    import dp_gsat_amd as G
    ei, N, batch = io.dual_by_source_case()
    want = obk.line_graph_by_source(ei)
    deg = np.bincount(ei[0], minlength=N)
    assert want.shape == (2, int((deg * (deg - 1)).sum()))
    for rep in range(2):
        dei, dbatch = G.line_graph(_dev_i64(ei, dev), N, _dev_i64(batch, dev))
        _sync()
        got = dei.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero((got != want).any(axis=0))[:8].tolist()
        assert np.array_equal(dbatch.cpu().numpy(), batch[ei[0]])


def test_undirected_line_graph_with_a_star(dev):
    """k_lg_counts / k_lg_fill merge the rows of a 300-leaf star with duplicated edges in them; a triangle in a second graph.  The self
    loop is no dual node and changes nothing else (rule: compared with the oracle on the list without it, whose loops would index
    dual_dense[-1] through a loop)."""
    import dp_gsat_amd as G
    eu, N, batch, eu_no_loop = io.dual_undirected_case()
    want_ei, want_und, want_batch, _, _ = obk.line_graph_undirected(eu_no_loop, batch, None)
    assert want_und.shape[1] == 305 and want_ei.shape[1] == 300 * 299 + 12          # the star's edges all meet; six adjacencies in graph 1
    for ei in (eu, eu_no_loop):
        got = G.line_graph_undirected(_dev_i64(ei, dev), N, _dev_i64(batch, dev))
        _sync()
        assert np.array_equal(got.edge_index.cpu().numpy(), want_ei)
        assert np.array_equal(got.und_index.cpu().numpy(), want_und)
        assert np.array_equal(got.batch.cpu().numpy(), want_batch)
        assert np.array_equal(got.und_of_edge.cpu().numpy(), io.und_of_edge(ei, want_und))
        assert got.num_dual_nodes == 305
    assert io.und_of_edge(eu, want_und)[-1] == -1 and (io.und_of_edge(eu, want_und)[:-1] >= 0).all()
