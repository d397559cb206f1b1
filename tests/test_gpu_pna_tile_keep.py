"""-m gpu: the tiled PNA backward keeps its bits at every window size at which its dx path takes another turn.

k_pna_bwd_tile keeps the dx_self rows of a lane group's last K rows in registers, stores the earlier ones to dx, and requests what the
per-source pass reads (the stored dx rows, dx_add, d node_att) for the group's first five rows ahead of the window's barrier.  Which of
these a row takes depends on the window's row count relative to the lane groups per workgroup (g) and to K, so the windows here are
built to hold exactly {1, g-1, g, g+1, K*g-1, K*g, K*g+1, (K+1)*g, (K+1)*g+1, rows_cap} rows (those within [1, rows_cap]) at H = 128
(g 16), 80 (g 24, five aggregators; K = 2 with node attention, 3 with edge attention: both sets), 64 (g 32) and 256 (g 8), out of small
ring and path graphs; the test reads the window descriptors back and asserts the set is covered.  Two more cases run the H = 128
graphs at other LDS budgets: 12 KiB (8-row windows, most sources spill) and 128 KiB (120-row windows: lane groups with more than five
rows, whose later rows load inside the per-source loop; no smaller budget than the default can reach that arm).

tests/golden/pna_tile_keep_bits.npz holds SHA-256 digests of dx and datt / d node_att (and of the inputs) written by the build BEFORE
that change (one kept row, loads behind the barrier).  Every operation and its order per channel are unchanged, so the comparison is a
byte comparison.  The record is never regenerated from the kernel under test; `python -m tests.test_gpu_pna_tile_keep OUT.npz` exists
to write it from a build whose results are the agreed ones."""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pna_tile_keep_bits.npz")
AGG4, AGG5 = (1, 2, 3, 5), (1, 2, 3, 5, 0)            # (mean,min,max,std[,sum]): ops.AGGREGATOR_CODES
MODES = [("edge", 0), ("node", 0), ("node", 1)]        # (attention kind, accumulate into an existing d node_att)
PREFETCH = 5                                          # rows per lane group requested ahead of the barrier (TILE_PREFETCH)
DEFAULT_LDS = 80 * 1024

# name -> (H, GSAT_PNA_TILE_LDS, the budget the graphs were planned for)
CASES = {
    "H128": (128, 0, 0),
    "H80": (80, 0, 0),
    "H64": (64, 0, 0),
    "H256": (256, 0, 0),
    "H128-lds12k": (128, 12288, 0),              # the H128 graphs under 8-row windows: sources outside their window
    "H128-lds128k": (128, 131072, 131072),       # lane groups of up to 8 rows
}


def _lpr(H):
    q = H // 4
    return 4 if q <= 4 else 8 if q <= 8 else 16 if q <= 16 else 20 if q <= 20 else 32 if q <= 32 else 64


def _groups(H):
    """g: lane groups (rows in flight) of a 512-thread workgroup."""
    return 8 * (64 // _lpr(H))


def _keeps(H):
    """K of the instantiations this width runs (pna_tile_keep): 2 for <20,5,node attention>, else 3."""
    return (2, 3) if H == 80 else (3,)


def _plan(H, budget):
    """(rows_nominal, rows_cap) of gsat_pna_tile_plan."""
    te = ((budget or DEFAULT_LDS) - 64) // (_lpr(H) * 16 + 24) // 8 * 8
    half = max(4, te // 4 // 4 * 4)
    return half, 2 * half


def _wanted(H, budget):
    g, (n, cap) = _groups(H), _plan(H, budget)
    want = {1, g - 1, g, g + 1, cap}
    for K in _keeps(H):
        want |= {K * g - 1, K * g, K * g + 1, (K + 1) * g, (K + 1) * g + 1}
    if budget > DEFAULT_LDS:
        want |= {PREFETCH * g, PREFETCH * g + 1}
    return sorted(w for w in want if 1 <= w <= cap)


def _window_rows(sizes, n):
    """Row counts of the windows of k_pna_tiles (nominal n, slack n) over graphs of the given sizes: window t starts at
    min(p, max(start of the graph that holds row p, p - slack)), p = t * n."""
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N = int(ptr[-1])
    T = -(-N // n)
    p = np.arange(T) * n
    g0 = ptr[np.searchsorted(ptr, p, side="right") - 1]
    start = np.concatenate([np.minimum(p, np.maximum(g0, p - n)), [N]])
    return np.diff(start)


def _graph_sizes(n, targets):
    """Graph sizes whose windows hold the target row counts, with filler windows between where the offsets do not chain.
    With window t starting a rows before t * n, a window of w rows (a < w <= n + a) is one graph of a + 1 nodes that reaches row t * n
    and small graphs behind it; the next window then starts n + a - w rows early.  A full window (2 n rows) is one graph of 2 n nodes
    that starts on a multiple of n: the window in front of it is empty."""
    fill = [3, 5, 1, 4, 2, 6, 7]
    sizes, a, f = [], 0, 0

    def window(w):
        nonlocal a, f
        assert a < w <= n + a
        sizes.append(a + 1)
        left = w - a - 1
        while left:
            s = min(left, fill[f % len(fill)])
            f += 1
            sizes.append(s)
            left -= s
        a = n + a - w

    for w in targets:
        if w == 2 * n:
            if a:
                window(n + a)
            sizes.append(2 * n)
        else:
            if not a < w <= n + a:
                window(n + a - max(0, w - n))
            window(w)
    return sizes


@functools.lru_cache(maxsize=None)
def _graph(H, budget):
    """(edge_index, batch, N, graph sizes): rings, two-way paths and one-way paths (a first node without in-edges, a last node without
    out-edges) in turn; single nodes are isolated."""
    n, _ = _plan(H, budget)
    sizes = _graph_sizes(n, _wanted(H, budget))
    assert set(_wanted(H, budget)) <= set(_window_rows(sizes, n).tolist())
    src, dst, batch, base = [], [], [], 0
    for gi, s in enumerate(sizes):
        i = np.arange(s - 1) + base
        kind = gi % 3
        if s > 1:
            src.append(i); dst.append(i + 1)
            if kind != 2:
                src.append(i + 1); dst.append(i)
            if kind == 0 and s > 2:
                src.append(np.array([base + s - 1, base])); dst.append(np.array([base, base + s - 1]))
        batch.append(np.full(s, gi))
        base += s
    ei = torch.from_numpy(np.stack([np.concatenate(src), np.concatenate(dst)])).long()
    ei = ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(7))].contiguous()
    return ei, torch.from_numpy(np.concatenate(batch)).long(), base, tuple(sizes)


@functools.lru_cache(maxsize=None)
def _inputs(H, planned):
    ei, batch, N, _ = _graph(H, planned)
    E = ei.shape[1]
    nagg = 5 if H == 80 else 4
    g = torch.Generator().manual_seed(3000 * H + planned)
    x = torch.randn(N, H, generator=g)
    x[::5] = x[::5].relu()                               # exact zeros: the sign selects of the self part
    att = torch.rand(E, generator=g)
    na = torch.rand(N, generator=g)
    na[::7] = 0.0                                        # zero attention: ties in the first-occurrence args
    go = torch.randn(N, nagg * 2 * H, generator=g)
    dx_add = torch.randn(N, H, generator=g)
    dna0 = torch.randn(N, generator=g)
    return dict(ei=ei, batch=batch, N=N, E=E, nagg=nagg, x=x, att=att, na=na, go=go, dx_add=dx_add, dna0=dna0)


def _digest(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def _run(dev, name):
    """Every (mode, dx_add) combination of one case -> {key: digest}; asserts that the windows cover the wanted row counts.
    GSAT_PNA_TILE_LDS must be set to the case's budget by the caller."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.graph_index import BatchIndex
    H, budget, planned = CASES[name]
    inp = _inputs(H, planned)
    N, E, nagg = inp["N"], inp["E"], inp["nagg"]
    out = {f"{name}/inputs": _digest(torch.cat([inp[k].reshape(-1).float() for k in ("ei", "x", "att", "na", "go", "dx_add", "dna0")]))}
    ix = BatchIndex(inp["ei"].to(dev), N)
    ix.graphs(inp["batch"].to(dev))                     # graph-aligned windows, as in a training step
    tiles = ix.pna_tiles(H)
    assert tiles, f"the tiled backward must cover H={H}"
    tile_ptr, T, rows_nominal, rows_cap, edges_cap, spill = tiles
    assert (rows_nominal, rows_cap) == _plan(H, budget), "the windows are not the ones the graphs were sized for"
    torch.cuda.synchronize()
    starts = tile_ptr[:, 0].cpu().numpy()
    rows = np.diff(starts)
    assert starts[0] == 0 and starts[-1] == N and rows.min() >= 0 and rows.max() <= rows_cap
    g = _groups(H)
    if budget == planned:
        missing = set(_wanted(H, budget)) - set(rows.tolist())
        assert not missing, f"{name}: no window of {sorted(missing)} rows (g={g}, K={_keeps(H)}, cap={rows_cap})"
        assert rows.min() < g, "a lane group that owns no row"
    if budget > DEFAULT_LDS:
        assert rows.max() > PREFETCH * g, "lane groups with more rows than are requested ahead of the barrier"
    x, att, na, go, dx_add = (inp[k].to(dev) for k in ("x", "att", "na", "go", "dx_add"))
    a_arr = (ctypes.c_int32 * nagg)(*(AGG5 if nagg == 5 else AGG4))
    s_arr = (ctypes.c_int32 * 1)(0)
    for mode, acc in MODES:
        for add in (0, 1):
            dx = torch.full((N, H), float("nan"), device=dev)
            dmsg = torch.full((max(E, 1), H), float("nan"), device=dev)
            if mode == "edge":
                datt = torch.full((E,), float("nan"), device=dev)
                call("gsat_pna_bwd_tiled", ptr(x), ptr(att), ptr(go), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst),
                     ptr(tile_ptr), T, rows_nominal, rows_cap, edges_cap, ptr(ix.rowptr_src), ptr(ix.slot_dst_of_srcslot), N, E, H,
                     a_arr, nagg, s_arr, 1, ptr(spill[1:]), ptr(spill[:1]), ptr(dx), ptr(dmsg), ptr(datt), ptr(dx_add) if add else None,
                     stream())
            else:
                datt = inp["dna0"].to(dev) if acc else torch.full((N,), float("nan"), device=dev)
                dw = torch.full((max(E, 1),), float("nan"), device=dev)
                call("gsat_pna_bwd_tiled_node_att", ptr(x), ptr(na), ptr(go), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(tile_ptr), T,
                     rows_nominal, rows_cap, edges_cap, ptr(ix.rowptr_src), ptr(ix.slot_dst_of_srcslot), N, E, H, a_arr, nagg, s_arr, 1,
                     ptr(spill[1:]), ptr(spill[:1]), ptr(dx), ptr(dmsg), ptr(datt), ptr(dw), ptr(dx_add) if add else None, acc, stream())
            torch.cuda.synchronize()
            assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(datt).all()), "an output element was not written"
            key = f"{name}-{mode}-add{add}-acc{acc}"
            out[key + "/dx"] = _digest(dx)
            out[key + "/datt"] = _digest(datt)
    count = int(spill[0])
    assert 0 <= count <= N, f"spill list overflowed: {count} > {N}"
    deg_in = (ix.rowptr_dst[1:] - ix.rowptr_dst[:-1])
    deg_out = (ix.rowptr_src[1:] - ix.rowptr_src[:-1])
    assert int(deg_in.min()) == 0 and int(deg_out.min()) == 0, "rows without in-edges and nodes without out-edges"
    if 0 < budget < DEFAULT_LDS:
        assert count > 0, "the small-LDS case is meant to have sources outside their window"
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_tiled_backward_keeps_its_bits_at_every_window_size(dev, monkeypatch, name):
    """dx and datt / d node_att, byte for byte against the record, over windows of every row count at which a row changes between
    registers, the prefetched reload and the in-loop reload: edge and node attention, with and without dx_add, with and without
    accumulation into an existing d node_att."""
    monkeypatch.setenv("GSAT_PNA_TILE_LDS", str(CASES[name][1]))
    monkeypatch.setattr("dp_gsat_amd.graph_index._HUBS_SEEN", [False])
    want = np.load(GOLDEN)
    got = _run(dev, name)
    key = f"{name}/inputs"
    assert bytes(got[key]) == bytes(want[key]), "the seeded inputs differ from the recorded ones: the comparison would mean nothing"
    bad = [k for k in sorted(got) if bytes(got[k]) != bytes(want[k])]
    print(f"{name}: {len(got) - len(bad)}/{len(got)} arrays byte-equal to the record")
    assert not bad, f"not byte-equal to the record: {bad}"


if __name__ == "__main__":
    import sys
    assert torch.cuda.is_available()
    rec = {}
    for name_ in CASES:
        os.environ["GSAT_PNA_TILE_LDS"] = str(CASES[name_][1])
        rec.update(_run(torch.device("cuda:0"), name_))
    np.savez(sys.argv[1], **rec)
    print(f"wrote {len(rec)} digests to {sys.argv[1]}")
