"""-m gpu: the tiled PNA backward (gsat_pna_bwd_tiled / gsat_pna_bwd_tiled_node_att) reproduces recorded results BIT FOR BIT.

tests/golden/pna_tile_bits.npz holds SHA-256 digests of dx and datt / d node_att (and of the inputs) that the tiled backward produced
on an MI355X BEFORE its edge loops, addressing and dx path were reworked for speed.  Rewrites of that kernel must keep every
operation and its order per channel (an fma stays an fma, a separate multiply and add stay separate, the per-source sums run in
by-source slot order), so the comparison is a byte comparison, not a tolerance.  The record is never regenerated from the kernel under
test; `python -m tests.test_gpu_pna_tile_bits OUT.npz` exists to write it from a build whose results are the agreed ones."""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

from tests.graphs import random_batch, shuffle_edges

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pna_tile_bits.npz")
AGG4, AGG5 = (1, 2, 3, 5), (1, 2, 3, 5, 0)            # (mean,min,max,std[,sum]): ops.AGGREGATOR_CODES
SMALL_LDS = 12288                                     # 16-40 edge slots per window: most edges spill, the hub row overflows the capacity

SHAPES = ["c3", "small"]
WIDTHS = [64, 80, 128]
MODES = [("edge", 0), ("node", 0), ("node", 1)]        # (attention kind, accumulate into an existing d node_att)


@functools.lru_cache(maxsize=None)
def _graph(shape):
    """(edge_index, batch, N).  c3: the molhiv-shaped batch of the flagship workload (2048 graphs) with the in-edges of every 97th node
    removed (rows without in-edges).  small: molecule-like graphs with isolated nodes and a 199-edge star (a hub row)."""
    if shape == "c3":
        from dp_gsat_amd import synth
        b = synth.molhiv_batch(2048, 0)
        ei = b.edge_index[:, b.edge_index[1] % 97 != 0].contiguous()
        return ei, b.batch, b.num_nodes
    ei, batch, N = random_batch(23, 24, 1, 40)
    hub = torch.arange(1, 200)
    star = torch.stack([torch.cat([hub, torch.zeros_like(hub)]), torch.cat([torch.zeros_like(hub), hub])]) + (N - 200 if N > 400 else 0)
    return shuffle_edges(torch.cat([ei, star.clamp_(max=N - 1)], dim=1), 2), batch, N


def _inputs(shape, H):
    ei, batch, N = _graph(shape)
    E = ei.shape[1]
    nagg = 5 if H == 80 else 4
    g = torch.Generator().manual_seed(1000 * H + len(shape))
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


def _run(dev, shape, H):
    """Every (mode, dx_add) combination of one shape and width -> {key: digest}; asserts the spill list did not overflow."""
    from dp_gsat_amd._lib import call, ptr, stream
    from dp_gsat_amd.graph_index import BatchIndex
    inp = _inputs(shape, H)
    N, E, nagg = inp["N"], inp["E"], inp["nagg"]
    out = {f"{shape}-H{H}/inputs": _digest(torch.cat([inp[k].reshape(-1).float() for k in ("ei", "x", "att", "na", "go", "dx_add", "dna0")]))}
    ix = BatchIndex(inp["ei"].to(dev), N)
    ix.graphs(inp["batch"].to(dev))                     # graph-aligned windows, as in a training step
    tiles = ix.pna_tiles(H)
    assert tiles, f"the tiled backward must cover H={H}"
    tile_ptr, T, rows_nominal, rows_cap, edges_cap, spill = tiles
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
            key = f"{shape}-H{H}-{mode}-add{add}-acc{acc}"
            out[key + "/dx"] = _digest(dx)
            out[key + "/datt"] = _digest(datt)
    count = int(spill[0])
    # the counter doubles as the overflow record: k_pna_spill_rows keeps counting past the list's capacity, so a value above N would mean
    # dropped spill rows, i.e. a silently wrong dx
    assert 0 <= count <= N, f"spill list overflowed: {count} > {N}"
    if shape == "small":
        assert count > 0, "the small shape is meant to have sources outside their window"
        deg = (ix.rowptr_dst[1:] - ix.rowptr_dst[:-1])
        assert int(deg.max()) > edges_cap and int(deg.min()) == 0, "the small shape is meant to have a hub row and rows without in-edges"
    else:
        deg = (ix.rowptr_dst[1:] - ix.rowptr_dst[:-1])
        assert int(deg.min()) == 0, "the c3 shape is meant to have rows without in-edges"
    return out


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_tiled_backward_matches_the_recorded_bits(dev, monkeypatch, shape, H):
    """dx and datt / d node_att of the tiled backward, byte for byte against the record: edge and node attention, with and without
    dx_add, with and without accumulation into an existing d node_att; the flagship shape and tiny windows with a hub row; empty rows;
    spilled sources.  The spill counter stays within the list."""
    monkeypatch.setenv("GSAT_PNA_TILE_LDS", str(SMALL_LDS if shape == "small" else 0))
    monkeypatch.setattr("dp_gsat_amd.graph_index._HUBS_SEEN", [False])
    want = np.load(GOLDEN)
    got = _run(dev, shape, H)
    key = f"{shape}-H{H}/inputs"
    assert bytes(got[key]) == bytes(want[key]), "the seeded inputs differ from the recorded ones: the comparison would mean nothing"
    bad = [k for k in sorted(got) if bytes(got[k]) != bytes(want[k])]
    print(f"{shape} H={H}: {len(got) - len(bad)}/{len(got)} arrays byte-equal to the record")
    assert not bad, f"not byte-equal to the record: {bad}"


if __name__ == "__main__":
    import sys
    assert torch.cuda.is_available()
    rec = {}
    for shape_ in SHAPES:
        os.environ["GSAT_PNA_TILE_LDS"] = str(SMALL_LDS if shape_ == "small" else 0)
        for H_ in WIDTHS:
            rec.update(_run(torch.device("cuda:0"), shape_, H_))
    np.savez(sys.argv[1], **rec)
    print(f"wrote {len(rec)} digests to {sys.argv[1]}")
