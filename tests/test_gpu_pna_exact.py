"""-m gpu: every kernel of csrc/pna.hip through the C ABI against the plain fp64 reference of tests/pna_oracle.py, on graphs whose row
lengths, ties and window sizes are fixed where the kernels branch.

Two recipes per case.  On the exact recipe (pna_oracle: dyadic-grid values drawn from a few distinct rows, ties everywhere, std dormant)
every fp32 evaluation in any order is the exact result (tests/test_pna_oracle_host.py), so sum, min, max, the mean of power-of-two rows,
dx, datt / d node_att and dedge must be torch.equal to the fp64 reference cast to fp32: a gradient routed to another slot among tied ones
moves a value by a grid step and cannot hide next to a large entry.  The mean of the other rows (the kernel multiplies by 1/n) and std
go through ``close`` with the default TOL.  On the float recipe (randn / rand, full dout, std / var / scalers live) the comparison is the
one of tests/test_gpu_pna.py, unchanged.

The entry points are called directly, as tests/test_gpu_pna_tile_keep.py does, so the test chooses the path; buffers are sized as
dp_gsat_amd/ops.py sizes them, every output is filled with NaN first and must be written in full.

  A  row lengths 0,1,2,3,4,5,7,8,9,16,17 x 14 widths (all six LPRs, partial lane groups, a second channel chunk) x the NAGG 4 / 5 /
     generic staged / generic unstaged instantiations x no / edge attention (x an edge embedding on a subset of widths)
  B  the x_i part: sign patterns > 0, < 0, +0, -0 and an attention whose extremes are attained twice per row (two-pass and tiled)
  C  hub rows of 256 (not long), 257, 512, 513, 1025 in-edges through the *_long entry points, ties across chunks; E = 256
  D  the node-attention forward
  E  the tiled backward on the window-size graphs of test_gpu_pna_tile_keep.py, float (the recorded arrays) and exact
  F  the tiled backward at LPR 4 and 8, partial lane groups, a star row that crosses the LDS edge capacity, spilled sources

Instantiations and the cases that launch them.  LPR by width: 4: 4, 12, 16; 8: 32; 16: 48, 64; 20: 72, 80; 32: 100, 128; 64: 132, 256;
above 256 channels a second launch takes H - 256 (260: LPR 4, 336: LPR 20, 512: LPR 64).
  k_pna_fwd, k_pna_bwd_dst <LPR, HAS_EE, NAGG, LONG = false>   A: six LPRs x NAGG 0 / 4 / 5, HAS_EE at widths 4, 32, 64, 80, 100, 132, 260, 336;
                                                               the node-attention arm of k_pna_fwd (eid == NULL): D, six LPRs
  k_pna_fwd, k_pna_bwd_dst <LPR, HAS_EE, NAGG, LONG = true>,   C: widths 16, 32, 64, 80, 100, 256 (+ 336) = six LPRs x both HAS_EE x NAGG 0 / 4 / 5
  k_pna_chunk_stats, k_pna_chunk_apply <LPR, HAS_EE>
  k_pna_bwd_tile <LPR, NAGG 4 | 5, NATT>                       F: widths 8, 32, 48, 72, 100, 132 = six LPRs x both NAGG x both NATT; E: <16, 4>, <20, 5>,
                                                               <32, 4>, <64, 4> x both NATT at every window size; B: <4, *, false>, <20, *, false>
  k_pna_bwd_spill <LPR>                                        F at the smallest budget: six LPRs; E: H128-lds12k
The compact forward (scal_out) and gsat_pna_post_* are opt-in, live in gemm.hip and are left to tests/test_gpu_pna.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import pna_oracle as po
from tests.test_gpu_pna import close_weighted, std_conditioning
from tests.test_gpu_pna_tile_keep import CASES, MODES, _graph, _inputs, _plan
from tests.util import close

pytestmark = pytest.mark.gpu

AVG = {"lin": 2.5, "log": 1.25}
NAN = float("nan")
WIDTHS_A = (4, 12, 16, 32, 64, 72, 80, 100, 128, 132, 256, 260, 336, 512)
WIDTHS_EE = (4, 32, 64, 80, 100, 132, 260, 336)                  # one per LPR, a second chunk at LPR 4 and at LPR 20
LISTS = {"nagg4": (po.AGG4, ["identity"]), "nagg5": (po.AGG5, ["identity"]), "staged": (po.AGG_STAGED, ["identity"]),
         "unstaged": (po.AGG_ALL, po.SCALERS3)}                  # unstaged: 18 x parts segments > 8, float recipe only


@pytest.fixture(autouse=True)
def _no_hubs_seen(monkeypatch):
    monkeypatch.setattr("dp_gsat_amd.graph_index._HUBS_SEEN", [False])


def _codes(aggr, scalers):
    a = (ctypes.c_int32 * len(aggr))(*(po.AGG_CODES[k] for k in aggr))
    s = (ctypes.c_int32 * len(scalers))(*(po.SCALER_CODES[k] for k in scalers))
    return a, len(aggr), s, len(scalers)


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _written(what, **tensors):
    for name, t in tensors.items():
        if t is not None:
            assert bool(torch.isfinite(t).all()), f"{what}: {int((~torch.isfinite(t)).sum())} elements of {name} were not written"


def _index(dev, ei, N):
    from dp_gsat_amd.graph_index import BatchIndex
    return BatchIndex(ei.to(dev), N)


def _two_pass(dev, ix, H, x, att, emb, aggr, scalers, dout, long, what):
    """Forward and two-pass backward (gsat_pna_bwd[_long] + gsat_aggr_sum_fwd, as PnaAggregate.backward) -> (out, dx, datt, dedge)."""
    from dp_gsat_amd._lib import call, ptr, stream
    N, E = ix.N, ix.E
    a, A, s, S = _codes(aggr, scalers)
    parts = 3 if emb is not None else 2
    x, dout = x.to(dev), dout.to(dev).contiguous()
    att = None if att is None else att.to(dev)
    emb = None if emb is None else emb.to(dev)
    out = _nan(dev, N, S * A * parts * H)
    dx_self, dx, dmsg = _nan(dev, N, H), _nan(dev, N, H), _nan(dev, max(E, 1), H)
    datt = None if att is None else _nan(dev, E)
    dee = None if emb is None else _nan(dev, E, H)
    if long:
        part = ix.pna_partial(H, emb is not None)
        call("gsat_pna_fwd_long", ptr(x), ptr(att), ptr(emb), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst), N, E, H, a, A, s, S,
             AVG["lin"], AVG["log"], ptr(out), ptr(ix.chunk_ptr_dst), ptr(part), stream())
        call("gsat_pna_bwd_long", ptr(x), ptr(att), ptr(emb), ptr(dout), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst), N, E, H,
             a, A, s, S, AVG["lin"], AVG["log"], ptr(dx_self), ptr(dmsg), ptr(datt), ptr(dee), ptr(ix.chunk_ptr_dst), ptr(part), stream())
    else:
        call("gsat_pna_fwd", ptr(x), ptr(att), ptr(emb), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst), N, H, a, A, s, S,
             AVG["lin"], AVG["log"], ptr(out), stream())
        call("gsat_pna_bwd", ptr(x), ptr(att), ptr(emb), ptr(dout), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst), N, H,
             a, A, s, S, AVG["lin"], AVG["log"], ptr(dx_self), ptr(dmsg), ptr(datt), ptr(dee), stream())
    hubs_src = ix.long_rows[1]
    call("gsat_aggr_sum_fwd", ptr(dmsg), ptr(dx_self), None, None, ptr(ix.rowptr_src), ptr(ix.slot_dst_of_srcslot), None, N, E, H, 1.0,
         ptr(dx), ptr(hubs_src), ptr(ix.partial(H)) if hubs_src is not None else None, stream())
    torch.cuda.synchronize()
    _written(what, out=out, dx_self=dx_self, dmsg=dmsg[:E], dx=dx, datt=datt, dedge=dee)
    return out, dx, datt, dee


def _build_tiles(ix, H, budget, seg=None):
    """BatchIndex.pna_tiles for any width (it declines H < 64, where ops prefers the two-pass backward) at an explicit LDS budget."""
    from dp_gsat_amd import _lib
    from dp_gsat_amd._lib import call, ptr, stream
    nominal, slack, ecap = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    rc = _lib.load().gsat_pna_tile_plan(int(H), int(budget), ctypes.byref(nominal), ctypes.byref(slack), ctypes.byref(ecap))
    assert rc == 0, f"gsat_pna_tile_plan declined H={H} at {budget} bytes"
    T = (ix.N + nominal.value - 1) // nominal.value
    tile_ptr = torch.empty(T + 1, 4, dtype=torch.int32, device=ix.device)
    spill = torch.empty(ix.N + 1, dtype=torch.int32, device=ix.device)
    call("gsat_pna_build_tiles", ptr(seg.node_ptr) if seg is not None else None, ptr(seg.node_seg32) if seg is not None else None,
         ptr(ix.rowptr_dst), ptr(ix.rowptr_src), ptr(ix.slot_dst_of_srcslot) if ix.E else None, ix.N, nominal.value, slack.value, ecap.value,
         ptr(tile_ptr), ptr(spill[1:]), ptr(spill[:1]), stream())
    return tile_ptr, T, nominal.value, nominal.value + slack.value, ecap.value, spill


def _tiled(dev, ix, tiles, H, x, w, aggr, dout, mode, what, dx_add=None, dna0=None):
    """gsat_pna_bwd_tiled (mode "edge": w = att [E]) or gsat_pna_bwd_tiled_node_att (w = na [N]; dna0: accumulate into it) -> (dx, datt)."""
    from dp_gsat_amd._lib import call, ptr, stream
    N, E = ix.N, ix.E
    tile_ptr, T, rows_nominal, rows_cap, edges_cap, spill = tiles
    a, A, s, S = _codes(aggr, ["identity"])
    x, w, dout = x.to(dev), w.to(dev), dout.to(dev).contiguous()
    add = None if dx_add is None else dx_add.to(dev)
    dx, dmsg = _nan(dev, N, H), _nan(dev, max(E, 1), H)
    if mode == "edge":
        datt = _nan(dev, E)
        call("gsat_pna_bwd_tiled", ptr(x), ptr(w), ptr(dout), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(ix.eid_by_dst), ptr(tile_ptr), T,
             rows_nominal, rows_cap, edges_cap, ptr(ix.rowptr_src), ptr(ix.slot_dst_of_srcslot), N, E, H, a, A, s, S, ptr(spill[1:]),
             ptr(spill[:1]), ptr(dx), ptr(dmsg), ptr(datt), ptr(add), stream())
    else:
        datt = dna0.to(dev).clone() if dna0 is not None else _nan(dev, N)
        dw = _nan(dev, max(E, 1))
        call("gsat_pna_bwd_tiled_node_att", ptr(x), ptr(w), ptr(dout), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), ptr(tile_ptr), T, rows_nominal,
             rows_cap, edges_cap, ptr(ix.rowptr_src), ptr(ix.slot_dst_of_srcslot), N, E, H, a, A, s, S, ptr(spill[1:]), ptr(spill[:1]),
             ptr(dx), ptr(dmsg), ptr(datt), ptr(dw), ptr(add), 1 if dna0 is not None else 0, stream())
    torch.cuda.synchronize()
    _written(what, dx=dx, datt=datt)
    count = int(spill[0])
    assert 0 <= count <= N, f"{what}: spill list overflowed: {count} > {N}"
    return dx, datt


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _equal(what, got, ref64):
    """Bit comparison (as values: -0.0 == +0.0) with the fp64 reference cast to fp32."""
    got, want = got.detach().cpu(), _t(ref64).float().view(got.shape)
    bad = got != want
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} entries differ from the fp64 reference, first at "
                                 f"{tuple(bad.nonzero()[0].tolist())}: {got[bad][0].item()!r} != {want[bad][0].item()!r}")


def _check_out_exact(what, out, ref, aggr, F, pow2):
    out = out.detach().cpu()
    r = _t(ref.out)
    for ai, a in enumerate(aggr):
        seg = slice(ai * F, (ai + 1) * F)
        if a in ("sum", "min", "max"):
            _equal(f"{what} out[{a}]", out[:, seg], r[:, seg].numpy())
        elif a == "mean":
            _equal(f"{what} out[mean], power-of-two rows", out[pow2][:, seg], r[pow2][:, seg].numpy())
            close(out[~pow2][:, seg], r[~pow2][:, seg], what=f"{what} out[mean], other rows")
        else:
            close(out[:, seg], r[:, seg], what=f"{what} out[{a}]")


def _check_exact(what, got, ref, aggr, F, pow2):
    out, dx, datt, dee = got
    if out is not None:
        _check_out_exact(what, out, ref, aggr, F, pow2)
    _equal(f"{what} dx", dx, ref.dx)
    if datt is not None:
        _equal(f"{what} datt", datt, ref.datt if ref.datt is not None else ref.dna)
    if dee is not None:
        _equal(f"{what} dedge", dee, ref.dedge)


def _check_float(what, got, r32, r64, x, ei, N, w_edge):
    """The comparison of tests/test_gpu_pna.py: conditioning-weighted dx / datt without an edge embedding (test_pna_fwd_bwd), plain
    ``close`` with one (test_pna_with_edge_attr); w_edge: the [E] edge weights or None."""
    out, dx, datt, dee = got
    if out is not None:
        close(out, _t(r32.out), ref64=_t(r64.out), what=f"{what} out")
    if dee is not None:
        close(dx, _t(r32.dx), ref64=_t(r64.dx), what=f"{what} dx")
        close(dee, _t(r32.dedge), ref64=_t(r64.dedge), what=f"{what} dedge")
        if datt is not None:
            close(datt, _t(r32.datt), ref64=_t(r64.datt), what=f"{what} datt")
        return
    w_dx, w_e = std_conditioning(x, ei, None if w_edge is None else w_edge.view(-1, 1), N)
    close_weighted(dx, _t(r32.dx), _t(r64.dx), w_dx, f"{what} dx")
    if datt is not None:
        close_weighted(datt, _t(r32.datt), _t(r64.datt), w_e, f"{what} datt")


def _refs(x, ei, aggr, scalers, dout, att=None, na=None, emb=None, both=False):
    kw = dict(att=att, node_att=na, edge_emb=emb, dout=dout)
    r64 = po.pna_reference(x, ei, aggr, scalers, AVG, dtype=np.float64, **kw)
    return (po.pna_reference(x, ei, aggr, scalers, AVG, dtype=np.float32, **kw), r64) if both else r64


def _two_pass_case(dev, ei, N, H, which, modes, embs, seed, long, tag, exact_inputs=None):
    aggr, scalers = LISTS[which]
    ix = _index(dev, ei, N)
    for ee in embs:
        parts = 3 if ee else 2
        F = parts * H
        for mode in modes:
            what = f"{tag} H={H} {which} {mode} ee={int(ee)}"
            if which != "unstaged":
                inp = exact_inputs(ee) if exact_inputs is not None else po.exact_inputs(ei, N, H, seed, edge_emb=ee)
                dout, pow2 = po.exact_dout(ei, N, H, aggr, scalers, parts, seed + 1)
                att = inp.att if mode == "edge" else None
                got = _two_pass(dev, ix, H, inp.x, att, inp.emb, aggr, scalers, dout, long, what + " exact")
                _check_exact(what + " exact", got, _refs(inp.x, ei, aggr, scalers, dout, att=att, emb=inp.emb), aggr, F, pow2)
            inp = po.float_inputs(ei, N, H, seed + 2, edge_emb=ee)
            dout = po.float_dout(N, H, aggr, scalers, parts, seed + 3)
            att = inp.att if mode == "edge" else None
            got = _two_pass(dev, ix, H, inp.x, att, inp.emb, aggr, scalers, dout, long, what + " float")
            r32, r64 = _refs(inp.x, ei, aggr, scalers, dout, att=att, emb=inp.emb, both=True)
            _check_float(what + " float", got, r32, r64, inp.x, ei, N, att)


# ---- A: row lengths, two-pass kernels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(LISTS))
@pytest.mark.parametrize("H", WIDTHS_A)
def test_two_pass_kernels_at_every_row_length(dev, H, which):
    """k_pna_fwd / k_pna_bwd_dst<LPR, HAS_EE, NAGG, false> on rows of 0 .. 17 in-edges: the empty row, the rows of 1-4 that reuse pass 1's
    indices, the batch-of-4 tails at 5, 8, 9, 16, 17; duplicate edges and a self-loop.  Above 256 channels datt is summed over two launches."""
    ei, N = po.row_length_graph()
    _two_pass_case(dev, ei, N, H, which, ("none", "edge"), (False, True) if H in WIDTHS_EE else (False,), 1000 + H, False, "A")


# ---- B: the x_i part ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["nagg4", "nagg5"])
@pytest.mark.parametrize("H", [16, 80])
def test_self_part_signs_and_attention_ties(dev, H, which):
    """x_i > 0, < 0, +0 and -0 per channel and an attention whose minimum and maximum are each attained twice per row: the closed-form
    x_i part routes min / max to the first slot of the att extreme its sign selects (kmin_a / kmax_a) and to the row's first slot where
    x_i is a zero (wfirst); dx holds the dx_self term and datt the tmn / tmx terms.  Two-pass and tiled kernels."""
    ei, N = po.row_length_graph()
    aggr, scalers = LISTS[which]
    inp = po.self_part_inputs(ei, N, H, 2000 + H)
    dout, pow2 = po.exact_dout(ei, N, H, aggr, scalers, 2, 2001 + H)
    ref = _refs(inp.x, ei, aggr, scalers, dout, att=inp.att)
    ix = _index(dev, ei, N)
    what = f"B H={H} {which}"
    _check_exact(what + " two-pass", _two_pass(dev, ix, H, inp.x, inp.att, None, aggr, scalers, dout, False, what), ref, aggr, 2 * H, pow2)
    dx, datt = _tiled(dev, ix, _build_tiles(ix, H, 0), H, inp.x, inp.att, aggr, dout, "edge", what + " tiled")
    _check_exact(what + " tiled", (None, dx, datt, None), ref, aggr, 2 * H, pow2)


# ---- C: hub rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["nagg4", "nagg5", "staged"])
@pytest.mark.parametrize("ee", [False, True])
@pytest.mark.parametrize("H", [16, 32, 64, 80, 100, 256, 336])          # every LPR; 100, 336: partial lane groups
def test_hub_rows_through_the_long_entry_points(dev, H, ee, which):
    """gsat_pna_fwd_long / gsat_pna_bwd_long on rows of 256 (the row kernels' own loop: > 256 is the hub test), 257, 512, 513 and 1025
    in-edges (k_pna_chunk_stats, the LONG row kernels, k_pna_chunk_apply).  Exact recipe: an extremum attained in chunk 0 and again in a
    later chunk (chunk 0 must win, arg_update / rec_combine), one attained only by the single edge of the last chunk, an att minimum
    repeated across chunks (kmin_a)."""
    ei, N, _ = po.hub_graph()
    _two_pass_case(dev, ei, N, H, which, ("edge",), (ee,), 3000 + H, True, "C", exact_inputs=lambda e: po.hub_exact_inputs(H, 3000 + H, edge_emb=e))


@pytest.mark.parametrize("H", [16, 80, 336])
def test_long_entry_points_on_a_batch_of_one_chunk(dev, H):
    """E = 256 in all: no row can be long, the *_long entry points drop the chunk list (E <= CH) and the row kernels take every row."""
    ei, N = po.one_chunk_graph()
    assert ei.shape[1] == po.LONG_ROW
    _two_pass_case(dev, ei, N, H, "nagg5", ("edge",), (False, True), 3500 + H, True, "C one chunk")


# ---- D: node-attention forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [12, 16, 32, 64, 72, 80, 128, 256])
def test_node_attention_forward(dev, H):
    """gsat_pna_fwd_node_att: the edge weight na[row] * na[source] formed at the load, some na = 0; bit-equal to the lifted reference."""
    from dp_gsat_amd._lib import call, ptr, stream
    ei, N = po.row_length_graph()
    ix = _index(dev, ei, N)
    _, pow2 = po.exact_dout(ei, N, H, po.AGG5, ["identity"], 2, 0)
    for which in ("nagg4", "nagg5", "staged"):
        aggr, scalers = LISTS[which]
        a, A, s, S = _codes(aggr, scalers)
        for recipe in ("exact", "float"):
            inp = po.exact_inputs(ei, N, H, 4000 + H) if recipe == "exact" else po.float_inputs(ei, N, H, 4001 + H)
            assert int((inp.na == 0).sum()) > 0
            out = _nan(dev, N, S * A * 2 * H)
            x, na = inp.x.to(dev), inp.na.to(dev)
            call("gsat_pna_fwd_node_att", ptr(x), ptr(na), ptr(ix.rowptr_dst), ptr(ix.src_by_dst), N, H, a, A, s, S, AVG["lin"], AVG["log"],
                 ptr(out), stream())
            torch.cuda.synchronize()
            what = f"D H={H} {which} {recipe}"
            _written(what, out=out)
            if recipe == "exact":
                _check_out_exact(what, out, po.pna_reference(inp.x, ei, aggr, scalers, AVG, node_att=inp.na), aggr, 2 * H, pow2)
            else:
                r32, r64 = (po.pna_reference(inp.x, ei, aggr, scalers, AVG, node_att=inp.na, dtype=dt) for dt in (np.float32, np.float64))
                close(out, _t(r32.out), ref64=_t(r64.out), what=what)


# ---- E: tiled backward at every window size ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _window_size_refs(name, recipe, mode):
    H, _, planned = CASES[name]
    ei, _, N, _ = _graph(H, planned)
    if recipe == "float":
        inp = _inputs(H, planned)                                # the arrays whose result digests are recorded
        x, att, na, go, dx_add, dna0 = (inp[k] for k in ("x", "att", "na", "go", "dx_add", "dna0"))
        aggr = po.AGG5 if inp["nagg"] == 5 else po.AGG4
    else:
        aggr = po.AGG5 if H == 80 else po.AGG4
        e = po.exact_inputs(ei, N, H, 5000 + H + planned % 7)
        x, att, na, dx_add, dna0 = e.x, e.att, e.na, e.dx_add, e.dna0
        go, _ = po.exact_dout(ei, N, H, aggr, ["identity"], 2, 5001 + H)
    kw = dict(att=att) if mode == "edge" else dict(na=na)
    refs = _refs(x, ei, aggr, ["identity"], go, both=(recipe == "float"), **kw)
    return dict(x=x, w=att if mode == "edge" else na, go=go, dx_add=dx_add, dna0=dna0, aggr=aggr, refs=refs)


@pytest.mark.parametrize("recipe", ["float", "exact"])
@pytest.mark.parametrize("name", list(CASES))
def test_tiled_backward_against_fp64_at_every_window_size(dev, monkeypatch, name, recipe):
    """Every (mode, dx_add, acc) combination of tests/test_gpu_pna_tile_keep.py against the reference: on that file's own inputs (the
    float recipe: this validates the recorded digests, which only say that nothing changed) and, bit for bit, on exact-recipe inputs over
    the same graphs (in-degrees 0, 1, 2; windows of every row count at which a dx_self row changes between registers, the prefetched
    reload and the in-loop reload).  acc = 1 adds the existing d node_att, add = 1 adds dx_add."""
    H, budget, planned = CASES[name]
    monkeypatch.setenv("GSAT_PNA_TILE_LDS", str(budget))
    ei, batch, N, _ = _graph(H, planned)
    ix = _index(dev, ei, N)
    ix.graphs(batch.to(dev))
    tiles = ix.pna_tiles(H)
    assert tiles and (tiles[2], tiles[3]) == _plan(H, budget), "the windows are not the ones the graphs were sized for"
    for mode, acc in MODES:
        c = _window_size_refs(name, recipe, mode)
        lifted = None if mode == "edge" else c["w"][ei[1]] * c["w"][ei[0]]
        for add in (0, 1):
            what = f"E {name} {recipe} {mode} add{add} acc{acc}"
            dx, datt = _tiled(dev, ix, tiles, H, c["x"], c["w"], c["aggr"], c["go"], mode, what, dx_add=c["dx_add"] if add else None,
                              dna0=c["dna0"] if acc else None)
            plus_dx = c["dx_add"].double().numpy() if add else 0.0
            plus_na = c["dna0"].double().numpy() if acc else 0.0
            if recipe == "exact":
                r64 = c["refs"]
                _equal(f"{what} dx", dx, r64.dx + plus_dx)
                _equal(f"{what} datt", datt, r64.datt if mode == "edge" else r64.dna + plus_na)
                continue
            r32, r64 = c["refs"]
            w_dx, w_e = std_conditioning(c["x"], ei, (c["w"] if mode == "edge" else lifted).view(-1, 1), N)
            close_weighted(dx, _t(r32.dx + np.float32(plus_dx)), _t(r64.dx + plus_dx), w_dx, f"{what} dx")
            if mode == "edge":
                close_weighted(datt, _t(r32.datt), _t(r64.datt), w_e, f"{what} datt")
            else:
                close(datt, _t(r32.dna + np.float32(plus_na)), ref64=_t(r64.dna + plus_na), what=f"{what} d node_att")


# ---- F: tiled backward, narrow widths, partial lane groups, a row across the LDS edge capacity ---------------------------------------------
def _smallest_budget(H, edges_cap=16):
    """The smallest GSAT_PNA_TILE_LDS that gsat_pna_tile_plan accepts: te = (budget - 64) / (16 LPR + 24), rounded down to a multiple
    of 8, must reach 16."""
    return 64 + edges_cap * (po.lpr(H) * 16 + 24)


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("H", [8, 12, 16, 32, 48, 72, 100, 132])          # 48: LPR 16 (with five aggregators nowhere else), lanes 12-15 off
def test_tiled_backward_narrow_widths_and_split_rows(dev, H, small):
    """k_pna_bwd_tile<LPR, 4 | 5, edge | node attention> at LPR 4 and 8 (no other test launches them) and with the last lanes of a group
    off at LPR 4, 16, 20, 32 and 64; at the default budget (one window holds the batch) and at the smallest one the plan accepts, where the
    star row of 40 in-edges crosses the LDS edge capacity (`mid` strictly inside the row: its leaves share two feature rows, so the
    extrema tie between a slot in LDS and a slot read from memory) and sources outside their window spill (k_pna_bwd_spill)."""
    from dp_gsat_amd import _lib
    ei, batch, N = po.window_graph()
    ix = _index(dev, ei, N)
    seg = ix.graphs(batch.to(dev))
    budget = _smallest_budget(H) if small else 0
    if small:
        nul = ctypes.c_int32()
        assert _lib.load().gsat_pna_tile_plan(H, budget - 1, ctypes.byref(nul), ctypes.byref(nul), ctypes.byref(nul)) != 0, "not the smallest budget"
    tiles = _build_tiles(ix, H, budget, seg)
    tile_ptr, T, rows_nominal, rows_cap, edges_cap, spill = tiles
    torch.cuda.synchronize()
    desc, rowptr = tile_ptr.cpu().numpy(), ix.rowptr_dst.cpu().numpy()
    starts = desc[:, 0]
    assert starts[0] == 0 and starts[-1] == N and np.diff(starts).min() >= 0 and np.diff(starts).max() <= rows_cap
    lds_slots = None
    if small:
        assert edges_cap in (16, 24)
        t = int(np.searchsorted(starts, po.STAR_CENTRE, side="right")) - 1
        k0 = desc[t, 1]
        beg, end, ne = rowptr[po.STAR_CENTRE] - k0, rowptr[po.STAR_CENTRE + 1] - k0, min(desc[t + 1, 1] - k0, edges_cap)
        assert beg < ne < end, f"the star row [{beg}, {end}) does not cross the LDS edge capacity {ne}"
        assert int(spill[0]) > 0, "no source spilled"
        lds_slots = int(ne - beg)
    for which in ("nagg4", "nagg5"):
        aggr, scalers = LISTS[which]
        for recipe in ("exact", "float"):
            if recipe == "exact":
                inp = po.exact_inputs(ei, N, H, 6000 + H, pool=2)
                dout, _ = po.exact_dout(ei, N, H, aggr, scalers, 2, 6001 + H)
            else:
                inp = po.float_inputs(ei, N, H, 6002 + H)
                dout = po.float_dout(N, H, aggr, scalers, 2, 6003 + H)
            for mode in ("edge", "node"):
                what = f"F H={H} {'small' if small else 'default'} {which} {recipe} {mode}"
                w = inp.att if mode == "edge" else inp.na
                kw = dict(att=w) if mode == "edge" else dict(na=w)
                lifted = w if mode == "edge" else w[ei[1]] * w[ei[0]]
                if recipe == "exact" and lds_slots is not None:          # the tie between an LDS slot and a memory slot is really there
                    es = np.nonzero(ei[1].numpy() == po.STAR_CENTRE)[0]
                    m = (lifted[es, None] * inp.x[ei[0][es]]).numpy()
                    both = [(m[:lds_slots, c_] == m[:, c_].min()).any() and (m[lds_slots:, c_] == m[:, c_].min()).any() for c_ in range(H)]
                    assert any(both), "no minimum tied between an LDS slot and a memory slot"
                dx, datt = _tiled(dev, ix, tiles, H, inp.x, w, aggr, dout, mode, what)
                if recipe == "exact":
                    r64 = _refs(inp.x, ei, aggr, scalers, dout, **kw)
                    _equal(f"{what} dx", dx, r64.dx)
                    _equal(f"{what} datt", datt, r64.datt if mode == "edge" else r64.dna)
                    continue
                r32, r64 = _refs(inp.x, ei, aggr, scalers, dout, both=True, **kw)
                w_dx, w_e = std_conditioning(inp.x, ei, lifted.view(-1, 1), N)
                close_weighted(dx, _t(r32.dx), _t(r64.dx), w_dx, f"{what} dx")
                if mode == "edge":
                    close_weighted(datt, _t(r32.datt), _t(r64.datt), w_e, f"{what} datt")
                else:
                    close(datt, _t(r32.dna), ref64=_t(r64.dna), what=f"{what} d node_att")
