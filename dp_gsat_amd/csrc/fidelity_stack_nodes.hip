// Fidelity curves over NODES: every sparsity level of a node explanation as ONE stacked batch (dp_gsat_amd/subgraph.py:
// explanation_stack_nodes).
//
//   gsat_fidelity_stack_nodes : the V = 2 S + 1 padded NODE-INDUCED extractions "everything", "the nodes of level <= s alone", "everything
//                               but them" side by side -- variant v owns node rows [v N_cap, (v + 1) N_cap), graph ids [v Gp, (v + 1) Gp)
//                               and a fixed edge segment, and holds inside them exactly what gsat_subgraph_padded (node mode) gives for
//                               that mask and capacity.
//
// Unlike the edge stack (fidelity_stack.hip) a variant deletes rows, relabels its endpoints and keeps an edge only when both ends
// survive.  All of it still comes out of order-preserving compactions over the S + 1 level bins:
//   nodes : a node of level L sits in the full variant at its own row, in the keep variants s >= L at the number of earlier real nodes of
//           the bins 0 .. s, in the drop variants s < L at its own row minus that number.  The per-node counts "earlier real nodes of the
//           bins 0 .. b" are kept as an int32 table [N, S + 1]: two of its rows relabel the endpoints of an edge in every variant.
//   edges : hi = max(level[src], level[dst]) -- the edge is in keep variant s iff hi <= s; lo = min(...) -- it is in drop variant s iff
//           lo > s.  Two compactions over one load of the endpoints.
// Workgroups own STKN_ITEMS consecutive node rows or edge slots: k_stkn_hist counts them per bin (wave64 ballots; node and edge
// workgroups in one launch), one workgroup scans the counts and writes the valid words (k_stkn_scan), k_stkn_nodes writes the table and
// the kept rows, k_stkn_edges the kept edges, k_stkn_fill the slack by padding_edge().  5 launches whatever S is, no atomics, integer
// work only.
#include "common.h"
#include "compact.h"
#include <algorithm>

namespace gsat {

constexpr int STKN_BLOCK = 256;                    // 4 waves
constexpr int STKN_IPT = 4;                        // consecutive items per thread
constexpr int STKN_ITEMS = STKN_BLOCK * STKN_IPT;  // node rows / edge slots per workgroup: gsat_fidelity_stack_block_items()
constexpr int STKN_SCAN_BLOCK = 1024;
constexpr int STKN_MAX_LEVELS = 16;
constexpr int STKN_MAX_VARIANTS = 2 * STKN_MAX_LEVELS + 1;

struct StknSegs { int64_t off[STKN_MAX_VARIANTS + 1]; };      // variant v owns the edge slots [off[v], off[v + 1]) of the stack

// The counted nodes / edges of the input: (N_real, E_real) of its valid word, clamped to the arrays; nothing of an input that overflowed.
__device__ __forceinline__ void stkn_counts(const int32_t* __restrict__ valid_in, int64_t N, int64_t E, int64_t& Nv, int64_t& Ev) {
    Nv = N; Ev = E;
    if (valid_in) {
        const bool spoiled = valid_in[3] != 0;
        Nv = spoiled ? 0 : min<int64_t>(max<int64_t>(valid_in[0], 0), N);
        Ev = spoiled ? 0 : min<int64_t>(max<int64_t>(valid_in[1], 0), E);
    }
}

// This thread's node rows: bin (level clamped to S) and whether the row is real.  Rows at or beyond Nv are never loaded.
struct StknNodes { int bin[STKN_IPT]; uint32_t real; };

__device__ __forceinline__ StknNodes stkn_load_nodes(const uint8_t* __restrict__ level, int S, int64_t i0, int64_t Nv) {
    StknNodes it;
    it.real = 0;
#pragma unroll
    for (int j = 0; j < STKN_IPT; ++j) {
        it.bin[j] = S;
        if (i0 + j < Nv) {
            it.bin[j] = min((int)level[i0 + j], S);
            it.real |= 1u << j;
        }
    }
    return it;
}

// This thread's edge slots: endpoints, hi = max and lo = min of the endpoints' bins, and whether the slot counts -- below Ev with both
// ends below Nv.  `bad` receives 1 when a counted slot has an endpoint out of range.  Slots at or beyond Ev are never loaded, and a level
// byte is only read at an endpoint below Nv.
struct StknEdges { int32_t s[STKN_IPT], d[STKN_IPT]; int hi[STKN_IPT], lo[STKN_IPT]; uint32_t real; };

__device__ __forceinline__ StknEdges stkn_load_edges(const int64_t* __restrict__ ei, int64_t E, int64_t Ev, int64_t Nv,
                                                     const uint8_t* __restrict__ level, int S, int64_t i0, int& bad) {
    StknEdges it;
    it.real = 0;
    bad = 0;
#pragma unroll
    for (int j = 0; j < STKN_IPT; ++j) {
        it.s[j] = 0; it.d[j] = 0; it.hi[j] = S; it.lo[j] = S;
        if (i0 + j < Ev) {
            const int64_t s = ei[i0 + j], d = ei[E + i0 + j];
            if ((uint64_t)s < (uint64_t)Nv && (uint64_t)d < (uint64_t)Nv) {
                const int ls = min((int)level[s], S), ld = min((int)level[d], S);
                it.s[j] = (int32_t)s; it.d[j] = (int32_t)d;              // below Nv <= N < 2^31
                it.hi[j] = max(ls, ld); it.lo[j] = min(ls, ld);
                it.real |= 1u << j;
            } else {
                bad = 1;
            }
        }
    }
    return it;
}

// bit j = item j counts and its bin is b
__device__ __forceinline__ uint32_t stkn_bits(const int (&bin)[STKN_IPT], uint32_t real, int b) {
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < STKN_IPT; ++j) bits |= (((real >> j) & 1u) && bin[j] == b) ? (1u << j) : 0u;
    return bits;
}

// the workgroup's items with `bits` set, per wave, into sh[b][wave]
__device__ __forceinline__ void stkn_wave_count(uint32_t bits, int* row) {
    int wave_total = 0;
#pragma unroll
    for (int j = 0; j < STKN_IPT; ++j) wave_total += __popcll(__ballot((bits >> j) & 1u));
    if ((threadIdx.x & 63) == 0) row[threadIdx.x >> 6] = wave_total;
}

// Workgroups [0, nbn): cnt_n[b * nbn + workgroup] = the workgroup's real nodes of bin b, 0 <= b <= S.
// Workgroups [nbn, nbn + nbe): cnt_hi / cnt_lo[b * nbe + workgroup] = its counted edges whose hi / lo bin is b; bad[workgroup] = an
// endpoint was out of range.
__global__ void __launch_bounds__(STKN_BLOCK)
k_stkn_hist(const int64_t* __restrict__ ei, int64_t E, int64_t N, const int32_t* __restrict__ valid_in, const uint8_t* __restrict__ level, int S,
            int nbn, int nbe, int32_t* __restrict__ cnt_n, int32_t* __restrict__ cnt_hi, int32_t* __restrict__ cnt_lo,
            int32_t* __restrict__ bad) {
    __shared__ int sh[2][STKN_MAX_LEVELS + 1][STKN_BLOCK / 64];
    int64_t Nv, Ev;
    stkn_counts(valid_in, N, E, Nv, Ev);
    if ((int)blockIdx.x < nbn) {
        const StknNodes it = stkn_load_nodes(level, S, (int64_t)blockIdx.x * STKN_ITEMS + (int64_t)threadIdx.x * STKN_IPT, Nv);
        for (int b = 0; b <= S; ++b) stkn_wave_count(stkn_bits(it.bin, it.real, b), sh[0][b]);
        __syncthreads();
        if ((int)threadIdx.x <= S) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < STKN_BLOCK / 64; ++w) total += sh[0][threadIdx.x][w];
            cnt_n[(int64_t)threadIdx.x * nbn + blockIdx.x] = total;
        }
        return;
    }
    const int wg = (int)blockIdx.x - nbn;
    int any_bad;
    const StknEdges it = stkn_load_edges(ei, E, Ev, Nv, level, S, (int64_t)wg * STKN_ITEMS + (int64_t)threadIdx.x * STKN_IPT, any_bad);
    for (int b = 0; b <= S; ++b) {
        stkn_wave_count(stkn_bits(it.hi, it.real, b), sh[0][b]);
        stkn_wave_count(stkn_bits(it.lo, it.real, b), sh[1][b]);
    }
    any_bad = __syncthreads_or(any_bad);
    if ((int)threadIdx.x < 2 * (S + 1)) {
        const int k = (int)threadIdx.x / (S + 1), b = (int)threadIdx.x - k * (S + 1);
        int total = 0;
#pragma unroll
        for (int w = 0; w < STKN_BLOCK / 64; ++w) total += sh[k][b][w];
        (k ? cnt_lo : cnt_hi)[(int64_t)b * nbe + wg] = total;
    }
    if (threadIdx.x == 0) bad[wg] = any_bad ? 1 : 0;
}

// Workgroup counts -> workgroup offsets, bin by bin, for the nodes and both edge compactions, and the valid words: thread v < V writes
// valid_out[v] = (N'_v, E'_v, graphs, 0), or (0, 0, 0, 1) when two padding nodes would not remain behind the variant's N'_v rows, its edges
// do not fit its segment, the input had overflowed or an edge had a bad id -- the rule of k_subp_scan, variant by variant.
__global__ void __launch_bounds__(STKN_SCAN_BLOCK)
k_stkn_scan(int32_t* __restrict__ cnt_n, int nbn, int32_t* __restrict__ cnt_hi, int32_t* __restrict__ cnt_lo, int nbe,
            const int32_t* __restrict__ bad, int S, int64_t N, int64_t E, int64_t cap_nodes, StknSegs seg, const int32_t* __restrict__ valid_in,
            int64_t G, int32_t* __restrict__ valid_out) {
    __shared__ int sh[STKN_SCAN_BLOCK / 64];
    __shared__ int tot[3][STKN_MAX_LEVELS + 1];
    for (int b = 0; b <= S; ++b) {
        const int tn = scan_counts<STKN_SCAN_BLOCK>(cnt_n + (int64_t)b * nbn, nbn, sh);
        const int th = scan_counts<STKN_SCAN_BLOCK>(cnt_hi + (int64_t)b * nbe, nbe, sh);
        const int tl = scan_counts<STKN_SCAN_BLOCK>(cnt_lo + (int64_t)b * nbe, nbe, sh);
        if (threadIdx.x == 0) { tot[0][b] = tn; tot[1][b] = th; tot[2][b] = tl; }
    }
    int any_bad = 0;
    for (int i = threadIdx.x; i < nbe; i += STKN_SCAN_BLOCK) any_bad |= bad[i];
    any_bad = __syncthreads_or(any_bad);         // also orders the writes of tot
    const int V = 2 * S + 1, v = threadIdx.x;
    if (v >= V) return;
    const int s = v == 0 ? S : (v - 1) % S;
    int64_t n_all = 0, n_upto = 0, e_all = 0, hi_upto = 0, lo_upto = 0;
    for (int b = 0; b <= S; ++b) {
        n_all += tot[0][b];
        e_all += tot[1][b];
        if (b <= s) { n_upto += tot[0][b]; hi_upto += tot[1][b]; lo_upto += tot[2][b]; }
    }
    const int64_t kept_n = v == 0 ? n_all : (v <= S ? n_upto : n_all - n_upto);
    const int64_t kept_e = v == 0 ? e_all : (v <= S ? hi_upto : e_all - lo_upto);
    int64_t lo = 0, hi = 0;
    for (int u = 0; u < V; ++u)
        if (u == v) { lo = seg.off[u]; hi = seg.off[u + 1]; }
    const bool over = kept_n + 2 > cap_nodes || kept_e > hi - lo || any_bad || (valid_in && valid_in[3] != 0);
    int32_t* o = valid_out + 4 * v;
    o[0] = over ? 0 : (int32_t)kept_n;
    o[1] = over ? 0 : (int32_t)kept_e;
    o[2] = over ? 0 : (valid_in ? valid_in[2] : (int32_t)G);
    o[3] = over ? 1 : 0;
}

// table[i * (S + 1) + b] = the real nodes before i whose bin is in 0 .. b, for every real node i, built up bin by bin on top of the
// workgroup offsets; and every real node goes to its S + 1 variants: row i of the full variant, row table[i][s] of keep variant s >= its
// bin, row i - table[i][s] of drop variant s < its bin.  A row at or beyond cap_nodes is not written (that variant has overflowed and
// k_stkn_fill owns all of it).
__global__ void __launch_bounds__(STKN_BLOCK)
k_stkn_nodes(int64_t N, const int32_t* __restrict__ valid_in, const uint8_t* __restrict__ level, int S, int nbn, const int32_t* __restrict__ off_n,
             const int64_t* __restrict__ batch, int64_t cap_nodes, int64_t Gp, int32_t* __restrict__ table, int64_t* __restrict__ out_node_id,
             int64_t* __restrict__ out_batch) {
    __shared__ int sh[STKN_BLOCK / 64];
    int64_t Nv, Ev;
    stkn_counts(valid_in, N, 0, Nv, Ev);
    const int64_t i0 = (int64_t)blockIdx.x * STKN_ITEMS + (int64_t)threadIdx.x * STKN_IPT;
    const StknNodes it = stkn_load_nodes(level, S, i0, Nv);
    int64_t g[STKN_IPT];
    int32_t upto[STKN_IPT];
#pragma unroll
    for (int j = 0; j < STKN_IPT; ++j) {
        upto[j] = 0;
        g[j] = 0;
        if ((it.real >> j) & 1u) {
            g[j] = batch[i0 + j];
            if (i0 + j < cap_nodes) {
                out_node_id[i0 + j] = i0 + j;
                out_batch[i0 + j] = g[j];
            }
        }
    }
    int unused;
    for (int b = 0; b <= S; ++b) {
        const uint32_t bits = stkn_bits(it.bin, it.real, b);
        const int first = off_n[(int64_t)b * nbn + blockIdx.x] + block_rank<STKN_IPT, STKN_BLOCK>(bits, sh, unused);
#pragma unroll
        for (int j = 0; j < STKN_IPT; ++j) {
            upto[j] += first + __popc(bits & ((1u << j) - 1u));
            if (!((it.real >> j) & 1u)) continue;
            table[(i0 + j) * (int64_t)(S + 1) + b] = upto[j];
            if (b == S) continue;
            const bool kept = it.bin[j] <= b;
            const int64_t v = kept ? 1 + b : 1 + S + b;
            const int64_t pos = kept ? (int64_t)upto[j] : i0 + j - (int64_t)upto[j];
            if (pos < cap_nodes) {
                out_node_id[v * cap_nodes + pos] = i0 + j;
                out_batch[v * cap_nodes + pos] = v * Gp + g[j];
            }
        }
    }
}

// Every counted edge goes to the full variant, the keep variants s >= hi and the drop variants s < lo, at segment start + its rank among
// the variant's edges, its endpoints relabelled through the table and moved to the variant's node rows.  `full` is the edge's rank among
// all counted edges, `upto_hi` / `upto_lo` its rank among those whose hi / lo bin is in 0 .. s, built up bin by bin.  A position at or
// beyond the segment's capacity is not written (that variant has overflowed and k_stkn_fill owns all of it).
__global__ void __launch_bounds__(STKN_BLOCK)
k_stkn_edges(const int64_t* __restrict__ ei, int64_t E, int64_t N, const int32_t* __restrict__ valid_in, const uint8_t* __restrict__ level, int S,
             int nbe, const int32_t* __restrict__ off_hi, const int32_t* __restrict__ off_lo, const int32_t* __restrict__ table,
             int64_t cap_nodes, StknSegs seg, int64_t E_stack, int64_t* __restrict__ out_ei, int64_t* __restrict__ out_id) {
    __shared__ int sh[STKN_BLOCK / 64];
    int64_t Nv, Ev;
    stkn_counts(valid_in, N, E, Nv, Ev);
    const int64_t i0 = (int64_t)blockIdx.x * STKN_ITEMS + (int64_t)threadIdx.x * STKN_IPT;
    int any_bad;
    const StknEdges it = stkn_load_edges(ei, E, Ev, Nv, level, S, i0, any_bad);
    int32_t block_all = 0;
    for (int b = 0; b <= S; ++b) block_all += off_hi[(int64_t)b * nbe + blockIdx.x];
    int unused;
    const int first_all = block_rank<STKN_IPT, STKN_BLOCK>(it.real, sh, unused);
    int32_t full[STKN_IPT], upto_hi[STKN_IPT], upto_lo[STKN_IPT];
    {
        const int64_t lo = seg.off[0], cap = seg.off[1] - lo;
#pragma unroll
        for (int j = 0; j < STKN_IPT; ++j) {
            full[j] = block_all + first_all + __popc(it.real & ((1u << j) - 1u));
            upto_hi[j] = 0; upto_lo[j] = 0;
            if (((it.real >> j) & 1u) && full[j] < cap) {                // every real node sits at its own row of the full variant
                out_ei[lo + full[j]] = it.s[j];
                out_ei[E_stack + lo + full[j]] = it.d[j];
                out_id[lo + full[j]] = i0 + j;
            }
        }
    }
    const int64_t stride = S + 1;
    for (int s = 0; s < S; ++s) {
        const uint32_t bits_hi = stkn_bits(it.hi, it.real, s), bits_lo = stkn_bits(it.lo, it.real, s);
        const int first_hi = off_hi[(int64_t)s * nbe + blockIdx.x] + block_rank<STKN_IPT, STKN_BLOCK>(bits_hi, sh, unused);
        const int first_lo = off_lo[(int64_t)s * nbe + blockIdx.x] + block_rank<STKN_IPT, STKN_BLOCK>(bits_lo, sh, unused);
        const int64_t keep_lo = seg.off[1 + s], keep_cap = seg.off[2 + s] - keep_lo;
        const int64_t drop_lo = seg.off[1 + S + s], drop_cap = seg.off[2 + S + s] - drop_lo;
#pragma unroll
        for (int j = 0; j < STKN_IPT; ++j) {
            upto_hi[j] += first_hi + __popc(bits_hi & ((1u << j) - 1u));
            upto_lo[j] += first_lo + __popc(bits_lo & ((1u << j) - 1u));
            if (!((it.real >> j) & 1u)) continue;
            const bool kept = it.hi[j] <= s, dropped = it.lo[j] > s;      // never both: lo <= hi
            if (!kept && !dropped) continue;
            const int v = kept ? 1 + s : 1 + S + s;
            const int64_t pos = kept ? (int64_t)upto_hi[j] : (int64_t)full[j] - upto_lo[j];
            const int64_t lo = kept ? keep_lo : drop_lo, cap = kept ? keep_cap : drop_cap;
            if (pos < cap) {
                const int64_t ts = table[it.s[j] * stride + s], td = table[it.d[j] * stride + s];
                out_ei[lo + pos] = (kept ? ts : it.s[j] - ts) + (int64_t)v * cap_nodes;
                out_ei[E_stack + lo + pos] = (kept ? td : it.d[j] - td) + (int64_t)v * cap_nodes;
                out_id[lo + pos] = i0 + j;
            }
        }
    }
}

// Thread i takes node row i and edge slot i of the stack and reads the counts of its variant from valid_out.  A row behind the
// variant's N' is a padding node (id -1, the variant's padding graph); an edge slot behind its E' is padding edge number (slot - E') among
// the variant's own padding nodes, id -1.
__global__ void __launch_bounds__(STKN_BLOCK)
k_stkn_fill(const int32_t* __restrict__ valid_out, int V, int64_t cap_nodes, int64_t Gp, StknSegs seg, int64_t E_stack,
            int64_t* __restrict__ out_node_id, int64_t* __restrict__ out_batch, int64_t* __restrict__ out_ei, int64_t* __restrict__ out_id) {
    const int64_t i = (int64_t)blockIdx.x * STKN_BLOCK + threadIdx.x;
    if (i < (int64_t)V * cap_nodes) {
        const int64_t v = i / cap_nodes, r = i - v * cap_nodes;
        if (r >= valid_out[4 * v]) {
            out_node_id[i] = -1;
            out_batch[i] = v * Gp + Gp - 1;
        }
    }
    if (i < E_stack) {
        int v = 0;
        int64_t lo = seg.off[0], hi = seg.off[V];
        for (int u = 1; u < V; ++u) {
            const int64_t o = seg.off[u];
            if (i >= o) { lo = o; v = u; } else { hi = min(hi, o); }
        }
        const int64_t Nr = valid_out[4 * v], Er = valid_out[4 * v + 1], j = i - lo;
        if (j >= Er) {
            int64_t src, dst;
            padding_edge(Nr, cap_nodes - Nr, (hi - lo) - Er, j - Er, src, dst);
            out_id[i] = -1;
            out_ei[i] = src + (int64_t)v * cap_nodes;
            out_ei[E_stack + i] = dst + (int64_t)v * cap_nodes;
        }
    }
}

struct StknLayout {
    int nbn, nbe;
    size_t rows_n, rows_e, table, bytes;
    StknLayout(int64_t N, int64_t E, int64_t S) {
        nbn = (int)ceil_div(N, STKN_ITEMS);
        nbe = (int)ceil_div(E, STKN_ITEMS);
        rows_n = (size_t)(S + 1) * (size_t)std::max(nbn, 1);
        rows_e = (size_t)(S + 1) * (size_t)std::max(nbe, 1);
        table = (size_t)std::max<int64_t>(N, 1) * (size_t)(S + 1);
        bytes = 256 + align_up(rows_n * 4, 256) + 2 * align_up(rows_e * 4, 256) + align_up((size_t)std::max(nbe, 1) * 4, 256) +
                align_up(table * 4, 256);
    }
};

}  // namespace gsat

using namespace gsat;

extern "C" {

size_t gsat_fidelity_stack_nodes_workspace_bytes(int64_t N, int64_t E, int64_t levels) {
    if (N < 0 || E < 0 || N >= (1ll << 31) || E >= (1ll << 31) || levels < 1 || levels > STKN_MAX_LEVELS) return 0;
    return StknLayout(N, E, levels).bytes;
}

int gsat_fidelity_stack_nodes(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* batch, int64_t G, const int32_t* valid_in,
                              const uint8_t* node_level, int64_t levels, int64_t graphs_per_variant, int64_t cap_nodes,
                              const int64_t* segment_offsets, int64_t* out_edge_index, int64_t* out_edge_id, int64_t* out_node_id,
                              int64_t* out_batch, int32_t* valid_out, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && N >= 0 && G >= 0 && levels >= 1 && levels <= STKN_MAX_LEVELS && graphs_per_variant >= 1 && cap_nodes >= 2 &&
                 segment_offsets, GSAT_ERR_ARG, "gsat_fidelity_stack_nodes: bad argument (1..16 levels, a padding graph, two padding nodes)");
    const int S = (int)levels, V = 2 * S + 1;
    StknSegs seg;
    for (int v = 0; v <= STKN_MAX_VARIANTS; ++v) seg.off[v] = segment_offsets[std::min(v, V)];
    GSAT_REQUIRE(seg.off[0] == 0, GSAT_ERR_ARG, "gsat_fidelity_stack_nodes: segment_offsets must start at 0");
    for (int v = 0; v < V; ++v)
        GSAT_REQUIRE(seg.off[v + 1] >= seg.off[v], GSAT_ERR_ARG, "gsat_fidelity_stack_nodes: segment_offsets must not decrease");
    const int64_t E_stack = seg.off[V];
    GSAT_REQUIRE(E < (1ll << 31) && N < (1ll << 31) && G < (1ll << 31) && E_stack < (1ll << 31) && cap_nodes < (1ll << 31) / V &&
                 graphs_per_variant < (1ll << 31) / V, GSAT_ERR_UNSUPPORTED, "gsat_fidelity_stack_nodes: >2^31 entries");
    GSAT_REQUIRE(valid_out && out_batch && out_node_id && (N == 0 || (batch && node_level)) && (E == 0 || edge_index) &&
                 (E_stack == 0 || (out_edge_index && out_edge_id)), GSAT_ERR_ARG, "gsat_fidelity_stack_nodes: null pointer");
    const StknLayout lay(N, E, S);
    Arena ar(workspace, ws_bytes);
    int32_t* cnt_n = ar.take<int32_t>(lay.rows_n);
    int32_t* cnt_hi = ar.take<int32_t>(lay.rows_e);
    int32_t* cnt_lo = ar.take<int32_t>(lay.rows_e);
    int32_t* bad = ar.take<int32_t>((size_t)std::max(lay.nbe, 1));
    int32_t* table = ar.take<int32_t>(lay.table);
    GSAT_REQUIRE(ar.ok() && table, GSAT_ERR_WORKSPACE, "gsat_fidelity_stack_nodes: workspace %zu < %zu", ws_bytes, ar.off);
    // without a node no edge counts (every endpoint is out of range): the edge workgroups still run, to report it
    const int nbn = lay.nbn, nbe = lay.nbe;
    if (nbn + nbe > 0) {
        k_stkn_hist<<<nbn + nbe, STKN_BLOCK, 0, stream>>>(edge_index, E, N, valid_in, node_level, S, nbn, nbe, cnt_n, cnt_hi, cnt_lo, bad);
        GSAT_LAUNCH_CHECK();
    }
    k_stkn_scan<<<1, STKN_SCAN_BLOCK, 0, stream>>>(cnt_n, nbn, cnt_hi, cnt_lo, nbe, bad, S, N, E, cap_nodes, seg, valid_in, G, valid_out);
    GSAT_LAUNCH_CHECK();
    if (nbn > 0) {
        k_stkn_nodes<<<nbn, STKN_BLOCK, 0, stream>>>(N, valid_in, node_level, S, nbn, cnt_n, batch, cap_nodes, graphs_per_variant, table,
                                                     out_node_id, out_batch);
        GSAT_LAUNCH_CHECK();
    }
    if (nbe > 0) {
        k_stkn_edges<<<nbe, STKN_BLOCK, 0, stream>>>(edge_index, E, N, valid_in, node_level, S, nbe, cnt_hi, cnt_lo, table, cap_nodes, seg,
                                                     E_stack, out_edge_index, out_edge_id);
        GSAT_LAUNCH_CHECK();
    }
    const int64_t items = std::max<int64_t>(std::max(E_stack, (int64_t)V * cap_nodes), 1);
    k_stkn_fill<<<(unsigned)ceil_div(items, STKN_BLOCK), STKN_BLOCK, 0, stream>>>(valid_out, V, cap_nodes, graphs_per_variant, seg, E_stack,
                                                                                out_node_id, out_batch, out_edge_index, out_edge_id);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
