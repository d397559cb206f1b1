// Fidelity curves: every sparsity level of a batch's explanation as ONE stacked batch (dp_gsat_amd/subgraph.py: explanation_stack).
//
//   gsat_fidelity_levels : level[e] = the smallest level s whose top-k_s (or top-ratio_s) of the edge's graph holds the edge, from ONE
//                          ranking; S when no level does.  `level <= s` is the mask of level s: the kept sets are nested.
//   gsat_fidelity_stack  : the V = 2 S + 1 padded extractions "everything", "level s alone", "everything but level s" side by side --
//                          variant v owns node rows [v N_cap, (v + 1) N_cap), graph ids [v Gp, (v + 1) Gp) and a fixed edge segment, and
//                          holds inside it exactly what gsat_subgraph_padded gives for that mask and capacity (every node kept).
//   gsat_fidelity_stack_multi : the same for R rankings around ONE full variant, V = 1 + 2 R S (explanation_stack_multi).
//   gsat_level_overlap   : per level, how many edges two rankings both keep, and how many each keeps (level_overlap).
//
// Every node is kept, so a variant differs from the batch in its edge list only, and an edge of level L goes to the full variant, the
// keep variants s >= L and the drop variants s < L: S + 1 copies.  Its position in "level <= s" is the number of earlier edges of the
// bins 0 .. s, in "level > s" its position among all edges minus that: ONE order-preserving compaction over the S + 1 level bins gives
// every position.  Workgroups own STK_ITEMS consecutive edge slots: k_stk_hist counts them per bin (wave64 ballots), one workgroup scans
// the counts per bin and writes the valid words, k_stk_scatter redoes the in-workgroup ranks bin by bin on top of its offsets, and
// k_stk_fill writes the slack by padding_edge() and the batch vector.  4 launches whatever S is, no atomics, integer work only.
#include "common.h"
#include "compact.h"
#include <algorithm>

namespace gsat {

constexpr int STK_BLOCK = 256;                   // 4 waves
constexpr int STK_IPT = 4;                       // consecutive edge slots per thread
constexpr int STK_ITEMS = STK_BLOCK * STK_IPT;   // edge slots per workgroup
constexpr int STK_SCAN_BLOCK = 1024;
constexpr int STK_MAX_LEVELS = 16;
constexpr int STK_MAX_VARIANTS = 2 * STK_MAX_LEVELS + 1;

struct StkLevels { int S, by_ratio; int64_t k[STK_MAX_LEVELS]; double ratio[STK_MAX_LEVELS]; };
struct StkSegs { int64_t off[STK_MAX_VARIANTS + 1]; };      // variant v owns the edge slots [off[v], off[v + 1]) of the stack

// One thread per edge slot.  An edge of a graph that was not ranked (the padding graph) is in no level, and its rank is not read.
__global__ void __launch_bounds__(STK_BLOCK)
k_stk_levels(const int32_t* __restrict__ rank, const int32_t* __restrict__ edge_ptr, const int32_t* __restrict__ edge_graph, int64_t E,
             int64_t G, StkLevels lv, uint8_t* __restrict__ level) {
    const int64_t e = (int64_t)blockIdx.x * STK_BLOCK + threadIdx.x;
    if (e >= E) return;
    const int64_t g = edge_graph[e];
    int out = lv.S;
    if (g >= 0 && g < G) {
        const int64_t Eg = (int64_t)edge_ptr[g + 1] - (int64_t)edge_ptr[g], r = rank[e];
        for (int s = lv.S - 1; s >= 0; --s) {    // the counts do not decrease with s: the last s that holds the edge is the smallest
            const int64_t kc = lv.by_ratio ? (int64_t)ceil((double)Eg * lv.ratio[s]) : min<int64_t>(lv.k[s], Eg);
            if (r < kc) out = s;
        }
    }
    level[e] = (uint8_t)out;
}

// The counted nodes / edges of the input: (N_real, E_real) of its valid word, clamped to the arrays; nothing of an input that overflowed.
__device__ __forceinline__ void stk_counts(const int32_t* __restrict__ valid_in, int64_t N, int64_t E, int64_t& Nv, int64_t& Ev) {
    Nv = N; Ev = E;
    if (valid_in) {
        const bool spoiled = valid_in[3] != 0;
        Nv = spoiled ? 0 : min<int64_t>(max<int64_t>(valid_in[0], 0), N);
        Ev = spoiled ? 0 : min<int64_t>(max<int64_t>(valid_in[1], 0), E);
    }
}

// This thread's STK_IPT edge slots: endpoints, bin (level clamped to S) and whether the slot counts -- below Ev with both ends below Nv.
// `bad` receives 1 when a counted slot has an endpoint out of range.  Slots at or beyond Ev are never loaded.
struct StkItems { int64_t s[STK_IPT], d[STK_IPT]; int bin[STK_IPT]; uint32_t real; };

__device__ __forceinline__ StkItems stk_load(const int64_t* __restrict__ ei, int64_t E, int64_t Ev, int64_t Nv, const uint8_t* __restrict__ level,
                                             int S, int64_t i0, int& bad) {
    StkItems it;
    it.real = 0;
    bad = 0;
#pragma unroll
    for (int j = 0; j < STK_IPT; ++j) {
        it.s[j] = 0; it.d[j] = 0; it.bin[j] = S;
        if (i0 + j < Ev) {
            it.s[j] = ei[i0 + j];
            it.d[j] = ei[E + i0 + j];
            it.bin[j] = min((int)level[i0 + j], S);
            const bool in_range = (uint64_t)it.s[j] < (uint64_t)Nv && (uint64_t)it.d[j] < (uint64_t)Nv;
            if (in_range) it.real |= 1u << j; else bad = 1;
        }
    }
    return it;
}

// bit j = item j counts and lies in bin b
__device__ __forceinline__ uint32_t stk_bits(const StkItems& it, int b) {
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < STK_IPT; ++j) bits |= (((it.real >> j) & 1u) && it.bin[j] == b) ? (1u << j) : 0u;
    return bits;
}

// cnt[b * nb + workgroup] = the workgroup's counted edges of bin b, 0 <= b <= S; bad[workgroup] = an endpoint was out of range
__global__ void __launch_bounds__(STK_BLOCK)
k_stk_hist(const int64_t* __restrict__ ei, int64_t E, int64_t N, const int32_t* __restrict__ valid_in, const uint8_t* __restrict__ level, int S,
           int nb, int32_t* __restrict__ cnt, int32_t* __restrict__ bad) {
    __shared__ int sh[STK_MAX_LEVELS + 1][STK_BLOCK / 64];
    int64_t Nv, Ev;
    stk_counts(valid_in, N, E, Nv, Ev);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int any_bad;
    const StkItems it = stk_load(ei, E, Ev, Nv, level, S, (int64_t)blockIdx.x * STK_ITEMS + (int64_t)threadIdx.x * STK_IPT, any_bad);
    for (int b = 0; b <= S; ++b) {
        const uint32_t bits = stk_bits(it, b);
        int wave_total = 0;
#pragma unroll
        for (int j = 0; j < STK_IPT; ++j) wave_total += __popcll(__ballot((bits >> j) & 1u));
        if (lane == 0) sh[b][wave] = wave_total;
    }
    any_bad = __syncthreads_or(any_bad);
    if ((int)threadIdx.x <= S) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < STK_BLOCK / 64; ++w) total += sh[threadIdx.x][w];
        cnt[(int64_t)threadIdx.x * nb + blockIdx.x] = total;
    }
    if (threadIdx.x == 0) bad[blockIdx.x] = any_bad ? 1 : 0;
}

// Workgroup counts -> workgroup offsets, bin by bin, and the valid words: thread v < V writes valid_out[v] = (N', E'_v, graphs, 0), or
// (0, 0, 0, 1) when the variant does not fit its segment, two padding nodes would not remain, the input had overflowed or an edge had a
// bad id -- the rule of k_subp_scan, variant by variant.
__global__ void __launch_bounds__(STK_SCAN_BLOCK)
k_stk_scan(int32_t* __restrict__ cnt, int nb, const int32_t* __restrict__ bad, int S, int64_t N, int64_t E, int64_t cap_nodes, StkSegs seg,
           const int32_t* __restrict__ valid_in, int64_t G, int32_t* __restrict__ valid_out) {
    __shared__ int sh[STK_SCAN_BLOCK / 64];
    __shared__ int tot[STK_MAX_LEVELS + 1];
    for (int b = 0; b <= S; ++b) {
        const int t = scan_counts<STK_SCAN_BLOCK>(cnt + (int64_t)b * nb, nb, sh);
        if (threadIdx.x == 0) tot[b] = t;
    }
    int any_bad = 0;
    for (int i = threadIdx.x; i < nb; i += STK_SCAN_BLOCK) any_bad |= bad[i];
    any_bad = __syncthreads_or(any_bad);         // also orders the writes of tot
    const int V = 2 * S + 1, v = threadIdx.x;
    if (v >= V) return;
    int64_t Nv, Ev;
    stk_counts(valid_in, N, E, Nv, Ev);
    int64_t all = 0, upto = 0;                   // every counted edge; those of the bins 0 .. s of this variant's level s
    const int s = v == 0 ? S : (v - 1) % S;
    for (int b = 0; b <= S; ++b) {
        all += tot[b];
        if (b <= s) upto += tot[b];
    }
    const int64_t kept = v == 0 ? all : (v <= S ? upto : all - upto);
    int64_t lo = 0, hi = 0;
    for (int u = 0; u < V; ++u)
        if (u == v) { lo = seg.off[u]; hi = seg.off[u + 1]; }
    const bool over = Nv + 2 > cap_nodes || kept > hi - lo || any_bad || (valid_in && valid_in[3] != 0);
    int32_t* o = valid_out + 4 * v;
    o[0] = over ? 0 : (int32_t)Nv;
    o[1] = over ? 0 : (int32_t)kept;
    o[2] = over ? 0 : (valid_in ? valid_in[2] : (int32_t)G);
    o[3] = over ? 1 : 0;
}

// Every counted edge goes to its S + 1 variants, at segment start + its rank among the variant's edges, with its endpoints moved to the
// variant's node rows.  `full` is the edge's rank among all counted edges, `upto` its rank among those of the bins 0 .. s, built up bin
// by bin.  A position at or beyond the segment's capacity is not written (that variant has overflowed and k_stk_fill owns all of it).
__global__ void __launch_bounds__(STK_BLOCK)
k_stk_scatter(const int64_t* __restrict__ ei, int64_t E, int64_t N, const int32_t* __restrict__ valid_in, const uint8_t* __restrict__ level, int S,
              int nb, const int32_t* __restrict__ off, int64_t cap_nodes, StkSegs seg, int64_t E_stack, int64_t* __restrict__ out_ei,
              int64_t* __restrict__ out_id) {
    __shared__ int sh[STK_BLOCK / 64];
    int64_t Nv, Ev;
    stk_counts(valid_in, N, E, Nv, Ev);
    const int64_t i0 = (int64_t)blockIdx.x * STK_ITEMS + (int64_t)threadIdx.x * STK_IPT;
    int any_bad;
    const StkItems it = stk_load(ei, E, Ev, Nv, level, S, i0, any_bad);
    int64_t block_all = 0;
    for (int b = 0; b <= S; ++b) block_all += off[(int64_t)b * nb + blockIdx.x];
    int unused;
    const int first_all = block_rank<STK_IPT, STK_BLOCK>(it.real, sh, unused);
    int64_t full[STK_IPT], upto[STK_IPT];
    {
        const int64_t lo = seg.off[0], cap = seg.off[1] - lo;
#pragma unroll
        for (int j = 0; j < STK_IPT; ++j) {
            full[j] = block_all + first_all + __popc(it.real & ((1u << j) - 1u));
            upto[j] = 0;
            if (((it.real >> j) & 1u) && full[j] < cap) {
                out_ei[lo + full[j]] = it.s[j];
                out_ei[E_stack + lo + full[j]] = it.d[j];
                out_id[lo + full[j]] = i0 + j;
            }
        }
    }
    for (int s = 0; s < S; ++s) {
        const uint32_t bits = stk_bits(it, s);
        const int64_t first = (int64_t)off[(int64_t)s * nb + blockIdx.x] + block_rank<STK_IPT, STK_BLOCK>(bits, sh, unused);
        const int64_t keep_lo = seg.off[1 + s], keep_cap = seg.off[2 + s] - keep_lo;
        const int64_t drop_lo = seg.off[1 + S + s], drop_cap = seg.off[2 + S + s] - drop_lo;
#pragma unroll
        for (int j = 0; j < STK_IPT; ++j) {
            // earlier edges of bin s: those of the workgroups and threads before, and this thread's own earlier items
            upto[j] += first + __popc(bits & ((1u << j) - 1u));
            if (!((it.real >> j) & 1u)) continue;
            const bool kept = it.bin[j] <= s;
            const int v = kept ? 1 + s : 1 + S + s;
            const int64_t pos = kept ? upto[j] : full[j] - upto[j];
            const int64_t lo = kept ? keep_lo : drop_lo, cap = kept ? keep_cap : drop_cap;
            if (pos < cap) {
                out_ei[lo + pos] = it.s[j] + (int64_t)v * cap_nodes;
                out_ei[E_stack + lo + pos] = it.d[j] + (int64_t)v * cap_nodes;
                out_id[lo + pos] = i0 + j;
            }
        }
    }
}

// Thread i takes node row i and edge slot i of the stack and reads the counts of its variant from valid_out.  batch_out = v Gp + the
// input's graph id for the variant's real rows (every row when the variants share the input's own padded rows: `share`), v Gp + pad_graph
// for the rest; an edge slot behind the variant's E' is padding edge number (slot - E') among the variant's own padding nodes, id -1.
__global__ void __launch_bounds__(STK_BLOCK)
k_stk_fill(const int32_t* __restrict__ valid_out, int V, int64_t N, const int64_t* __restrict__ batch, int share, int64_t cap_nodes, int64_t Gp,
           StkSegs seg, int64_t E_stack, int64_t* __restrict__ batch_out, int64_t* __restrict__ out_ei, int64_t* __restrict__ out_id) {
    const int64_t i = (int64_t)blockIdx.x * STK_BLOCK + threadIdx.x;
    if (i < (int64_t)V * cap_nodes) {
        const int64_t v = i / cap_nodes, r = i - v * cap_nodes;
        const bool real = r < N && (share || r < valid_out[4 * v]);
        batch_out[i] = v * Gp + (real ? batch[r] : Gp - 1);
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

struct StkLayout {
    int nb;
    size_t bytes;
    StkLayout(int64_t E, int64_t S) {
        nb = (int)ceil_div(E, STK_ITEMS);
        bytes = 256 + align_up((size_t)(S + 1) * (size_t)std::max(nb, 1) * 4, 256) + align_up((size_t)std::max(nb, 1) * 4, 256);
    }
};

// ---- R rankings around ONE full variant (gsat_fidelity_stack_multi) -----------------------------------------------------------------------
// level is uint8[R, E]; ranking r owns the count rows r (S + 1) + b, 0 <= b <= S, of the workspace.  The variants: 0 the batch itself,
// 1 + r S + s "ranking r, level s alone", 1 + R S + r S + s "the batch without it".  The kernels above stay what gsat_fidelity_stack
// launches: these are separate instantiations, so its register counts and its outputs do not move.  The endpoints of a thread's edge
// slots are loaded once and kept; the R level bytes of a slot are loaded ranking by ranking, each once, and the bin counters are
// wave-uniform ballot popcounts that go straight to LDS: nothing per thread grows with R (S + 1).
constexpr int STK_MAX_BINS = 2 * STK_MAX_LEVELS;        // R (S + 1) <= R S + R <= 2 R S <= 32

// the bins of ranking row `level_r` for this thread's slots; slots at or beyond Ev are never loaded
__device__ __forceinline__ void stkm_bins(StkItems& it, const uint8_t* __restrict__ level_r, int S, int64_t i0, int64_t Ev) {
#pragma unroll
    for (int j = 0; j < STK_IPT; ++j) it.bin[j] = i0 + j < Ev ? min((int)level_r[i0 + j], S) : S;
}

// cnt[(r (S + 1) + b) * nb + workgroup] = the workgroup's counted edges of bin b of ranking r; bad[workgroup] as in k_stk_hist
__global__ void __launch_bounds__(STK_BLOCK)
k_stkm_hist(const int64_t* __restrict__ ei, int64_t E, int64_t N, const int32_t* __restrict__ valid_in, const uint8_t* __restrict__ level, int R,
            int S, int nb, int32_t* __restrict__ cnt, int32_t* __restrict__ bad) {
    __shared__ int sh[STK_MAX_BINS][STK_BLOCK / 64];
    int64_t Nv, Ev;
    stk_counts(valid_in, N, E, Nv, Ev);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * STK_ITEMS + (int64_t)threadIdx.x * STK_IPT;
    int any_bad;
    StkItems it = stk_load(ei, E, Ev, Nv, level, S, i0, any_bad);
    for (int r = 0; r < R; ++r) {
        if (r > 0) stkm_bins(it, level + (int64_t)r * E, S, i0, Ev);
        for (int b = 0; b <= S; ++b) {
            const uint32_t bits = stk_bits(it, b);
            int wave_total = 0;
#pragma unroll
            for (int j = 0; j < STK_IPT; ++j) wave_total += __popcll(__ballot((bits >> j) & 1u));
            if (lane == 0) sh[r * (S + 1) + b][wave] = wave_total;
        }
    }
    any_bad = __syncthreads_or(any_bad);
    if ((int)threadIdx.x < R * (S + 1)) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < STK_BLOCK / 64; ++w) total += sh[threadIdx.x][w];
        cnt[(int64_t)threadIdx.x * nb + blockIdx.x] = total;
    }
    if (threadIdx.x == 0) bad[blockIdx.x] = any_bad ? 1 : 0;
}

// k_stk_scan over the R (S + 1) count rows; thread v < V = 1 + 2 R S writes valid_out[v] by the same rule, its kept edges being those
// of the bins 0 .. s of its own ranking (keep) or the rest (drop).  Every ranking counts the same edges, so `all` is ranking 0's total.
__global__ void __launch_bounds__(STK_SCAN_BLOCK)
k_stkm_scan(int32_t* __restrict__ cnt, int nb, const int32_t* __restrict__ bad, int R, int S, int64_t N, int64_t E, int64_t cap_nodes,
            StkSegs seg, const int32_t* __restrict__ valid_in, int64_t G, int32_t* __restrict__ valid_out) {
    __shared__ int sh[STK_SCAN_BLOCK / 64];
    __shared__ int tot[STK_MAX_BINS];
    const int bins = R * (S + 1);
    for (int b = 0; b < bins; ++b) {
        const int t = scan_counts<STK_SCAN_BLOCK>(cnt + (int64_t)b * nb, nb, sh);
        if (threadIdx.x == 0) tot[b] = t;
    }
    int any_bad = 0;
    for (int i = threadIdx.x; i < nb; i += STK_SCAN_BLOCK) any_bad |= bad[i];
    any_bad = __syncthreads_or(any_bad);         // also orders the writes of tot
    const int RS = R * S, V = 2 * RS + 1, v = threadIdx.x;
    if (v >= V) return;
    int64_t Nv, Ev;
    stk_counts(valid_in, N, E, Nv, Ev);
    const int f = v == 0 ? 0 : (v - 1) % RS, r = f / S, s = v == 0 ? S : f - r * S;
    int64_t all = 0, upto = 0;
    for (int b = 0; b <= S; ++b) {
        const int64_t t = tot[r * (S + 1) + b];
        all += t;
        if (b <= s) upto += t;
    }
    const int64_t kept = v == 0 ? all : (v <= RS ? upto : all - upto);
    int64_t lo = 0, hi = 0;
    for (int u = 0; u < V; ++u)
        if (u == v) { lo = seg.off[u]; hi = seg.off[u + 1]; }
    const bool over = Nv + 2 > cap_nodes || kept > hi - lo || any_bad || (valid_in && valid_in[3] != 0);
    int32_t* o = valid_out + 4 * v;
    o[0] = over ? 0 : (int32_t)Nv;
    o[1] = over ? 0 : (int32_t)kept;
    o[2] = over ? 0 : (valid_in ? valid_in[2] : (int32_t)G);
    o[3] = over ? 1 : 0;
}

// k_stk_scatter ranking by ranking: the full variant once, then for ranking r the S keep and S drop variants from the offsets of its
// own count rows.  An edge goes to 1 + R S slots.  Positions at or beyond a segment's capacity are not written.
__global__ void __launch_bounds__(STK_BLOCK)
k_stkm_scatter(const int64_t* __restrict__ ei, int64_t E, int64_t N, const int32_t* __restrict__ valid_in, const uint8_t* __restrict__ level, int R,
               int S, int nb, const int32_t* __restrict__ off, int64_t cap_nodes, StkSegs seg, int64_t E_stack, int64_t* __restrict__ out_ei,
               int64_t* __restrict__ out_id) {
    __shared__ int sh[STK_BLOCK / 64];
    int64_t Nv, Ev;
    stk_counts(valid_in, N, E, Nv, Ev);
    const int64_t i0 = (int64_t)blockIdx.x * STK_ITEMS + (int64_t)threadIdx.x * STK_IPT;
    int any_bad;
    StkItems it = stk_load(ei, E, Ev, Nv, level, S, i0, any_bad);
    int64_t block_all = 0;
    for (int b = 0; b <= S; ++b) block_all += off[(int64_t)b * nb + blockIdx.x];
    int unused;
    const int first_all = block_rank<STK_IPT, STK_BLOCK>(it.real, sh, unused);
    int64_t full[STK_IPT], upto[STK_IPT];
    {
        const int64_t lo = seg.off[0], cap = seg.off[1] - lo;
#pragma unroll
        for (int j = 0; j < STK_IPT; ++j) {
            full[j] = block_all + first_all + __popc(it.real & ((1u << j) - 1u));
            if (((it.real >> j) & 1u) && full[j] < cap) {
                out_ei[lo + full[j]] = it.s[j];
                out_ei[E_stack + lo + full[j]] = it.d[j];
                out_id[lo + full[j]] = i0 + j;
            }
        }
    }
    const int RS = R * S;
    for (int r = 0; r < R; ++r) {
        if (r > 0) stkm_bins(it, level + (int64_t)r * E, S, i0, Ev);
#pragma unroll
        for (int j = 0; j < STK_IPT; ++j) upto[j] = 0;
        for (int s = 0; s < S; ++s) {
            const uint32_t bits = stk_bits(it, s);
            const int64_t first = (int64_t)off[(int64_t)(r * (S + 1) + s) * nb + blockIdx.x] + block_rank<STK_IPT, STK_BLOCK>(bits, sh, unused);
            const int vk = 1 + r * S + s, vd = vk + RS;
            const int64_t keep_lo = seg.off[vk], keep_cap = seg.off[vk + 1] - keep_lo;
            const int64_t drop_lo = seg.off[vd], drop_cap = seg.off[vd + 1] - drop_lo;
#pragma unroll
            for (int j = 0; j < STK_IPT; ++j) {
                upto[j] += first + __popc(bits & ((1u << j) - 1u));
                if (!((it.real >> j) & 1u)) continue;
                const bool kept = it.bin[j] <= s;
                const int v = kept ? vk : vd;
                const int64_t pos = kept ? upto[j] : full[j] - upto[j];
                const int64_t lo = kept ? keep_lo : drop_lo, cap = kept ? keep_cap : drop_cap;
                if (pos < cap) {
                    out_ei[lo + pos] = it.s[j] + (int64_t)v * cap_nodes;
                    out_ei[E_stack + lo + pos] = it.d[j] + (int64_t)v * cap_nodes;
                    out_id[lo + pos] = i0 + j;
                }
            }
        }
    }
}

struct StkmLayout {
    int nb;
    size_t rows, bytes;
    StkmLayout(int64_t E, int64_t R, int64_t S) {
        nb = (int)ceil_div(E, STK_ITEMS);
        rows = (size_t)(R * (S + 1));
        bytes = 256 + align_up(rows * (size_t)std::max(nb, 1) * 4, 256) + align_up((size_t)std::max(nb, 1) * 4, 256);
    }
};

// ---- agreement of two rankings (gsat_level_overlap) ---------------------------------------------------------------------------------------
constexpr int OVL_BLOCK = 256;
constexpr int OVL_IPT = 4;

// Per workgroup: LDS histograms of a, b and max(a, b) over its counted entries with a level below S, then their running sums --
// #(a <= s), #(b <= s), #(a <= s & b <= s) = #(max(a, b) <= s) -- one int64 atomicAdd per bin.  Integer sums: order does not matter.
__global__ void __launch_bounds__(OVL_BLOCK)
k_level_overlap(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int64_t E, int S, const int32_t* __restrict__ valid,
                unsigned long long* __restrict__ acc) {
    __shared__ int hist[3][STK_MAX_LEVELS];
    int64_t Nv, Ev;
    stk_counts(valid, 0, E, Nv, Ev);
    const int64_t base = (int64_t)blockIdx.x * (OVL_BLOCK * OVL_IPT);
    if (base >= Ev) return;                      // uniform over the workgroup: nothing to add
    if (threadIdx.x < 3 * STK_MAX_LEVELS) hist[threadIdx.x / STK_MAX_LEVELS][threadIdx.x % STK_MAX_LEVELS] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < OVL_IPT; ++j) {
        const int64_t i = base + (int64_t)j * OVL_BLOCK + threadIdx.x;
        if (i < Ev) {
            const int la = a[i], lb = b[i], lm = max(la, lb);
            if (la < S) atomicAdd(&hist[1][la], 1);
            if (lb < S) atomicAdd(&hist[2][lb], 1);
            if (lm < S) atomicAdd(&hist[0][lm], 1);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * S) {
        const int s = threadIdx.x / 3, k = threadIdx.x - 3 * s;
        int upto = 0;
        for (int l = 0; l <= s; ++l) upto += hist[k][l];
        if (upto) atomicAdd(acc + threadIdx.x, (unsigned long long)upto);
    }
}

__global__ void k_level_overlap_reset(int64_t* __restrict__ acc, int n) {
    if (blockIdx.x == 0 && (int)threadIdx.x < n) acc[threadIdx.x] = 0;
}

}  // namespace gsat

using namespace gsat;

extern "C" {

int64_t gsat_fidelity_stack_block_items(void) { return STK_ITEMS; }

size_t gsat_fidelity_stack_workspace_bytes(int64_t E, int64_t levels) {
    if (E < 0 || E >= (1ll << 31) || levels < 1 || levels > STK_MAX_LEVELS) return 0;
    return StkLayout(E, levels).bytes;
}

int gsat_fidelity_levels(const int32_t* rank, const int32_t* edge_ptr, const int32_t* edge_graph, int64_t E, int64_t G, const int64_t* ks,
                         const double* ratios, int64_t levels, uint8_t* level, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && G >= 0 && levels >= 1 && levels <= STK_MAX_LEVELS && (ks != nullptr) != (ratios != nullptr), GSAT_ERR_ARG,
                 "gsat_fidelity_levels: need 1..16 levels as exactly one of ks and ratios");
    GSAT_REQUIRE(E < (1ll << 31) && G < (1ll << 31), GSAT_ERR_UNSUPPORTED, "gsat_fidelity_levels: >2^31 entries");
    StkLevels lv;
    lv.S = (int)levels;
    lv.by_ratio = ratios != nullptr;
    for (int s = 0; s < STK_MAX_LEVELS; ++s) {
        lv.k[s] = ks && s < lv.S ? ks[s] : 0;
        lv.ratio[s] = ratios && s < lv.S ? ratios[s] : 0.0;
    }
    for (int s = 0; s < lv.S; ++s) {
        const bool rising = s == 0 || (ks ? ks[s] > ks[s - 1] : ratios[s] > ratios[s - 1]);
        GSAT_REQUIRE(rising && (ks ? ks[s] >= 1 : (ratios[s] > 0.0 && ratios[s] <= 1.0)), GSAT_ERR_ARG,
                     "gsat_fidelity_levels: levels must be strictly increasing, ks >= 1, ratios in (0, 1]");
    }
    if (E == 0) return GSAT_OK;
    GSAT_REQUIRE(rank && edge_ptr && edge_graph && level, GSAT_ERR_ARG, "gsat_fidelity_levels: null pointer");
    k_stk_levels<<<(unsigned)ceil_div(E, STK_BLOCK), STK_BLOCK, 0, stream>>>(rank, edge_ptr, edge_graph, E, G, lv, level);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_fidelity_stack(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* batch, int64_t G, const int32_t* valid_in,
                        const uint8_t* level, int64_t levels, int64_t graphs_per_variant, int64_t cap_nodes, const int64_t* segment_offsets,
                        int64_t* out_edge_index, int64_t* out_edge_id, int64_t* out_batch, int32_t* valid_out, void* workspace,
                        size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && N >= 0 && G >= 0 && levels >= 1 && levels <= STK_MAX_LEVELS && graphs_per_variant >= 1 && cap_nodes >= 2 &&
                 cap_nodes >= N && segment_offsets, GSAT_ERR_ARG,
                 "gsat_fidelity_stack: bad argument (1..16 levels, a padding graph, two padding nodes, node rows for every input row)");
    const int S = (int)levels, V = 2 * S + 1;
    StkSegs seg;
    for (int v = 0; v <= STK_MAX_VARIANTS; ++v) seg.off[v] = segment_offsets[std::min(v, V)];
    GSAT_REQUIRE(seg.off[0] == 0, GSAT_ERR_ARG, "gsat_fidelity_stack: segment_offsets must start at 0");
    for (int v = 0; v < V; ++v)
        GSAT_REQUIRE(seg.off[v + 1] >= seg.off[v], GSAT_ERR_ARG, "gsat_fidelity_stack: segment_offsets must not decrease");
    const int64_t E_stack = seg.off[V];
    GSAT_REQUIRE(E < (1ll << 31) && N < (1ll << 31) && G < (1ll << 31) && E_stack < (1ll << 31) && cap_nodes < (1ll << 31) / V &&
                 graphs_per_variant < (1ll << 31) / V, GSAT_ERR_UNSUPPORTED, "gsat_fidelity_stack: >2^31 entries");
    GSAT_REQUIRE(valid_out && out_batch && (N == 0 || batch) && (E == 0 || (edge_index && level)) &&
                 (E_stack == 0 || (out_edge_index && out_edge_id)), GSAT_ERR_ARG, "gsat_fidelity_stack: null pointer");
    const StkLayout lay(E, S);
    Arena ar(workspace, ws_bytes);
    int32_t* cnt = ar.take<int32_t>((size_t)(S + 1) * (size_t)std::max(lay.nb, 1));
    int32_t* bad = ar.take<int32_t>((size_t)std::max(lay.nb, 1));
    GSAT_REQUIRE(ar.ok() && bad, GSAT_ERR_WORKSPACE, "gsat_fidelity_stack: workspace %zu < %zu", ws_bytes, ar.off);
    const int nb = lay.nb;
    if (nb > 0) {
        k_stk_hist<<<nb, STK_BLOCK, 0, stream>>>(edge_index, E, N, valid_in, level, S, nb, cnt, bad);
        GSAT_LAUNCH_CHECK();
    }
    k_stk_scan<<<1, STK_SCAN_BLOCK, 0, stream>>>(cnt, nb, bad, S, N, E, cap_nodes, seg, valid_in, G, valid_out);
    GSAT_LAUNCH_CHECK();
    if (nb > 0) {
        k_stk_scatter<<<nb, STK_BLOCK, 0, stream>>>(edge_index, E, N, valid_in, level, S, nb, cnt, cap_nodes, seg, E_stack, out_edge_index,
                                                    out_edge_id);
        GSAT_LAUNCH_CHECK();
    }
    // the variants share the input's rows and graph ids where gsat_subgraph_padded's caller does: a padded input at its own node capacity
    const int share = valid_in != nullptr && cap_nodes == N;
    const int64_t items = std::max<int64_t>(std::max(E_stack, (int64_t)V * cap_nodes), 1);
    k_stk_fill<<<(unsigned)ceil_div(items, STK_BLOCK), STK_BLOCK, 0, stream>>>(valid_out, V, N, batch, share, cap_nodes, graphs_per_variant, seg,
                                                                              E_stack, out_batch, out_edge_index, out_edge_id);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

size_t gsat_fidelity_stack_multi_workspace_bytes(int64_t E, int64_t rankings, int64_t levels) {
    if (E < 0 || E >= (1ll << 31) || rankings < 1 || levels < 1 || rankings > STK_MAX_LEVELS || levels > STK_MAX_LEVELS ||
        rankings * levels > STK_MAX_LEVELS)
        return 0;
    return StkmLayout(E, rankings, levels).bytes;
}

int gsat_fidelity_stack_multi(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* batch, int64_t G, const int32_t* valid_in,
                              const uint8_t* level, int64_t rankings, int64_t levels, int64_t graphs_per_variant, int64_t cap_nodes,
                              const int64_t* segment_offsets, int64_t* out_edge_index, int64_t* out_edge_id, int64_t* out_batch,
                              int32_t* valid_out, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && N >= 0 && G >= 0 && rankings >= 1 && levels >= 1 && rankings <= STK_MAX_LEVELS && levels <= STK_MAX_LEVELS &&
                 rankings * levels <= STK_MAX_LEVELS && graphs_per_variant >= 1 && cap_nodes >= 2 && cap_nodes >= N && segment_offsets,
                 GSAT_ERR_ARG, "gsat_fidelity_stack_multi: bad argument (rankings, levels >= 1 with rankings * levels <= 16, a padding "
                 "graph, two padding nodes, node rows for every input row)");
    const int R = (int)rankings, S = (int)levels, V = 2 * R * S + 1;
    StkSegs seg;
    for (int v = 0; v <= STK_MAX_VARIANTS; ++v) seg.off[v] = segment_offsets[std::min(v, V)];
    GSAT_REQUIRE(seg.off[0] == 0, GSAT_ERR_ARG, "gsat_fidelity_stack_multi: segment_offsets must start at 0");
    for (int v = 0; v < V; ++v)
        GSAT_REQUIRE(seg.off[v + 1] >= seg.off[v], GSAT_ERR_ARG, "gsat_fidelity_stack_multi: segment_offsets must not decrease");
    const int64_t E_stack = seg.off[V];
    GSAT_REQUIRE(E < (1ll << 31) && N < (1ll << 31) && G < (1ll << 31) && E_stack < (1ll << 31) && cap_nodes < (1ll << 31) / V &&
                 graphs_per_variant < (1ll << 31) / V, GSAT_ERR_UNSUPPORTED, "gsat_fidelity_stack_multi: >2^31 entries");
    GSAT_REQUIRE(valid_out && out_batch && (N == 0 || batch) && (E == 0 || (edge_index && level)) &&
                 (E_stack == 0 || (out_edge_index && out_edge_id)), GSAT_ERR_ARG, "gsat_fidelity_stack_multi: null pointer");
    const StkmLayout lay(E, R, S);
    Arena ar(workspace, ws_bytes);
    int32_t* cnt = ar.take<int32_t>(lay.rows * (size_t)std::max(lay.nb, 1));
    int32_t* bad = ar.take<int32_t>((size_t)std::max(lay.nb, 1));
    GSAT_REQUIRE(ar.ok() && bad, GSAT_ERR_WORKSPACE, "gsat_fidelity_stack_multi: workspace %zu < %zu", ws_bytes, ar.off);
    const int nb = lay.nb;
    if (nb > 0) {
        k_stkm_hist<<<nb, STK_BLOCK, 0, stream>>>(edge_index, E, N, valid_in, level, R, S, nb, cnt, bad);
        GSAT_LAUNCH_CHECK();
    }
    k_stkm_scan<<<1, STK_SCAN_BLOCK, 0, stream>>>(cnt, nb, bad, R, S, N, E, cap_nodes, seg, valid_in, G, valid_out);
    GSAT_LAUNCH_CHECK();
    if (nb > 0) {
        k_stkm_scatter<<<nb, STK_BLOCK, 0, stream>>>(edge_index, E, N, valid_in, level, R, S, nb, cnt, cap_nodes, seg, E_stack, out_edge_index,
                                                     out_edge_id);
        GSAT_LAUNCH_CHECK();
    }
    const int share = valid_in != nullptr && cap_nodes == N;
    const int64_t items = std::max<int64_t>(std::max(E_stack, (int64_t)V * cap_nodes), 1);
    k_stk_fill<<<(unsigned)ceil_div(items, STK_BLOCK), STK_BLOCK, 0, stream>>>(valid_out, V, N, batch, share, cap_nodes, graphs_per_variant, seg,
                                                                              E_stack, out_batch, out_edge_index, out_edge_id);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_level_overlap(const uint8_t* level_a, const uint8_t* level_b, int64_t E, int64_t levels, const int32_t* valid, int64_t* acc,
                       void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && levels >= 1 && levels <= STK_MAX_LEVELS && acc, GSAT_ERR_ARG, "gsat_level_overlap: bad argument (1..16 levels)");
    GSAT_REQUIRE(E < (1ll << 31), GSAT_ERR_UNSUPPORTED, "gsat_level_overlap: >2^31 entries");
    if (E == 0) return GSAT_OK;
    GSAT_REQUIRE(level_a && level_b, GSAT_ERR_ARG, "gsat_level_overlap: null pointer");
    k_level_overlap<<<(unsigned)ceil_div(E, OVL_BLOCK * OVL_IPT), OVL_BLOCK, 0, stream>>>(level_a, level_b, E, (int)levels, valid,
                                                                                       (unsigned long long*)acc);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_level_overlap_reset(int64_t* acc, int64_t levels, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(acc && levels >= 1 && levels <= STK_MAX_LEVELS, GSAT_ERR_ARG, "gsat_level_overlap_reset: bad argument (1..16 levels)");
    k_level_overlap_reset<<<1, 64, 0, stream>>>(acc, 3 * (int)levels);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
