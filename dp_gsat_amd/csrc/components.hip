// Connectivity of explanations: connected components of every graph's kept edges at every sparsity level of a fidelity curve
// (gsat_level_components) -- replaces moving the attention to the host and a networkx / scipy loop over graphs and levels.
//
// `level` (gsat_fidelity_levels) gives for every edge the smallest level that keeps it, so the kept sets of levels 0 .. S - 1 are nested
// and one label array serves all of them: labels start as the node's own (graph-local) id, level s hooks along the edges with
// level == s only -- every older edge already lies inside one label class -- and level s + 1 goes on from the converged labels.
//
// One round = hook + shortcut (Shiloach-Vishkin with min-label hooking, the FastSV shape):
//   hook     : for a new edge (u, v) with labels a = lab[u], b = lab[v], a != b: atomicMin(&lab[max(a, b)], min(a, b)).  Labels only
//              ever decrease and lab[x] <= x, so the parent forest stays acyclic whatever the order of the atomics.
//   shortcut : lab[x] = lab[lab[x]] until nothing changes (pointer jumping: ceil(log2 n) + 1 sweeps on a path).
// Before a round every tree is a star (lab[x] is a root), so a hook that finds a != b strictly lowers the label of the root max(a, b):
// each round that is not the last one removes at least one root, and n rounds always suffice.  The fixed point -- every label the
// smallest node id of its component -- is unique, so the result does not depend on the order of the LDS atomics: integer, bitwise
// repeatable.  The loops are bounded by the node count (rounds) and by n + 1 (sweeps), so corrupt input ends them.
//
//   wave tier      : a graph of <= 64 nodes is taken by one wavefront with its labels and counters in a 1.3 KiB LDS slice of its own.
//                    The four waves of a workgroup run different trip counts: NO workgroup barrier inside this tier, only
//                    wave-level ordering (wave_sync) of the wave's own LDS traffic, and the exit votes are __ballot / __any.
//   workgroup tier : a larger graph, up to gsat_level_components_lds_cap() nodes, by the whole workgroup with the arrays in dynamic
//                    LDS; every loop leaves on a flag that __syncthreads_or hands to all threads behind the same barrier.
//
// Edges: a pre-pass validates the graph (pointer ranges, the declared bound, every loaded endpoint inside the graph's node range) and
// packs (local u, local v, level) into one word; the first slots of the graph are kept in LDS (256 per wave, 4 per node of the bound in
// the workgroup tier), the slots beyond that are packed again from L1 / L2 when read.  A graph that fails is skipped whole BEFORE
// anything indexes LDS with its ids.
#include "common.h"

namespace gsat {

constexpr int CC_BLOCK = 256;                   // 4 waves
constexpr int CC_GPB = 4;                       // consecutive graphs per workgroup: one per wave
constexpr int CC_WAVE_NODES = 64;               // wave tier: one node per lane
constexpr int CC_WAVE_EDGES = 256;              // packed edge words a wave keeps in LDS
constexpr int CC_LDS_CAP = 4096;                // nodes of the workgroup tier: 13 B per node + 16 B of edge words per node = 116 KiB of 160 KiB
constexpr int CC_EDGES_PER_NODE = 4;            // edge words kept in LDS per node of the declared bound (molecules: ~2.2 slots per node)
constexpr int CC_MAX_LEVELS = 16;
constexpr uint32_t CC_NONE = 31;                // level field of a slot that is in no level (unranked, or at or beyond valid[1])

// packed edge word: bits 0-12 local u, 13-25 local v, 26-30 level (0 .. 16, CC_NONE)
__device__ __forceinline__ uint32_t cc_pack(int u, int v, uint32_t lvl) { return (uint32_t)u | ((uint32_t)v << 13) | (lvl << 26); }
__device__ __forceinline__ int cc_u(uint32_t w) { return (int)(w & 0x1FFFu); }
__device__ __forceinline__ int cc_v(uint32_t w) { return (int)((w >> 13) & 0x1FFFu); }
__device__ __forceinline__ int cc_lvl(uint32_t w) { return (int)(w >> 26); }

// what the kernel reads of one graph, uniform over the threads that work on it
struct CcGraph {
    const int64_t* src; const int64_t* dst;     // the two rows of edge_index
    const int32_t* edge_order; const uint8_t* level;
    int E, Ev, S;                               // edge ids in [Ev, E) are never loaded
    int nlo, n, elo, ne;                        // node range [nlo, nlo + n), slot range [elo, elo + ne)
};

// slot i of the graph as a packed word; `bad` is raised for an edge id outside [0, E) or a loaded endpoint outside the node range
// (the word is then harmless: u = v = 0, in no level)
__device__ __forceinline__ uint32_t cc_load(const CcGraph& g, int i, int& bad) {
    const int e = g.edge_order[g.elo + i];
    if (e < 0 || e >= g.E) { bad = 1; return cc_pack(0, 0, CC_NONE); }
    if (e >= g.Ev) return cc_pack(0, 0, CC_NONE);
    const int64_t u = g.src[e] - g.nlo, v = g.dst[e] - g.nlo;
    if (u < 0 || u >= g.n || v < 0 || v >= g.n) { bad = 1; return cc_pack(0, 0, CC_NONE); }
    const int l = g.level[e];
    return cc_pack((int)u, (int)v, l < g.S ? (uint32_t)l : CC_NONE);
}

// slot i of a graph that passed the pre-pass: from LDS when it was kept there
__device__ __forceinline__ uint32_t cc_edge(const CcGraph& g, const uint32_t* cache, int ncache, int i) {
    if (i < ncache) return cache[i];
    int bad = 0;
    return cc_load(g, i, bad);
}

// orders the LDS traffic of ONE wave: its ds operations execute in issue order, so it is enough that the compiler keeps them in
// program order and that all lanes have issued theirs
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// the eight words a counted graph adds to acc[s]
__device__ __forceinline__ void cc_add(unsigned long long* __restrict__ acc, int s, int comps, int kept, int big_e, int touched, int big_n) {
    unsigned long long* a = acc + 8 * s;
    atomicAdd(a + 0, 1ull);
    if (comps) atomicAdd(a + 1, (unsigned long long)comps);
    if (kept) atomicAdd(a + 2, (unsigned long long)kept);
    if (big_e) atomicAdd(a + 3, (unsigned long long)big_e);
    if (touched) atomicAdd(a + 4, (unsigned long long)touched);
    if (big_n) atomicAdd(a + 5, (unsigned long long)big_n);
    if (comps == 1) atomicAdd(a + 6, 1ull);
}

__device__ __forceinline__ void cc_skip(int g, int S, int lane, int32_t* __restrict__ per_graph, unsigned long long* __restrict__ acc) {
    if (per_graph)
        for (int i = lane; i < 5 * S; i += 64) per_graph[(int64_t)g * S * 5 + i] = -1;
    if (acc && lane == 0) atomicAdd(acc + 7, 1ull);
}

// the graph's rows of the last level: labels of its nodes, and its kept slots inside the component of root `best` (-1: none)
// `stride` threads with index `t` share the graph
__device__ __forceinline__ void cc_emit(const CcGraph& g, const uint32_t* cache, int ncache, const int* lab, const uint8_t* tch, int best,
                                        int t, int stride, int32_t* __restrict__ node_comp, uint8_t* __restrict__ edge_big) {
    if (node_comp)
        for (int i = t; i < g.n; i += stride) node_comp[g.nlo + i] = tch[i] ? g.nlo + lab[i] : -1;
    if (edge_big)
        for (int i = t; i < g.ne; i += stride) {
            const int e = g.edge_order[g.elo + i];
            if (e >= g.Ev) continue;                                  // not loaded, not written (e is in [0, E): the pre-pass)
            const uint32_t w = cc_edge(g, cache, ncache, i);
            edge_big[e] = (cc_lvl(w) < g.S && lab[cc_u(w)] == best) ? 1 : 0;
        }
}

__global__ void __launch_bounds__(CC_BLOCK)
k_level_components(const int64_t* __restrict__ edge_index, int E, int N, const int32_t* __restrict__ node_ptr,
                   const int32_t* __restrict__ edge_ptr, const int32_t* __restrict__ edge_order, int G, const uint8_t* __restrict__ level,
                   int S, int bound, int cap_n, const int32_t* __restrict__ valid, int32_t* __restrict__ per_graph,
                   unsigned long long* __restrict__ acc, int32_t* __restrict__ node_comp, uint8_t* __restrict__ edge_big) {
    extern __shared__ __align__(16) unsigned char dyn[];              // workgroup tier: lab, cn, ce int[cap_n]; edge words; tch uint8[cap_n]
    __shared__ int w_lab[CC_GPB][CC_WAVE_NODES], w_cn[CC_GPB][CC_WAVE_NODES], w_ce[CC_GPB][CC_WAVE_NODES];
    __shared__ uint32_t w_edges[CC_GPB][CC_WAVE_EDGES];
    __shared__ uint8_t w_tch[CC_GPB][CC_WAVE_NODES];
    __shared__ int red[6];                                            // workgroup tier: comps, kept, touched, big_nodes, big_edges, best root

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int Gv = G, Ev = E;
    if (valid) {
        const bool spoiled = valid[3] != 0;
        Gv = spoiled ? 0 : min(max(valid[2], 0), G);
        Ev = min(max(valid[1], 0), E);
    }
    const int g0 = blockIdx.x * CC_GPB;
    CcGraph gr;
    gr.src = edge_index; gr.dst = edge_index + E; gr.edge_order = edge_order; gr.level = level; gr.E = E; gr.Ev = Ev; gr.S = S;

    // ---- wave tier: wave w takes graph g0 + w.  No __syncthreads() from here to the end of the tier. ----
    {
        const int g = g0 + wave;
        bool mine = g < Gv;
        if (mine) {
            gr.nlo = node_ptr[g]; gr.n = node_ptr[g + 1] - gr.nlo;
            gr.elo = edge_ptr[g]; gr.ne = edge_ptr[g + 1] - gr.elo;
            const bool ranges = gr.nlo >= 0 && gr.n >= 0 && gr.nlo + (int64_t)gr.n <= N && gr.elo >= 0 && gr.ne >= 0 && gr.elo + (int64_t)gr.ne <= E;
            if (ranges && gr.n > CC_WAVE_NODES) mine = false;         // the workgroup tier's, or skipped there
            else if (!ranges || gr.n > bound) { cc_skip(g, S, lane, per_graph, acc); mine = false; }
        }
        if (mine) {
            int* lab = w_lab[wave]; int* cn = w_cn[wave]; int* ce = w_ce[wave];
            uint32_t* cache = w_edges[wave]; uint8_t* tch = w_tch[wave];
            const int ncache = min(gr.ne, CC_WAVE_EDGES);
            int bad = 0;
            for (int i = lane; i < gr.ne; i += 64) {                  // pre-pass: validate every slot, keep the first ones
                const uint32_t w = cc_load(gr, i, bad);
                if (i < ncache) cache[i] = w;
            }
            lab[lane] = lane; tch[lane] = 0;
            wave_sync();
            if (__any(bad)) {
                cc_skip(g, S, lane, per_graph, acc);
            } else {
                int kept = 0, touched = 0, best = -1;
                for (int s = 0; s < S; ++s) {
                    // new edges of this level: count them, mark their ends
                    int add = 0;
                    for (int i = lane; i < gr.ne; i += 64) {
                        const uint32_t w = cc_edge(gr, cache, ncache, i);
                        if (cc_lvl(w) == s) { ++add; tch[cc_u(w)] = 1; tch[cc_v(w)] = 1; }
                    }
                    add = wave_sum(add);
                    kept += add;
                    if (add) {                                        // uniform: a level that adds nothing keeps labels and marks
                        for (int round = 0; round < gr.n; ++round) {
                            int hooked = 0;
                            for (int i = lane; i < gr.ne; i += 64) {
                                const uint32_t w = cc_edge(gr, cache, ncache, i);
                                if (cc_lvl(w) != s) continue;
                                const int a = lab[cc_u(w)], b = lab[cc_v(w)];
                                if (a != b) { atomicMin(&lab[max(a, b)], min(a, b)); hooked = 1; }
                            }
                            wave_sync();
                            if (!__any(hooked)) break;
                            for (int sweep = 0; sweep <= gr.n; ++sweep) {         // shortcut: one node per lane
                                int moved = 0;
                                if (lane < gr.n) {
                                    const int p = lab[lane], q = lab[p];
                                    if (q != p) { lab[lane] = q; moved = 1; }     // q < p: concurrent readers see a valid ancestor either way
                                }
                                wave_sync();
                                if (!__any(moved)) break;
                            }
                        }
                    }
                    // counts of this level, by root
                    cn[lane] = 0; ce[lane] = 0;
                    wave_sync();
                    const bool on = lane < gr.n && tch[lane];
                    if (on) atomicAdd(&cn[lab[lane]], 1);
                    for (int i = lane; i < gr.ne; i += 64) {
                        const uint32_t w = cc_edge(gr, cache, ncache, i);
                        if (cc_lvl(w) <= s) atomicAdd(&ce[lab[cc_u(w)]], 1);
                    }
                    wave_sync();
                    const int comps = __popcll(__ballot(on && lab[lane] == lane));
                    touched = __popcll(__ballot(on));
                    const int my_n = lane < gr.n ? cn[lane] : 0, my_e = lane < gr.n ? ce[lane] : 0;
                    const int big_n = wave_max(my_n), big_e = wave_max(my_e);
                    if (s == S - 1) {                                 // largest component by kept slots, ties to the smaller label
                        const uint64_t m = __ballot(lane < gr.n && big_e > 0 && my_e == big_e);
                        best = m ? __ffsll((unsigned long long)m) - 1 : -1;
                    }
                    if (lane == 0) {
                        if (per_graph) {
                            int32_t* row = per_graph + ((int64_t)g * S + s) * 5;
                            row[0] = comps; row[1] = kept; row[2] = big_e; row[3] = touched; row[4] = big_n;
                        }
                        if (acc) cc_add(acc, s, comps, kept, big_e, touched, big_n);
                    }
                    wave_sync();                                      // the counters are zeroed again at the next level
                }
                cc_emit(gr, cache, ncache, lab, tch, best, lane, 64, node_comp, edge_big);
            }
        }
    }

    // ---- workgroup tier: the graphs of this workgroup with more than 64 nodes, one after the other.  Every condition up to a barrier
    //      is uniform over the workgroup (it depends on g and on values every thread reads alike). ----
    int* lab = reinterpret_cast<int*>(dyn);
    int* cn = lab + cap_n;
    int* ce = cn + cap_n;
    uint32_t* cache = reinterpret_cast<uint32_t*>(ce + cap_n);
    uint8_t* tch = reinterpret_cast<uint8_t*>(cache + (size_t)CC_EDGES_PER_NODE * cap_n);
    for (int w0 = 0; w0 < CC_GPB; ++w0) {
        const int g = g0 + w0;
        if (g >= Gv) break;
        gr.nlo = node_ptr[g]; gr.n = node_ptr[g + 1] - gr.nlo;
        gr.elo = edge_ptr[g]; gr.ne = edge_ptr[g + 1] - gr.elo;
        const bool ranges = gr.nlo >= 0 && gr.n >= 0 && gr.nlo + (int64_t)gr.n <= N && gr.elo >= 0 && gr.ne >= 0 && gr.elo + (int64_t)gr.ne <= E;
        if (!ranges || gr.n <= CC_WAVE_NODES) continue;              // the wave tier's (it also marks bad ranges)
        if (gr.n > bound) {                                           // larger than the declared bound (<= cap_n): skipped whole, LDS untouched
            if (wave == 0) cc_skip(g, S, lane, per_graph, acc);
            continue;
        }
        __syncthreads();                                              // the previous graph's readers of the arrays are done
        const int ncache = min(gr.ne, CC_EDGES_PER_NODE * cap_n);
        int bad = 0;
        for (int i = threadIdx.x; i < gr.ne; i += CC_BLOCK) {
            const uint32_t w = cc_load(gr, i, bad);
            if (i < ncache) cache[i] = w;
        }
        for (int i = threadIdx.x; i < gr.n; i += CC_BLOCK) { lab[i] = i; tch[i] = 0; }
        if (__syncthreads_or(bad)) {
            if (wave == 0) cc_skip(g, S, lane, per_graph, acc);
            continue;
        }
        int kept = 0, best = -1;
        for (int s = 0; s < S; ++s) {
            int add = 0;
            for (int i = threadIdx.x; i < gr.ne; i += CC_BLOCK) {
                const uint32_t w = cc_edge(gr, cache, ncache, i);
                if (cc_lvl(w) == s) { ++add; tch[cc_u(w)] = 1; tch[cc_v(w)] = 1; }
            }
            if (threadIdx.x < 6) red[threadIdx.x] = threadIdx.x < 5 ? 0 : gr.n;
            const bool any_new = __syncthreads_or(add) != 0;
            if (any_new) {
                for (int round = 0; round < gr.n; ++round) {
                    int hooked = 0;
                    for (int i = threadIdx.x; i < gr.ne; i += CC_BLOCK) {
                        const uint32_t w = cc_edge(gr, cache, ncache, i);
                        if (cc_lvl(w) != s) continue;
                        const int a = lab[cc_u(w)], b = lab[cc_v(w)];
                        if (a != b) { atomicMin(&lab[max(a, b)], min(a, b)); hooked = 1; }
                    }
                    if (!__syncthreads_or(hooked)) break;             // the flag every thread reads behind the same barrier
                    for (int sweep = 0; sweep <= gr.n; ++sweep) {
                        int moved = 0;
                        for (int i = threadIdx.x; i < gr.n; i += CC_BLOCK) {
                            const int p = lab[i], q = lab[p];
                            if (q != p) { lab[i] = q; moved = 1; }
                        }
                        if (!__syncthreads_or(moved)) break;
                    }
                }
            }
            for (int i = threadIdx.x; i < gr.n; i += CC_BLOCK) { cn[i] = 0; ce[i] = 0; }
            __syncthreads();
            int comps = 0, touched = 0;
            for (int i = threadIdx.x; i < gr.n; i += CC_BLOCK)
                if (tch[i]) { ++touched; comps += lab[i] == i; atomicAdd(&cn[lab[i]], 1); }
            for (int i = threadIdx.x; i < gr.ne; i += CC_BLOCK) {
                const uint32_t w = cc_edge(gr, cache, ncache, i);
                if (cc_lvl(w) <= s) atomicAdd(&ce[lab[cc_u(w)]], 1);
            }
            comps = wave_sum(comps); touched = wave_sum(touched); add = wave_sum(add);
            if (lane == 0) { atomicAdd(&red[0], comps); atomicAdd(&red[1], add); atomicAdd(&red[2], touched); }
            __syncthreads();
            int big_n = 0, big_e = 0;
            for (int i = threadIdx.x; i < gr.n; i += CC_BLOCK) { big_n = max(big_n, cn[i]); big_e = max(big_e, ce[i]); }
            big_n = wave_max(big_n); big_e = wave_max(big_e);
            if (lane == 0) { atomicMax(&red[3], big_n); atomicMax(&red[4], big_e); }
            __syncthreads();
            kept += red[1];
            comps = red[0]; touched = red[2]; big_n = red[3]; big_e = red[4];
            if (s == S - 1 && big_e > 0) {                            // smallest root whose component holds big_e kept slots
                int first = gr.n;
                for (int i = threadIdx.x; i < gr.n; i += CC_BLOCK)
                    if (ce[i] == big_e) { first = i; break; }         // a thread's indices ascend: its first hit is its smallest
                first = -wave_max(-first);
                if (lane == 0) atomicMin(&red[5], first);
                __syncthreads();
                best = red[5];
            }
            if (threadIdx.x == 0) {
                if (per_graph) {
                    int32_t* row = per_graph + ((int64_t)g * S + s) * 5;
                    row[0] = comps; row[1] = kept; row[2] = big_e; row[3] = touched; row[4] = big_n;
                }
                if (acc) cc_add(acc, s, comps, kept, big_e, touched, big_n);
            }
            __syncthreads();                                          // red and the counters are rewritten at the next level
        }
        cc_emit(gr, cache, ncache, lab, tch, best, threadIdx.x, CC_BLOCK, node_comp, edge_big);
    }
}

__global__ void k_level_components_reset(int64_t* __restrict__ acc, int n) {
    if (blockIdx.x == 0 && (int)threadIdx.x < n) acc[threadIdx.x] = 0;
}

}  // namespace gsat

using namespace gsat;

extern "C" {

int64_t gsat_level_components_lds_cap(void) { return CC_LDS_CAP; }
int64_t gsat_level_components_wave_nodes(void) { return CC_WAVE_NODES; }

int gsat_level_components(const int64_t* edge_index, int64_t E, int64_t N, const int32_t* node_ptr, const int32_t* edge_ptr,
                          const int32_t* edge_order, int64_t G, const uint8_t* level, int64_t levels, int64_t max_seg_nodes,
                          const int32_t* valid, int32_t* per_graph, int64_t* acc, int32_t* node_comp, uint8_t* edge_big, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && N >= 0 && G >= 0 && levels >= 1 && levels <= CC_MAX_LEVELS, GSAT_ERR_ARG,
                 "gsat_level_components: bad argument (1..16 levels)");
    GSAT_REQUIRE(E < (1ll << 31) && N < (1ll << 31) && G < (1ll << 31), GSAT_ERR_UNSUPPORTED, "gsat_level_components: >2^31 entries");
    GSAT_REQUIRE(max_seg_nodes >= 0 && max_seg_nodes <= CC_LDS_CAP, GSAT_ERR_ARG,
                 "gsat_level_components: max_seg_nodes = %lld (cap %d, -1 = unknown): the largest graph must be declared and fit LDS",
                 (long long)max_seg_nodes, CC_LDS_CAP);
    if (G == 0) return GSAT_OK;
    GSAT_REQUIRE(node_ptr && edge_ptr && (E == 0 || (edge_index && edge_order && level)), GSAT_ERR_ARG, "gsat_level_components: null pointer");
    int cap_n = 0;
    if (max_seg_nodes > CC_WAVE_NODES) cap_n = (int)((max_seg_nodes + 63) / 64 * 64);
    const size_t lds_bytes = (size_t)cap_n * (3 * sizeof(int) + CC_EDGES_PER_NODE * sizeof(uint32_t) + 1);
    if (lds_bytes > 32 * 1024)                  // with the static slices above the default dynamic-LDS limit: raised on the current device
        GSAT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_level_components), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           CC_LDS_CAP * (int)(3 * sizeof(int) + CC_EDGES_PER_NODE * sizeof(uint32_t) + 1)));
    k_level_components<<<(unsigned)ceil_div(G, CC_GPB), CC_BLOCK, lds_bytes, stream>>>(
        edge_index, (int)E, (int)N, node_ptr, edge_ptr, edge_order, (int)G, level, (int)levels, (int)max_seg_nodes, cap_n, valid, per_graph,
        reinterpret_cast<unsigned long long*>(acc), node_comp, edge_big);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_level_components_reset(int64_t* acc, int64_t levels, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(acc && levels >= 1 && levels <= CC_MAX_LEVELS, GSAT_ERR_ARG, "gsat_level_components_reset: bad argument (1..16 levels)");
    k_level_components_reset<<<1, 128, 0, stream>>>(acc, 8 * (int)levels);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
