// Explanation subgraphs on the device: order-preserving stream compaction of a collated batch's nodes and edges with node
// relabelling (PyG subgraph(..., relabel_nodes=True) / the edge-mask counterpart), and a row gather for the attributes that ride
// along (replaces the host-side subgraph() of example/trainer.py:140-170).
//
// Kept items stay in their original relative order, so every output is unique: new node id = number of kept nodes with a smaller
// old id; kept edges ascending by old edge id.  Integer work only.
//
// Two-level scan, no inter-workgroup waiting: every workgroup owns SUB_ITEMS consecutive items (8 per thread), ranks them with
// wave64 ballots and writes ONE count; a single workgroup scans the counts (and writes `counts`); the output passes redo the
// in-workgroup ranks on top of their workgroup's offset.
//
//   edge mode, all nodes kept / node mode : flags (nodes and edges in one launch) -> scan -> node outputs -> edge outputs     (4)
//   edge mode, isolated nodes dropped     : clear marks -> edge flags + endpoint marks -> node counts -> scan -> node outputs
//                                           -> edge outputs                                                                 (6)
// The endpoint marks are byte stores of the value 1 (they race only with identical values); nothing is cleared by a memset node.
//
// gsat_subgraph_padded: the same passes into outputs of a CAPACITY shape -- the flags pass reads the counted nodes / edges of a padded
// input from its valid word, the scan writes valid_out = (N', E', graphs, overflow), the two output passes emit the real part and one
// more pass (k_subp_fill) turns the slack into the padding graph by the rule of gsat_collate_padded.  5 launches (7), no size read back.
#include "common.h"
#include "compact.h"
#include <algorithm>

namespace gsat {

constexpr int SUB_BLOCK = 256;                  // 4 waves
constexpr int SUB_IPT = 8;                      // consecutive items per thread: 8-byte flag loads, 16-byte id loads, 2 x 16-byte rank stores
constexpr int SUB_ITEMS = SUB_BLOCK * SUB_IPT;  // items per workgroup
constexpr int SUB_SCAN_BLOCK = 1024;

// bit j = flag[i0 + j] != 0 (0 beyond n); i0 is a multiple of SUB_IPT
__device__ __forceinline__ uint32_t load_flags8(const uint8_t* __restrict__ p, int64_t i0, int64_t n) {
    uint32_t bits = 0;
    if (i0 + SUB_IPT <= n && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
        const uint2 v = *reinterpret_cast<const uint2*>(p + i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bits |= ((v.x >> (8 * j)) & 0xFFu) ? (1u << j) : 0u;
            bits |= ((v.y >> (8 * j)) & 0xFFu) ? (16u << j) : 0u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < SUB_IPT; ++j)
            if (i0 + j < n && p[i0 + j] != 0) bits |= 1u << j;
    }
    return bits;
}

// flag[i0 + j] = bit j as 0 / 1, for the items below n
__device__ __forceinline__ void store_flags8(uint8_t* __restrict__ p, int64_t i0, int64_t n, uint32_t bits) {
    if (i0 + SUB_IPT <= n && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
        uint2 v = make_uint2(0u, 0u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v.x |= ((bits >> j) & 1u) << (8 * j);
            v.y |= ((bits >> (4 + j)) & 1u) << (8 * j);
        }
        *reinterpret_cast<uint2*>(p + i0) = v;
    } else {
#pragma unroll
        for (int j = 0; j < SUB_IPT; ++j)
            if (i0 + j < n) p[i0 + j] = (uint8_t)((bits >> j) & 1u);
    }
}

// v[j] = p[i0 + j] (0 beyond n): four 16-byte loads when the row is 16-byte aligned
__device__ __forceinline__ void load_ids8(const int64_t* __restrict__ p, int64_t i0, int64_t n, int64_t v[SUB_IPT]) {
    if (i0 + SUB_IPT <= n && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
        for (int j = 0; j < SUB_IPT; j += 2) {
            const longlong2 t = *reinterpret_cast<const longlong2*>(p + i0 + j);
            v[j] = t.x; v[j + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < SUB_IPT; ++j) v[j] = i0 + j < n ? p[i0 + j] : 0;
    }
}

__global__ void __launch_bounds__(SUB_BLOCK) k_sub_clear(uint4* __restrict__ p, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * SUB_BLOCK + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// Workgroups [0, nb_nodes): node flags and counts.  node_src = the caller's node_keep (node mode), the endpoint marks (edge mode with
// isolated nodes dropped; then node_src == node_flag and nothing is rewritten) or null (every node kept).
// Workgroups [nb_nodes, ...): edge flags and counts.  Edge mode: flag = edge_keep != 0; node mode: both endpoints kept.  An edge with an
// id outside [0, Nv) is dropped and reported in bad[workgroup]; `mark` (edge mode, drop_isolated) receives a 1 at both endpoints.
// N / E are the arrays' extents, Nv <= N / Ev <= E the counted items: a node row >= Nv or an edge slot >= Ev gets flag 0 and its keep
// entry is never read (a padded input; otherwise Nv == N, Ev == E).
__device__ __forceinline__ void sub_flags(const int64_t* __restrict__ ei, int64_t E, int64_t N, int64_t Ev, int64_t Nv,
                                          const uint8_t* __restrict__ edge_keep, const uint8_t* __restrict__ node_keep,
                                          const uint8_t* node_src, uint8_t* node_flag, uint8_t* mark, int nb_nodes,
                                          uint8_t* __restrict__ edge_mask, int32_t* __restrict__ cnt_n, int32_t* __restrict__ cnt_e,
                                          int32_t* __restrict__ bad, int* sh) {
    int total;
    if ((int)blockIdx.x < nb_nodes) {
        const int64_t i0 = (int64_t)blockIdx.x * SUB_ITEMS + (int64_t)threadIdx.x * SUB_IPT;
        uint32_t bits;
        if (node_src) {
            bits = load_flags8(node_src, i0, Nv);
        } else {
            const int64_t left = Nv - i0;
            bits = left >= SUB_IPT ? 0xFFu : (left > 0 ? (1u << left) - 1u : 0u);
        }
        if (node_src != node_flag) store_flags8(node_flag, i0, N, bits);
        (void)block_rank<SUB_IPT, SUB_BLOCK>(bits, sh, total);
        if (threadIdx.x == 0) cnt_n[blockIdx.x] = total;
        return;
    }
    const int b = (int)blockIdx.x - nb_nodes;
    const int64_t i0 = (int64_t)b * SUB_ITEMS + (int64_t)threadIdx.x * SUB_IPT;
    int64_t s[SUB_IPT], d[SUB_IPT];
    load_ids8(ei, i0, E, s);
    load_ids8(ei + E, i0, E, d);
    const uint32_t want = edge_keep ? load_flags8(edge_keep, i0, Ev) : 0xFFu;
    uint32_t bits = 0;
    int any_bad = 0;
#pragma unroll
    for (int j = 0; j < SUB_IPT; ++j) {
        if (i0 + j >= Ev) continue;
        const bool in_range = (uint64_t)s[j] < (uint64_t)Nv && (uint64_t)d[j] < (uint64_t)Nv;
        any_bad |= in_range ? 0 : 1;
        bool k = in_range && ((want >> j) & 1u);
        if (k && node_keep) k = node_keep[s[j]] != 0 && node_keep[d[j]] != 0;
        if (k) {
            bits |= 1u << j;
            if (mark) { mark[s[j]] = 1; mark[d[j]] = 1; }
        }
    }
    store_flags8(edge_mask, i0, E, bits);
    (void)block_rank<SUB_IPT, SUB_BLOCK>(bits, sh, total);
    any_bad = __syncthreads_or(any_bad);
    if (threadIdx.x == 0) { cnt_e[b] = total; bad[b] = any_bad ? 1 : 0; }
}

__global__ void __launch_bounds__(SUB_BLOCK)
k_sub_flags(const int64_t* __restrict__ ei, int64_t E, int64_t N, const uint8_t* __restrict__ edge_keep, const uint8_t* __restrict__ node_keep,
            const uint8_t* node_src, uint8_t* node_flag, uint8_t* mark, int nb_nodes, uint8_t* __restrict__ edge_mask,
            int32_t* __restrict__ cnt_n, int32_t* __restrict__ cnt_e, int32_t* __restrict__ bad) {
    __shared__ int sh[SUB_BLOCK / 64];
    sub_flags(ei, E, N, E, N, edge_keep, node_keep, node_src, node_flag, mark, nb_nodes, edge_mask, cnt_n, cnt_e, bad, sh);
}

// The counts of a padded input: (N_real, E_real) of its valid word, clamped to the arrays; nothing of an input that overflowed.
__device__ __forceinline__ void valid_counts(const int32_t* __restrict__ valid_in, int64_t N, int64_t E, int64_t& Nv, int64_t& Ev) {
    Nv = N; Ev = E;
    if (valid_in) {
        const bool spoiled = valid_in[3] != 0;
        Nv = spoiled ? 0 : min<int64_t>(max<int64_t>(valid_in[0], 0), N);
        Ev = spoiled ? 0 : min<int64_t>(max<int64_t>(valid_in[1], 0), E);
    }
}

// k_sub_flags with the counted nodes / edges read from valid_in (int32[4], nullable) on the device
__global__ void __launch_bounds__(SUB_BLOCK)
k_subp_flags(const int64_t* __restrict__ ei, int64_t E, int64_t N, const int32_t* __restrict__ valid_in, const uint8_t* __restrict__ edge_keep,
             const uint8_t* __restrict__ node_keep, const uint8_t* node_src, uint8_t* node_flag, uint8_t* mark, int nb_nodes,
             uint8_t* __restrict__ edge_mask, int32_t* __restrict__ cnt_n, int32_t* __restrict__ cnt_e, int32_t* __restrict__ bad) {
    __shared__ int sh[SUB_BLOCK / 64];
    int64_t Nv, Ev;
    valid_counts(valid_in, N, E, Nv, Ev);
    sub_flags(ei, E, N, Ev, Nv, edge_keep, node_keep, node_src, node_flag, mark, nb_nodes, edge_mask, cnt_n, cnt_e, bad, sh);
}

// second scan level: workgroup counts -> workgroup offsets (the totals behind them), and counts = (N', E', overflow, bad id)
__global__ void __launch_bounds__(SUB_SCAN_BLOCK)
k_sub_scan(int32_t* __restrict__ cnt_n, int nb_nodes, int32_t* __restrict__ cnt_e, int nb_edges, const int32_t* __restrict__ bad,
           int64_t cap_nodes, int64_t cap_edges, int exact, int64_t* __restrict__ counts) {
    __shared__ int sh[SUB_SCAN_BLOCK / 64];
    const int kept_n = scan_counts<SUB_SCAN_BLOCK>(cnt_n, nb_nodes, sh);
    const int kept_e = scan_counts<SUB_SCAN_BLOCK>(cnt_e, nb_edges, sh);
    int any_bad = 0;
    for (int i = threadIdx.x; i < nb_edges; i += SUB_SCAN_BLOCK) any_bad |= bad[i];
    any_bad = __syncthreads_or(any_bad);
    if (threadIdx.x == 0) {
        cnt_n[nb_nodes] = kept_n;
        cnt_e[nb_edges] = kept_e;
        bool over = false;                       // a capacity of -1: not declared (the counting phase of a two-phase call)
        if (cap_nodes >= 0) over = over || (exact ? kept_n != cap_nodes : kept_n > cap_nodes);
        if (cap_edges >= 0) over = over || (exact ? kept_e != cap_edges : kept_e > cap_edges);
        counts[0] = kept_n;
        counts[1] = kept_e;
        counts[2] = over ? 1 : 0;
        counts[3] = any_bad ? 1 : 0;
    }
}

// node_rank[i] = kept nodes below i for EVERY node (node_rank[N] = N'), node_id / new_batch at the kept nodes' ranks below cap_nodes
__global__ void __launch_bounds__(SUB_BLOCK)
k_sub_node_out(const uint8_t* __restrict__ node_flag, int64_t N, const int32_t* __restrict__ off_n, int nb_nodes,
               const int64_t* __restrict__ batch, int64_t cap_nodes, int64_t* __restrict__ node_id, int64_t* __restrict__ new_batch,
               int32_t* __restrict__ node_rank) {
    __shared__ int sh[SUB_BLOCK / 64];
    const int b = blockIdx.x;
    const int64_t i0 = (int64_t)b * SUB_ITEMS + (int64_t)threadIdx.x * SUB_IPT;
    const uint32_t bits = b < nb_nodes ? load_flags8(node_flag, i0, N) : 0u;
    int total;
    const int first = off_n[b < nb_nodes ? b : nb_nodes] + block_rank<SUB_IPT, SUB_BLOCK>(bits, sh, total);
    int r[SUB_IPT];
#pragma unroll
    for (int j = 0; j < SUB_IPT; ++j) r[j] = first + __popc(bits & ((1u << j) - 1u));
    if (i0 + SUB_IPT <= N) {                     // node_rank is workspace: 256-byte aligned, i0 a multiple of 8
        int4* q = reinterpret_cast<int4*>(node_rank + i0);
        q[0] = make_int4(r[0], r[1], r[2], r[3]);
        q[1] = make_int4(r[4], r[5], r[6], r[7]);
    } else {
#pragma unroll
        for (int j = 0; j < SUB_IPT; ++j)
            if (i0 + j < N) node_rank[i0 + j] = r[j];
    }
#pragma unroll
    for (int j = 0; j < SUB_IPT; ++j) {
        if (((bits >> j) & 1u) && (int64_t)r[j] < cap_nodes) {
            node_id[r[j]] = i0 + j;
            if (batch) new_batch[r[j]] = batch[i0 + j];
        }
    }
    const int64_t kept = off_n[nb_nodes];
    if (b == (int)gridDim.x - 1 && threadIdx.x == 0) node_rank[N] = (int32_t)kept;
    // a declared capacity above the true count (reported in counts[2]): the tail holds valid ids, never uninitialised memory
    for (int64_t p = kept + (int64_t)b * SUB_BLOCK + threadIdx.x; p < cap_nodes; p += (int64_t)gridDim.x * SUB_BLOCK) {
        node_id[p] = 0;
        if (batch) new_batch[p] = 0;
    }
}

// Workgroups [0, nb_edges): edge_id and the relabelled edge_index (rows of cap_edges entries) at the kept edges' ranks below cap_edges.
// Workgroups behind them: new_node_ptr[g] = node_rank[node_ptr[g]], the exclusive node scan read at the old segment starts.
__global__ void __launch_bounds__(SUB_BLOCK)
k_sub_edge_out(const int64_t* __restrict__ ei, int64_t E, int64_t N, const uint8_t* __restrict__ edge_mask, const int32_t* __restrict__ off_e,
               int nb_edges, const int32_t* __restrict__ node_rank, int64_t cap_edges, int64_t* __restrict__ edge_id,
               int64_t* __restrict__ new_ei, const int32_t* __restrict__ node_ptr, int64_t G, int32_t* __restrict__ new_node_ptr) {
    __shared__ int sh[SUB_BLOCK / 64];
    const int b = blockIdx.x;
    if (b >= nb_edges) {
        const int64_t g = (int64_t)(b - nb_edges) * SUB_BLOCK + threadIdx.x;
        if (g <= G) {
            int64_t p = node_ptr[g];
            p = p < 0 ? 0 : (p > N ? N : p);
            new_node_ptr[g] = node_rank[p];
        }
        return;
    }
    const int64_t i0 = (int64_t)b * SUB_ITEMS + (int64_t)threadIdx.x * SUB_IPT;
    const uint32_t bits = load_flags8(edge_mask, i0, E);
    int total;
    const int first = off_e[b] + block_rank<SUB_IPT, SUB_BLOCK>(bits, sh, total);
    int64_t s[SUB_IPT], d[SUB_IPT];
    load_ids8(ei, i0, E, s);
    load_ids8(ei + E, i0, E, d);
#pragma unroll
    for (int j = 0; j < SUB_IPT; ++j) {
        const int64_t pos = first + __popc(bits & ((1u << j) - 1u));
        if (((bits >> j) & 1u) && pos < cap_edges && (uint64_t)s[j] < (uint64_t)N && (uint64_t)d[j] < (uint64_t)N) {
            edge_id[pos] = i0 + j;
            new_ei[pos] = node_rank[s[j]];
            new_ei[cap_edges + pos] = node_rank[d[j]];
        }
    }
    for (int64_t p = off_e[nb_edges] + (int64_t)b * SUB_BLOCK + threadIdx.x; p < cap_edges; p += (int64_t)nb_edges * SUB_BLOCK) {
        edge_id[p] = 0;                          // as in k_sub_node_out: a valid id behind the true count
        new_ei[p] = 0;
        new_ei[cap_edges + p] = 0;
    }
}

// k_sub_scan for a padded result: the workgroup offsets and valid_out = (N', E', graphs, overflow).  The result
// overflows when fewer than two padding nodes would remain, the edges do not fit, the input had overflowed or an edge had a bad id:
// valid_out = (0, 0, 0, 1) and k_subp_fill makes every row and slot padding.
__global__ void __launch_bounds__(SUB_SCAN_BLOCK)
k_subp_scan(int32_t* __restrict__ cnt_n, int nb_nodes, int32_t* __restrict__ cnt_e, int nb_edges, const int32_t* __restrict__ bad,
            int64_t cap_nodes, int64_t cap_edges, const int32_t* __restrict__ valid_in, int64_t G, int32_t* __restrict__ valid_out) {
    __shared__ int sh[SUB_SCAN_BLOCK / 64];
    const int kept_n = scan_counts<SUB_SCAN_BLOCK>(cnt_n, nb_nodes, sh);
    const int kept_e = scan_counts<SUB_SCAN_BLOCK>(cnt_e, nb_edges, sh);
    int any_bad = 0;
    for (int i = threadIdx.x; i < nb_edges; i += SUB_SCAN_BLOCK) any_bad |= bad[i];
    any_bad = __syncthreads_or(any_bad);
    if (threadIdx.x == 0) {
        // the entry behind the offsets is where k_sub_node_out / k_sub_edge_out start their filler (valid ids behind the true count);
        // here k_subp_fill owns everything behind the counts, so the start is put at the capacity and that loop writes nothing
        cnt_n[nb_nodes] = (int32_t)cap_nodes;
        cnt_e[nb_edges] = (int32_t)cap_edges;
        const bool over = (int64_t)kept_n + 2 > cap_nodes || (int64_t)kept_e > cap_edges || any_bad || (valid_in && valid_in[3] != 0);
        valid_out[0] = over ? 0 : kept_n;
        valid_out[1] = over ? 0 : kept_e;
        valid_out[2] = over ? 0 : (valid_in ? valid_in[2] : (int32_t)G);
        valid_out[3] = over ? 1 : 0;
    }
}

// The slack of a padded result, in the style of k_collate_padded: thread i takes node row i and edge slot i and reads the counts from
// valid_out.  Rows >= N' become padding nodes (graph pad_graph, node_id -1), slots >= E' padding edges among them (edge_id -1).
__global__ void k_subp_fill(const int32_t* __restrict__ valid_out, int64_t cap_nodes, int64_t cap_edges, int64_t pad_graph,
                            int64_t* __restrict__ node_id, int64_t* __restrict__ new_batch, int64_t* __restrict__ edge_id,
                            int64_t* __restrict__ new_ei) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = valid_out[0], E = valid_out[1];
    if (i < cap_nodes && i >= N) {
        node_id[i] = -1;
        if (new_batch) new_batch[i] = pad_graph;
    }
    if (i < cap_edges && i >= E) {
        int64_t src, dst;
        padding_edge(N, cap_nodes - N, cap_edges - E, i - E, src, dst);
        edge_id[i] = -1;
        new_ei[i] = src;
        new_ei[cap_edges + i] = dst;
    }
}

// out unit u = table unit index[u / U] * U + u % U, a unit being one T (16, 8, 4 or 1 bytes) and U the units per row
template <class T, class I>
__global__ void __launch_bounds__(256) k_gather_rows(const T* __restrict__ table, const int64_t* __restrict__ index, I total, I U,
                                                    T* __restrict__ out) {
    const I step = (I)gridDim.x * 256;
    for (I u = (I)blockIdx.x * 256 + threadIdx.x; u < total; u += step) {
        const I r = u / U, c = u - r * U;
        out[u] = table[index[r] * (int64_t)U + (int64_t)c];
    }
}

template <class T>
static void launch_gather(const void* table, const int64_t* index, int64_t n, int64_t row_bytes, void* out, hipStream_t stream) {
    const int64_t U = row_bytes / (int64_t)sizeof(T), total = n * U;
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(total, 256), 8192);
    if (total < (1ll << 31))
        k_gather_rows<T, uint32_t><<<blocks, 256, 0, stream>>>(static_cast<const T*>(table), index, (uint32_t)total, (uint32_t)U, static_cast<T*>(out));
    else
        k_gather_rows<T, int64_t><<<blocks, 256, 0, stream>>>(static_cast<const T*>(table), index, total, U, static_cast<T*>(out));
}

struct SubLayout {
    size_t flag_bytes, bytes;
    int nb_nodes, nb_edges;
    SubLayout(int64_t N, int64_t E) {
        nb_nodes = (int)ceil_div(N, SUB_ITEMS);
        nb_edges = (int)ceil_div(E, SUB_ITEMS);
        flag_bytes = align_up((size_t)(N > 0 ? N : 1), 256);
        bytes = 256 + flag_bytes + align_up((size_t)(N + 1) * 4, 256) + align_up((size_t)(nb_nodes + 1) * 4, 256) +
                2 * align_up((size_t)(nb_edges + 1) * 4, 256);
    }
};

}  // namespace gsat

using namespace gsat;

extern "C" {

int64_t gsat_subgraph_block_items(void) { return SUB_ITEMS; }

size_t gsat_subgraph_workspace_bytes(int64_t N, int64_t E) {
    if (N < 0 || E < 0 || N >= (1ll << 31) || E >= (1ll << 31)) return 0;
    return SubLayout(N, E).bytes;
}

int gsat_subgraph_index(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* batch, const int32_t* node_ptr, int64_t G,
                        const uint8_t* keep, int mode, int drop_isolated, int phases, int64_t cap_nodes, int64_t cap_edges, int exact,
                        int64_t* node_id, int64_t* edge_id, int64_t* new_edge_index, int64_t* new_batch, int32_t* new_node_ptr,
                        uint8_t* edge_mask, int64_t* counts, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && N >= 0 && G >= 0 && (mode == 0 || mode == 1) && phases >= 1 && phases <= 3 && cap_nodes >= -1 && cap_edges >= -1,
                 GSAT_ERR_ARG, "gsat_subgraph_index: bad argument");
    GSAT_REQUIRE(N < (1ll << 31) && E < (1ll << 31) && G < (1ll << 31), GSAT_ERR_UNSUPPORTED, "gsat_subgraph_index: >2^31 entries");
    const bool count = (phases & 1) != 0, emit = (phases & 2) != 0;
    GSAT_REQUIRE(!emit || (cap_nodes >= 0 && cap_edges >= 0), GSAT_ERR_ARG, "gsat_subgraph_index: the output phase needs both capacities");
    GSAT_REQUIRE(cap_nodes <= N && cap_edges <= E, GSAT_ERR_ARG, "gsat_subgraph_index: a capacity above the input's size");
    GSAT_REQUIRE(counts && (E == 0 || (edge_index && edge_mask)) && (mode == 0 ? (E == 0 || keep) : (N == 0 || keep)), GSAT_ERR_ARG,
                 "gsat_subgraph_index: null pointer");
    GSAT_REQUIRE(!emit || ((cap_nodes == 0 || (node_id && (!batch || new_batch))) && (cap_edges == 0 || (edge_id && new_edge_index)) &&
                           (!node_ptr || new_node_ptr)),
                 GSAT_ERR_ARG, "gsat_subgraph_index: null output");
    const SubLayout lay(N, E);
    Arena ar(workspace, ws_bytes);
    uint8_t* node_flag = ar.take<uint8_t>(lay.flag_bytes);
    int32_t* node_rank = ar.take<int32_t>((size_t)N + 1);
    int32_t* cnt_n = ar.take<int32_t>((size_t)lay.nb_nodes + 1);
    int32_t* cnt_e = ar.take<int32_t>((size_t)lay.nb_edges + 1);
    int32_t* bad = ar.take<int32_t>((size_t)lay.nb_edges + 1);
    GSAT_REQUIRE(ar.ok() && bad, GSAT_ERR_WORKSPACE, "gsat_subgraph_index: workspace %zu < %zu", ws_bytes, ar.off);
    const int nbn = lay.nb_nodes, nbe = lay.nb_edges;
    if (count) {
        if (mode == 0 && drop_isolated) {
            if (N > 0) {
                const int64_t n16 = (int64_t)(lay.flag_bytes / 16);
                k_sub_clear<<<(unsigned)ceil_div(n16, SUB_BLOCK), SUB_BLOCK, 0, stream>>>(reinterpret_cast<uint4*>(node_flag), n16);
                GSAT_LAUNCH_CHECK();
            }
            if (nbe > 0) {
                k_sub_flags<<<nbe, SUB_BLOCK, 0, stream>>>(edge_index, E, N, keep, nullptr, nullptr, nullptr, node_flag, 0, edge_mask, cnt_n,
                                                           cnt_e, bad);
                GSAT_LAUNCH_CHECK();
            }
            if (nbn > 0) {
                k_sub_flags<<<nbn, SUB_BLOCK, 0, stream>>>(edge_index, E, N, nullptr, nullptr, node_flag, node_flag, nullptr, nbn, edge_mask,
                                                           cnt_n, cnt_e, bad);
                GSAT_LAUNCH_CHECK();
            }
        } else if (nbn + nbe > 0) {
            const uint8_t* node_keep = mode == 1 ? keep : nullptr;
            k_sub_flags<<<nbn + nbe, SUB_BLOCK, 0, stream>>>(edge_index, E, N, mode == 0 ? keep : nullptr, node_keep, node_keep, node_flag,
                                                             nullptr, nbn, edge_mask, cnt_n, cnt_e, bad);
            GSAT_LAUNCH_CHECK();
        }
        k_sub_scan<<<1, SUB_SCAN_BLOCK, 0, stream>>>(cnt_n, nbn, cnt_e, nbe, bad, cap_nodes, cap_edges, exact, counts);
        GSAT_LAUNCH_CHECK();
    }
    if (emit) {
        k_sub_node_out<<<std::max(nbn, 1), SUB_BLOCK, 0, stream>>>(node_flag, N, cnt_n, nbn, batch, cap_nodes, node_id, new_batch, node_rank);
        GSAT_LAUNCH_CHECK();
        const int nbg = node_ptr ? (int)ceil_div(G + 1, SUB_BLOCK) : 0;
        if (nbe + nbg > 0) {
            k_sub_edge_out<<<nbe + nbg, SUB_BLOCK, 0, stream>>>(edge_index, E, N, edge_mask, cnt_e, nbe, node_rank, cap_edges, edge_id,
                                                                new_edge_index, node_ptr, G, new_node_ptr);
            GSAT_LAUNCH_CHECK();
        }
    }
    return GSAT_OK;
}

int gsat_subgraph_padded(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* batch, int64_t G, const uint8_t* keep, int mode,
                         int drop_isolated, const int32_t* valid_in, int64_t pad_graph, int64_t cap_nodes, int64_t cap_edges,
                         int64_t* node_id, int64_t* edge_id, int64_t* new_edge_index, int64_t* new_batch, uint8_t* edge_mask,
                         int32_t* valid_out, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && N >= 0 && G >= 0 && pad_graph >= 0 && (mode == 0 || mode == 1) && cap_nodes >= 2 && cap_edges >= 0, GSAT_ERR_ARG,
                 "gsat_subgraph_padded: bad argument (two padding nodes always remain)");
    GSAT_REQUIRE(N < (1ll << 31) && E < (1ll << 31) && G < (1ll << 31) && pad_graph < (1ll << 31) && cap_nodes < (1ll << 31) &&
                 cap_edges < (1ll << 31), GSAT_ERR_UNSUPPORTED, "gsat_subgraph_padded: >2^31 entries");
    GSAT_REQUIRE(valid_out && node_id && (E == 0 || (edge_index && edge_mask)) && (mode == 0 ? (E == 0 || keep) : (N == 0 || keep)) &&
                 (cap_edges == 0 || (edge_id && new_edge_index)) && (!batch || new_batch), GSAT_ERR_ARG,
                 "gsat_subgraph_padded: null pointer");
    const SubLayout lay(N, E);
    Arena ar(workspace, ws_bytes);
    uint8_t* node_flag = ar.take<uint8_t>(lay.flag_bytes);
    int32_t* node_rank = ar.take<int32_t>((size_t)N + 1);
    int32_t* cnt_n = ar.take<int32_t>((size_t)lay.nb_nodes + 1);
    int32_t* cnt_e = ar.take<int32_t>((size_t)lay.nb_edges + 1);
    int32_t* bad = ar.take<int32_t>((size_t)lay.nb_edges + 1);
    GSAT_REQUIRE(ar.ok() && bad, GSAT_ERR_WORKSPACE, "gsat_subgraph_padded: workspace %zu < %zu", ws_bytes, ar.off);
    const int nbn = lay.nb_nodes, nbe = lay.nb_edges;
    if (mode == 0 && drop_isolated) {
        if (N > 0) {
            const int64_t n16 = (int64_t)(lay.flag_bytes / 16);
            k_sub_clear<<<(unsigned)ceil_div(n16, SUB_BLOCK), SUB_BLOCK, 0, stream>>>(reinterpret_cast<uint4*>(node_flag), n16);
            GSAT_LAUNCH_CHECK();
        }
        if (nbe > 0) {
            k_subp_flags<<<nbe, SUB_BLOCK, 0, stream>>>(edge_index, E, N, valid_in, keep, nullptr, nullptr, nullptr, node_flag, 0, edge_mask,
                                                        cnt_n, cnt_e, bad);
            GSAT_LAUNCH_CHECK();
        }
        if (nbn > 0) {
            k_subp_flags<<<nbn, SUB_BLOCK, 0, stream>>>(edge_index, E, N, valid_in, nullptr, nullptr, node_flag, node_flag, nullptr, nbn,
                                                        edge_mask, cnt_n, cnt_e, bad);
            GSAT_LAUNCH_CHECK();
        }
    } else if (nbn + nbe > 0) {
        const uint8_t* node_keep = mode == 1 ? keep : nullptr;
        k_subp_flags<<<nbn + nbe, SUB_BLOCK, 0, stream>>>(edge_index, E, N, valid_in, mode == 0 ? keep : nullptr, node_keep, node_keep,
                                                          node_flag, nullptr, nbn, edge_mask, cnt_n, cnt_e, bad);
        GSAT_LAUNCH_CHECK();
    }
    k_subp_scan<<<1, SUB_SCAN_BLOCK, 0, stream>>>(cnt_n, nbn, cnt_e, nbe, bad, cap_nodes, cap_edges, valid_in, G, valid_out);
    GSAT_LAUNCH_CHECK();
    // the real part, as gsat_subgraph_index emits it (never at or beyond the capacities); k_subp_fill then owns everything behind the
    // counts of valid_out -- all of it after an overflow
    k_sub_node_out<<<std::max(nbn, 1), SUB_BLOCK, 0, stream>>>(node_flag, N, cnt_n, nbn, batch, cap_nodes, node_id, new_batch, node_rank);
    GSAT_LAUNCH_CHECK();
    if (nbe > 0) {
        k_sub_edge_out<<<nbe, SUB_BLOCK, 0, stream>>>(edge_index, E, N, edge_mask, cnt_e, nbe, node_rank, cap_edges, edge_id, new_edge_index,
                                                      nullptr, 0, nullptr);
        GSAT_LAUNCH_CHECK();
    }
    k_subp_fill<<<(unsigned)ceil_div(std::max(cap_nodes, cap_edges), SUB_BLOCK), SUB_BLOCK, 0, stream>>>(valid_out, cap_nodes, cap_edges, pad_graph,
                                                                                                      node_id, new_batch, edge_id, new_edge_index);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_gather_rows(const void* table, const int64_t* index, int64_t n, int64_t row_bytes, void* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(n >= 0 && row_bytes >= 1, GSAT_ERR_ARG, "gsat_gather_rows: bad argument");
    if (n == 0) return GSAT_OK;
    GSAT_REQUIRE(table && index && out, GSAT_ERR_ARG, "gsat_gather_rows: null pointer");
    GSAT_REQUIRE(n <= (1ll << 62) / row_bytes, GSAT_ERR_UNSUPPORTED, "gsat_gather_rows: n * row_bytes overflows");
    const uintptr_t a = (uintptr_t)row_bytes | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out);
    if ((a & 15) == 0) launch_gather<uint4>(table, index, n, row_bytes, out, stream);
    else if ((a & 7) == 0) launch_gather<uint2>(table, index, n, row_bytes, out, stream);
    else if ((a & 3) == 0) launch_gather<uint32_t>(table, index, n, row_bytes, out, stream);
    else launch_gather<uint8_t>(table, index, n, row_bytes, out, stream);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
