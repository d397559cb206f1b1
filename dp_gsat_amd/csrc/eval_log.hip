// Device log of one evaluation epoch (dp_gsat_amd/eval_log.py) and the per-segment delta-KL that scores it.
//
//   gsat_eval_log_append   : appends one batch -- attention and labels gathered graph by graph, the batch's edge pointers shifted by the
//                            running edge offset, the real rows of the logits and of y -- at the offsets held in `state` ON THE DEVICE.
//                            Two launches: the copies, then ONE thread that advances `state`.  The stream orders the second after the
//                            first, so whoever finds a count in `state` finds every entry below it already written, and entries
//                            below the count are never written again.
//   gsat_delta_kl_segments : gsat_delta_kl of every segment att[seg_ptr[s] : seg_ptr[s+1]] in one call.  Segments are few and long
//                            (the batches of an epoch), so a segment is cut into chunks of KLS_CHUNK entries and the grid is
//                            (chunks of the longest segment) x (segments): every workgroup owns one chunk of one segment.
//                            Three launches: per-chunk sums of clamp(a); per-chunk terms against the segment's own r (every chunk
//                            re-adds its segment's chunk sums in index order); one thread per segment adds the chunks in index
//                            order.  fp64, no float atomics: bitwise repeatable.
#include "common.h"

namespace gsat {

constexpr int LOG_BLOCK = 256;
constexpr int LOG_MAX_BLOCKS = 1024;
constexpr int LOG_FLAG_OVERFLOW = 1;            // a padded batch that did not fit its capacity (valid[3])
constexpr int LOG_FLAG_FULL = 2;                // the append would exceed max_edges / max_graphs / max_batches

struct LogBatch {                               // the batch being appended
    const float* att;                           // fp32[E_cap], by edge id
    const uint8_t* label;                       // uint8[E_cap], by edge id
    const int32_t* edge_ptr;                    // int32[G_cap + 1]: slots of the edges-by-graph order
    const int32_t* edge_order;                  // int32[E_cap]: edge ids graph by graph, ascending inside a graph
    const float* logits;                        // fp32[G_cap, logit_cols]
    const float* y;                             // fp32[G_cap, y_cols]
    const int32_t* valid;                       // int32[4] (N_real, E_real, B, overflow) or null: every graph is real
    const float* losses;                        // fp32[3] or null
    int64_t E_cap, G_cap, logit_cols, y_cols;
};

struct LogArrays {
    float* att;
    uint8_t* label;
    int32_t* graph_edge_ptr;
    float* logits;
    float* y;
    int64_t* batch_edge_ptr;
    double* loss_sums;
    int64_t* state;                             // edges, graphs, batches, flags
    int64_t max_edges, max_graphs, max_batches;
};

struct LogPlan { int64_t E, G, e0, g0, b0; int flag; };

// What this append does, from device memory alone; the copy kernel and the commit kernel both evaluate it on the same, unchanged state.
__device__ __forceinline__ LogPlan log_plan(const LogBatch& b, const LogArrays& l) {
    LogPlan p;
    p.e0 = l.state[0]; p.g0 = l.state[1]; p.b0 = l.state[2];
    p.E = p.G = 0;
    p.flag = 0;
    if (b.valid != nullptr && b.valid[3] != 0) { p.flag = LOG_FLAG_OVERFLOW; return p; }
    const int64_t G = b.valid != nullptr ? (int64_t)b.valid[2] : b.G_cap;
    if (G < 0 || G > b.G_cap) { p.flag = LOG_FLAG_FULL; return p; }
    const int64_t E = (int64_t)b.edge_ptr[G];
    const bool sane = E >= 0 && E <= b.E_cap && p.e0 >= 0 && p.g0 >= 0 && p.b0 >= 0;
    if (!sane || p.e0 + E > l.max_edges || p.g0 + G > l.max_graphs || p.b0 + 1 > l.max_batches) { p.flag = LOG_FLAG_FULL; return p; }
    p.E = E; p.G = G;
    return p;
}

// The launch geometry comes from the capacities; the counts are read here.  Stores of element width: the destinations start at
// arbitrary element offsets (no 16-byte alignment for the floats, none at all for the labels), consecutive lanes still write
// consecutive addresses, and the attention / label reads are gathers anyway.
__global__ void __launch_bounds__(LOG_BLOCK)
k_log_copy(LogBatch b, LogArrays l) {
    const LogPlan p = log_plan(b, l);
    if (p.flag) return;
    const int64_t stride = (int64_t)gridDim.x * LOG_BLOCK;
    const int64_t t0 = (int64_t)blockIdx.x * LOG_BLOCK + threadIdx.x;
    for (int64_t i = t0; i < p.E; i += stride) {
        int32_t e = b.edge_order[i];
        const bool ok = e >= 0 && (int64_t)e < b.E_cap;            // memory-safe on a corrupt permutation
        l.att[p.e0 + i] = ok ? b.att[e] : 0.f;
        l.label[p.e0 + i] = ok && b.label[e] != 0 ? 1 : 0;
    }
    // graph g's first slot; entry g0 itself belongs to the batch before (it is only written by the very first append, as 0)
    for (int64_t g = t0 + (p.g0 == 0 ? 0 : 1); g <= p.G; g += stride)
        l.graph_edge_ptr[p.g0 + g] = (int32_t)(p.e0 + (int64_t)b.edge_ptr[g]);
    for (int64_t i = t0; i < p.G * b.logit_cols; i += stride) l.logits[p.g0 * b.logit_cols + i] = b.logits[i];
    for (int64_t i = t0; i < p.G * b.y_cols; i += stride) l.y[p.g0 * b.y_cols + i] = b.y[i];
}

__global__ void k_log_commit(LogBatch b, LogArrays l) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const LogPlan p = log_plan(b, l);
    if (p.flag) { l.state[3] |= (int64_t)p.flag; return; }
    if (p.b0 == 0) l.batch_edge_ptr[0] = 0;
    l.batch_edge_ptr[p.b0 + 1] = p.e0 + p.E;
    // no losses given: the sums turn NaN, and so do the means compute() reports
    for (int c = 0; c < 3; ++c) l.loss_sums[c] += b.losses != nullptr ? (double)b.losses[c] : __longlong_as_double(0x7FF8000000000000ll);
    l.state[0] = p.e0 + p.E;
    l.state[1] = p.g0 + p.G;
    l.state[2] = p.b0 + 1;
}

// ---- delta KL per segment -----------------------------------------------------------------------------------------------------------
constexpr int KLS_BLOCK = 256;
constexpr int KLS_CHUNK = 4096;                 // entries one workgroup handles: 16 per thread

__device__ __forceinline__ double kls_clamp(double a, double lo, double hi) { return a < lo ? lo : (a > hi ? hi : a); }

// sum over the workgroup in a fixed order (butterfly inside the wave, waves in index order); valid in thread 0
__device__ __forceinline__ double kls_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < KLS_BLOCK / 64; ++w) s += sh[w];
    return s;
}

// bounds of segment s, or false when seg_ptr is not a non-decreasing sequence inside [0, E] or the segment is longer than the caller's
// bound (nc chunks): such a segment is never evaluated in part, its row becomes NaN
__device__ __forceinline__ bool kls_bounds(const int64_t* __restrict__ seg_ptr, int s, int64_t E, int nc, int64_t& lo, int64_t& n) {
    lo = seg_ptr[s];
    n = seg_ptr[s + 1] - lo;
    return lo >= 0 && n >= 0 && lo + n <= E && n <= (int64_t)nc * KLS_CHUNK;
}

// partial[(s * nc + c) * 5 + 0]: sum of clamp(a) over chunk c of segment s
__global__ void __launch_bounds__(KLS_BLOCK)
k_kls_mean(const float* __restrict__ att, const int64_t* __restrict__ seg_ptr, int64_t E, int nc, double eps, double* __restrict__ partial) {
    __shared__ double sh[KLS_BLOCK / 64];
    const int c = blockIdx.x, s = blockIdx.y;
    int64_t lo, n;
    if (!kls_bounds(seg_ptr, s, E, nc, lo, n) || (int64_t)c * KLS_CHUNK >= n) return;           // uniform over the workgroup
    const int64_t c0 = (int64_t)c * KLS_CHUNK, c1 = c0 + KLS_CHUNK < n ? c0 + KLS_CHUNK : n;
    double acc = 0.0;
    for (int64_t i = c0 + threadIdx.x; i < c1; i += KLS_BLOCK) acc += kls_clamp((double)att[lo + i], eps, 1.0 - eps);
    const double t = kls_block_sum(acc, sh);
    if (threadIdx.x == 0) partial[((int64_t)s * nc + c) * 5] = t;
}

// partial[.. + 1 .. 4]: (kl, sum of labelled attention, labelled count, sum of unlabelled attention) of the chunk
__global__ void __launch_bounds__(KLS_BLOCK)
k_kls_terms(const float* __restrict__ att, const uint8_t* __restrict__ label, const int64_t* __restrict__ seg_ptr, int64_t E, int nc,
            double eps, double* __restrict__ partial) {
    __shared__ double sh[KLS_BLOCK / 64];
    const int c = blockIdx.x, s = blockIdx.y;
    int64_t lo, n;
    if (!kls_bounds(seg_ptr, s, E, nc, lo, n) || (int64_t)c * KLS_CHUNK >= n) return;
    const int chunks = (int)((n + KLS_CHUNK - 1) / KLS_CHUNK);
    double* mine = partial + (int64_t)s * nc * 5;
    double total = 0.0;
    for (int q = 0; q < chunks; ++q) total += mine[q * 5];          // every chunk forms its segment's mean in the same order
    const double r = kls_clamp(total / (double)n, eps, 1.0 - eps);
    const double lr = log(r), l1r = log(1.0 - r);
    const int64_t c0 = (int64_t)c * KLS_CHUNK, c1 = c0 + KLS_CHUNK < n ? c0 + KLS_CHUNK : n;
    double kl = 0.0, sig = 0.0, cnt = 0.0, bkg = 0.0;
    for (int64_t i = c0 + threadIdx.x; i < c1; i += KLS_BLOCK) {
        const double raw = (double)att[lo + i];
        const double a = kls_clamp(raw, eps, 1.0 - eps);
        const bool pos = label[lo + i] != 0;
        const double p = pos ? 1.0 - eps : eps;
        kl += p * (log(a) - lr) + (1.0 - p) * (log(1.0 - a) - l1r);
        if (pos) { sig += raw; cnt += 1.0; } else bkg += raw;
    }
    const double s0 = kls_block_sum(kl, sh), s1 = kls_block_sum(sig, sh), s2 = kls_block_sum(cnt, sh), s3 = kls_block_sum(bkg, sh);
    if (threadIdx.x == 0) { double* o = mine + c * 5; o[1] = s0; o[2] = s1; o[3] = s2; o[4] = s3; }
}

__global__ void k_kls_finish(const double* __restrict__ partial, const int64_t* __restrict__ seg_ptr, int64_t S, int64_t E, int nc,
                             float* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    int64_t lo, n;
    float* o = out + 3 * s;
    if (!kls_bounds(seg_ptr, (int)s, E, nc, lo, n)) {
        o[0] = o[1] = o[2] = __uint_as_float(0x7FC00000u);
        return;
    }
    const int chunks = (int)((n + KLS_CHUNK - 1) / KLS_CHUNK);
    const double* mine = partial + s * nc * 5;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < chunks; ++q)
        for (int c = 0; c < 4; ++c) t[c] += mine[q * 5 + 1 + c];
    const double nneg = (double)n - t[2];
    o[0] = (float)t[0];
    o[1] = t[2] > 0.0 ? (float)(t[1] / t[2]) : 0.f;
    o[2] = nneg > 0.0 ? (float)(t[3] / nneg) : 0.f;
}

static int64_t kls_chunks(int64_t max_seg_len) { return std::max<int64_t>(ceil_div(max_seg_len, KLS_CHUNK), 1); }

}  // namespace gsat

using namespace gsat;

extern "C" {

int gsat_eval_log_append(const float* att, const uint8_t* label, const int32_t* edge_ptr, const int32_t* edge_order, const float* logits,
                         const float* y, const int32_t* valid, const float* losses, int64_t edge_cap, int64_t graph_cap,
                         int64_t logit_cols, int64_t y_cols, float* log_att, uint8_t* log_label, int32_t* log_graph_edge_ptr,
                         float* log_logits, float* log_y, int64_t* log_batch_edge_ptr, double* log_loss_sums, int64_t* log_state,
                         int64_t max_edges, int64_t max_graphs, int64_t max_batches, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(edge_cap >= 0 && graph_cap >= 0 && logit_cols >= 0 && y_cols >= 0 && max_edges >= 0 && max_graphs >= 0 && max_batches >= 0,
                 GSAT_ERR_ARG, "gsat_eval_log_append: negative extent");
    GSAT_REQUIRE(max_edges < (1ll << 31) && edge_cap < (1ll << 31) && graph_cap < (1ll << 31) && max_graphs < (1ll << 31),
                 GSAT_ERR_UNSUPPORTED, "gsat_eval_log_append: >2^31 entries (the ranking kernels carry int32 edge ids)");
    GSAT_REQUIRE(edge_ptr && log_graph_edge_ptr && log_batch_edge_ptr && log_loss_sums && log_state, GSAT_ERR_ARG,
                 "gsat_eval_log_append: null pointer");
    GSAT_REQUIRE(edge_cap == 0 || max_edges == 0 || (att && label && edge_order && log_att && log_label), GSAT_ERR_ARG,
                 "gsat_eval_log_append: null edge array");
    GSAT_REQUIRE(graph_cap == 0 || max_graphs == 0 || ((logit_cols == 0 || (logits && log_logits)) && (y_cols == 0 || (y && log_y))),
                 GSAT_ERR_ARG, "gsat_eval_log_append: null graph array");
    const LogBatch b{att, label, edge_ptr, edge_order, logits, y, valid, losses, edge_cap, graph_cap, logit_cols, y_cols};
    const LogArrays l{log_att, log_label, log_graph_edge_ptr, log_logits, log_y, log_batch_edge_ptr, log_loss_sums, log_state,
                      max_edges, max_graphs, max_batches};
    const int64_t work = std::max<int64_t>(std::max<int64_t>(edge_cap, graph_cap + 1), graph_cap * std::max<int64_t>(logit_cols, y_cols));
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(work, LOG_BLOCK), 1), LOG_MAX_BLOCKS);
    k_log_copy<<<blocks, LOG_BLOCK, 0, stream>>>(b, l);
    GSAT_LAUNCH_CHECK();
    k_log_commit<<<1, 64, 0, stream>>>(b, l);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int64_t gsat_delta_kl_segments_chunk(void) { return KLS_CHUNK; }

size_t gsat_delta_kl_segments_workspace_bytes(int64_t num_segments, int64_t max_seg_len) {
    const int64_t S = num_segments > 0 ? num_segments : 1;
    return 256 + (size_t)S * (size_t)kls_chunks(max_seg_len) * 5 * sizeof(double);
}

int gsat_delta_kl_segments(const float* att, const uint8_t* label, const int64_t* seg_ptr, int64_t num_segments, int64_t num_edges,
                           int64_t max_seg_len, double eps, float* out, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(num_segments >= 0 && num_edges >= 0 && max_seg_len >= 0 && eps > 0.0 && eps < 0.5, GSAT_ERR_ARG,
                 "gsat_delta_kl_segments: bad argument");
    if (num_segments == 0) return GSAT_OK;
    GSAT_REQUIRE(seg_ptr && out && (num_edges == 0 || (att && label)), GSAT_ERR_ARG, "gsat_delta_kl_segments: null pointer");
    const int64_t nc = kls_chunks(max_seg_len);
    GSAT_REQUIRE(num_segments <= 65535 && nc < (1ll << 31), GSAT_ERR_UNSUPPORTED, "gsat_delta_kl_segments: more than 65535 segments");
    Arena ar(workspace, ws_bytes);
    double* partial = ar.take<double>((size_t)num_segments * nc * 5);
    GSAT_REQUIRE(ar.ok() && partial, GSAT_ERR_WORKSPACE, "gsat_delta_kl_segments: workspace %zu < %zu", ws_bytes, ar.off);
    const dim3 grid((unsigned)nc, (unsigned)num_segments);
    k_kls_mean<<<grid, KLS_BLOCK, 0, stream>>>(att, seg_ptr, num_edges, (int)nc, eps, partial);
    GSAT_LAUNCH_CHECK();
    k_kls_terms<<<grid, KLS_BLOCK, 0, stream>>>(att, label, seg_ptr, num_edges, (int)nc, eps, partial);
    GSAT_LAUNCH_CHECK();
    k_kls_finish<<<(unsigned)ceil_div(num_segments, 64), 64, 0, stream>>>(partial, seg_ptr, num_segments, num_edges, (int)nc, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
