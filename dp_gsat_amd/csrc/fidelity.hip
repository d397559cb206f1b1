// Device log of one explanation-fidelity epoch (dp_gsat_amd/eval_log.py: FidelityLog).
//
//   gsat_fidelity_append : one batch of three logit blocks (full graph, explanation alone, explanation removed) becomes, per graph, the
//                          three predicted classes and the three probabilities of the class predicted from the full graph, at the
//                          offset held in `state` ON THE DEVICE.  Two launches, as gsat_eval_log_append: the rows, then ONE thread that
//                          advances `state`; the stream orders them, so entries below the count never change again.
//   gsat_fidelity_reduce : the sums of everything logged, by one workgroup in a fixed order (fp64, no float atomics: bitwise
//                          repeatable), packed with the counters for ONE host read.
//   gsat_fidelity_reset  : zeroes the counters with a kernel (no memset node).
//   gsat_fidelity_curve_append / _reduce / _reset : the same log with a level axis, for the logits of a stacked batch (fidelity_stack.hip).
//   gsat_fidelity_curve_append_tasks / _reduce_tasks : the curve log of a multi-label head, one binary decision per (graph, task).
#include "common.h"
#include <algorithm>

namespace gsat {

constexpr int FID_BLOCK = 256;
constexpr int FID_MAX_BLOCKS = 1024;
constexpr int FID_FLAG_OVERFLOW = 1;            // a padded batch that did not fit its capacity (valid[3])
constexpr int FID_FLAG_FULL = 2;                // the append would exceed max_graphs

struct FidPlan { int64_t g, g0; int flag; };

// What this append does, from device memory alone; the row kernel and the commit kernel both evaluate it on the same, unchanged state.
__device__ __forceinline__ FidPlan fid_plan(const int32_t* __restrict__ valid, int64_t G_rows, const int64_t* __restrict__ state,
                                            int64_t max_graphs) {
    FidPlan p;
    p.g0 = state[0];
    p.g = 0;
    p.flag = 0;
    if (valid != nullptr && valid[3] != 0) { p.flag = FID_FLAG_OVERFLOW; return p; }
    const int64_t g = valid != nullptr ? min<int64_t>(max<int64_t>(valid[2], 0), G_rows) : G_rows;
    if (p.g0 < 0 || p.g0 + g > max_graphs) { p.flag = FID_FLAG_FULL; return p; }
    p.g = g;
    return p;
}

// class of a row (one logit: z >= 0; otherwise the argmax, lowest index on ties)
__device__ __forceinline__ int fid_class(const float* __restrict__ z, int C) {
    if (C == 1) return z[0] >= 0.f ? 1 : 0;
    int best = 0;
    float top = z[0];
    for (int c = 1; c < C; ++c) {
        const float v = z[c];
        if (v > top) { top = v; best = c; }
    }
    return best;
}

// probability of class `cls` (one logit: sigmoid(+-z); otherwise the softmax with the row maximum subtracted), in fp64 from the fp32 logits
__device__ __forceinline__ double fid_prob(const float* __restrict__ z, int C, int cls) {
    if (C == 1) {
        const double t = cls ? (double)z[0] : -(double)z[0];
        return 1.0 / (1.0 + exp(-t));
    }
    float top = z[0];
    for (int c = 1; c < C; ++c) top = fmaxf(top, z[c]);
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += exp((double)z[c] - (double)top);
    return exp((double)z[cls] - (double)top) / sum;
}

// one thread per graph row below the count; rows at or beyond it are never loaded
__global__ void __launch_bounds__(FID_BLOCK)
k_fid_rows(const float* __restrict__ full, const float* __restrict__ keep, const float* __restrict__ drop, int64_t G_rows, int C,
           const int32_t* __restrict__ valid, int32_t* __restrict__ log_cls, double* __restrict__ log_p, const int64_t* __restrict__ state,
           int64_t max_graphs) {
    const FidPlan p = fid_plan(valid, G_rows, state, max_graphs);
    if (p.flag) return;
    const int64_t stride = (int64_t)gridDim.x * FID_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * FID_BLOCK + threadIdx.x; i < p.g; i += stride) {
        const float *zf = full + i * C, *zk = keep + i * C, *zd = drop + i * C;
        const int cls = fid_class(zf, C);
        int32_t* oc = log_cls + (p.g0 + i) * 3;
        double* op = log_p + (p.g0 + i) * 3;
        oc[0] = cls; oc[1] = fid_class(zk, C); oc[2] = fid_class(zd, C);
        op[0] = fid_prob(zf, C, cls); op[1] = fid_prob(zk, C, cls); op[2] = fid_prob(zd, C, cls);
    }
}

__global__ void k_fid_commit(int64_t G_rows, const int32_t* __restrict__ valid, int64_t* __restrict__ state, int64_t max_graphs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const FidPlan p = fid_plan(valid, G_rows, state, max_graphs);
    if (p.flag) { state[2] |= (int64_t)p.flag; return; }
    state[0] = p.g0 + p.g;
    state[1] += 1;
}

__global__ void k_fid_reset(int64_t* __restrict__ state) {
    if (blockIdx.x == 0 && threadIdx.x < 4) state[threadIdx.x] = 0;
}

// sum over the workgroup in a fixed order (butterfly inside the wave, waves in index order); valid in thread 0
__device__ __forceinline__ double fid_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < FID_BLOCK / 64; ++w) s += sh[w];
    return s;
}

// out int64[10] = (graphs, batches, flags, #(cls_drop != cls_full), #(cls_keep != cls_full), then the bits of five doubles: the sums of
// p_full - p_drop, p_full - p_keep, p_full, p_keep, p_drop).  One workgroup; thread t adds rows t, t + 256, ... in that order.
__global__ void __launch_bounds__(FID_BLOCK)
k_fid_reduce(const int32_t* __restrict__ log_cls, const double* __restrict__ log_p, const int64_t* __restrict__ state, int64_t max_graphs,
             int64_t* __restrict__ out) {
    __shared__ double sh[FID_BLOCK / 64];
    const int64_t n = min<int64_t>(max<int64_t>(state[0], 0), max_graphs);
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, flips[2] = {0.0, 0.0};        // counts below 2^31: exact in fp64
    for (int64_t i = threadIdx.x; i < n; i += FID_BLOCK) {
        const int32_t* c = log_cls + i * 3;
        const double* p = log_p + i * 3;
        s[0] += p[0] - p[2]; s[1] += p[0] - p[1]; s[2] += p[0]; s[3] += p[1]; s[4] += p[2];
        flips[0] += c[2] != c[0] ? 1.0 : 0.0;
        flips[1] += c[1] != c[0] ? 1.0 : 0.0;
    }
    double t[7];
    for (int k = 0; k < 5; ++k) t[k] = fid_block_sum(s[k], sh);
    for (int k = 0; k < 2; ++k) t[5 + k] = fid_block_sum(flips[k], sh);
    if (threadIdx.x == 0) {
        out[0] = state[0]; out[1] = state[1]; out[2] = state[2];
        out[3] = (int64_t)t[5]; out[4] = (int64_t)t[6];
        for (int k = 0; k < 5; ++k) out[5 + k] = __double_as_longlong(t[k]);
    }
}

// ---- the level-aware log of a fidelity curve (dp_gsat_amd/eval_log.py: FidelityCurveLog) ---------------------------------------------------
// One batch is the logits of a stacked batch (fidelity_stack.hip): V = 2 S + 1 blocks of Gp rows -- the full batch, level s alone, the batch
// without level s.  state int64[FIDC_STATE] = (graphs, batches, flags, real edges, kept edges of level 0 .. 15).
constexpr int FIDC_MAX_LEVELS = 16;
constexpr int FIDC_STATE = 4 + FIDC_MAX_LEVELS;

// fid_plan for a stacked batch: the graph count is the input's valid[2] (without it the full variant's), and the batch is refused when
// the input or any variant of the stack had overflowed
__device__ __forceinline__ FidPlan fidc_plan(const int32_t* __restrict__ valid, const int32_t* __restrict__ stack_valid, int V, int64_t Gp,
                                             const int64_t* __restrict__ state, int64_t max_graphs) {
    FidPlan p;
    p.g0 = state[0];
    p.g = 0;
    p.flag = 0;
    int over = valid != nullptr && valid[3] != 0;
    for (int v = 0; v < V; ++v) over |= stack_valid[4 * v + 3] != 0;
    if (over) { p.flag = FID_FLAG_OVERFLOW; return p; }
    const int64_t g = min<int64_t>(max<int64_t>(valid != nullptr ? valid[2] : stack_valid[2], 0), Gp);
    if (p.g0 < 0 || p.g0 + g > max_graphs) { p.flag = FID_FLAG_FULL; return p; }
    p.g = g;
    return p;
}

// one thread per (graph, variant) below the count: the variant's class, and its probability of the class predicted from the full variant
__global__ void __launch_bounds__(FID_BLOCK)
k_fidc_rows(const float* __restrict__ logits, int64_t Gp, int C, int V, const int32_t* __restrict__ valid, const int32_t* __restrict__ stack_valid,
            int32_t* __restrict__ log_cls, double* __restrict__ log_p, const int64_t* __restrict__ state, int64_t max_graphs) {
    const FidPlan p = fidc_plan(valid, stack_valid, V, Gp, state, max_graphs);
    if (p.flag) return;
    const int64_t stride = (int64_t)gridDim.x * FID_BLOCK, items = p.g * V;
    for (int64_t t = (int64_t)blockIdx.x * FID_BLOCK + threadIdx.x; t < items; t += stride) {
        const int64_t i = t / V, v = t - i * V;
        const float *zf = logits + i * C, *zv = logits + (v * Gp + i) * C;
        const int cls = fid_class(zf, C);
        log_cls[(p.g0 + i) * V + v] = v == 0 ? cls : fid_class(zv, C);
        log_p[(p.g0 + i) * V + v] = fid_prob(zv, C, cls);
    }
}

__global__ void k_fidc_commit(int64_t Gp, int V, const int32_t* __restrict__ valid, const int32_t* __restrict__ stack_valid,
                              int64_t* __restrict__ state, int64_t max_graphs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const FidPlan p = fidc_plan(valid, stack_valid, V, Gp, state, max_graphs);
    if (p.flag) { state[2] |= (int64_t)p.flag; return; }
    state[0] = p.g0 + p.g;
    state[1] += 1;
    state[3] += stack_valid[1];
    for (int s = 0; s < (V - 1) / 2; ++s) state[4 + s] += stack_valid[4 * (1 + s) + 1];
}

__global__ void k_fidc_reset(int64_t* __restrict__ state) {
    if (blockIdx.x == 0 && threadIdx.x < FIDC_STATE) state[threadIdx.x] = 0;
}

// out int64[5 + 7 S]: (graphs, batches, flags, real edges), kept edges [S], #(cls_drop_s != cls_full) [S], #(cls_keep_s != cls_full) [S],
// then the bits of doubles: the sum of p_full, and per level the sums of p_keep, p_drop, p_full - p_drop, p_full - p_keep ([S] each).
// One workgroup; thread t adds rows t, t + 256, ... in that order, level after level.
__global__ void __launch_bounds__(FID_BLOCK)
k_fidc_reduce(const int32_t* __restrict__ log_cls, const double* __restrict__ log_p, const int64_t* __restrict__ state, int64_t max_graphs, int S,
              int64_t* __restrict__ out) {
    __shared__ double sh[FID_BLOCK / 64];
    const int V = 2 * S + 1;
    const int64_t n = min<int64_t>(max<int64_t>(state[0], 0), max_graphs);
    double full = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += FID_BLOCK) full += log_p[i * V];
    full = fid_block_sum(full, sh);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 4; ++k) out[k] = state[k];
        for (int s = 0; s < S; ++s) out[4 + s] = state[4 + s];
        out[4 + 3 * S] = __double_as_longlong(full);
    }
    for (int s = 0; s < S; ++s) {
        double a[4] = {0.0, 0.0, 0.0, 0.0}, flips[2] = {0.0, 0.0};          // counts below 2^31: exact in fp64
        for (int64_t i = threadIdx.x; i < n; i += FID_BLOCK) {
            const int32_t* c = log_cls + i * V;
            const double* p = log_p + i * V;
            const double pk = p[1 + s], pd = p[1 + S + s];
            a[0] += pk; a[1] += pd; a[2] += p[0] - pd; a[3] += p[0] - pk;
            flips[0] += c[1 + S + s] != c[0] ? 1.0 : 0.0;
            flips[1] += c[1 + s] != c[0] ? 1.0 : 0.0;
        }
        double t[6];
        for (int k = 0; k < 4; ++k) t[k] = fid_block_sum(a[k], sh);
        for (int k = 0; k < 2; ++k) t[4 + k] = fid_block_sum(flips[k], sh);
        if (threadIdx.x == 0) {
            out[4 + S + s] = (int64_t)t[4];
            out[4 + 2 * S + s] = (int64_t)t[5];
            for (int k = 0; k < 4; ++k) out[5 + (3 + k) * S + s] = __double_as_longlong(t[k]);
        }
    }
}

// ---- the curve log with a task axis (FidelityCurveLog(..., tasks=T)) ------------------------------------------------------------------------
// A multi-label head: every (graph, task) is a binary decision of its own -- class z >= 0, probability sigmoid(+-z), the one-logit rules of
// fid_class / fid_prob.  logits fp32[V * Gp, T]; log_cls / log_p [max_graphs, T, V].  The state words and the plan are fidc_plan's, and the
// commit is k_fidc_commit itself: state[0] counts graphs.

// one thread per (graph, task) below the count, the task running fastest: a wavefront reads consecutive floats of one block's rows, V times
__global__ void __launch_bounds__(FID_BLOCK)
k_fidt_rows(const float* __restrict__ logits, int64_t Gp, int T, int V, const int32_t* __restrict__ valid, const int32_t* __restrict__ stack_valid,
            int32_t* __restrict__ log_cls, double* __restrict__ log_p, const int64_t* __restrict__ state, int64_t max_graphs) {
    const FidPlan p = fidc_plan(valid, stack_valid, V, Gp, state, max_graphs);
    if (p.flag) return;
    const int64_t stride = (int64_t)gridDim.x * FID_BLOCK, items = p.g * T;
    for (int64_t t = (int64_t)blockIdx.x * FID_BLOCK + threadIdx.x; t < items; t += stride) {   // t = i * T + task
        const int cls = fid_class(logits + t, 1);
        int32_t* oc = log_cls + (p.g0 * T + t) * V;
        double* op = log_p + (p.g0 * T + t) * V;
        for (int v = 0; v < V; ++v) {
            const float* zv = logits + (int64_t)v * Gp * T + t;
            oc[v] = v == 0 ? cls : fid_class(zv, 1);
            op[v] = fid_prob(zv, 1, cls);
        }
    }
}

// Workgroup t reduces task t: thread k adds graphs k, k + 256, ... in that order, level after level (the order of k_fidc_reduce, whose sums
// it therefore repeats bit for bit at T = 1).  out int64[4 + S + T (1 + 6 S)]:
//   [0, 4)                         graphs, batches, flags, real edges                      (workgroup 0)
//   [4, 4 + S)                     kept edges per level                                    (workgroup 0)
//   then, with A = 4 + S:  A + (0 T + t) S + s   #(cls_drop_s != cls_full) of task t
//                          A + (1 T + t) S + s   #(cls_keep_s != cls_full) of task t
//   then the bits of doubles, with D = A + 2 T S:  D + t   the sum of p_full of task t
//                          D + T + (k T + t) S + s   k = 0 .. 3: the sums of p_keep_s, p_drop_s, p_full - p_drop_s, p_full - p_keep_s
__global__ void __launch_bounds__(FID_BLOCK)
k_fidt_reduce(const int32_t* __restrict__ log_cls, const double* __restrict__ log_p, const int64_t* __restrict__ state, int64_t max_graphs, int S,
              int T, int64_t* __restrict__ out) {
    __shared__ double sh[FID_BLOCK / 64];
    const int V = 2 * S + 1, task = blockIdx.x;
    const int64_t n = min<int64_t>(max<int64_t>(state[0], 0), max_graphs);
    const int64_t A = 4 + S, D = A + 2 * (int64_t)T * S;
    double full = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += FID_BLOCK) full += log_p[(i * T + task) * V];
    full = fid_block_sum(full, sh);
    if (threadIdx.x == 0) {
        if (task == 0) {
            for (int k = 0; k < 4; ++k) out[k] = state[k];
            for (int s = 0; s < S; ++s) out[4 + s] = state[4 + s];
        }
        out[D + task] = __double_as_longlong(full);
    }
    for (int s = 0; s < S; ++s) {
        double a[4] = {0.0, 0.0, 0.0, 0.0}, flips[2] = {0.0, 0.0};          // counts below 2^31: exact in fp64
        for (int64_t i = threadIdx.x; i < n; i += FID_BLOCK) {
            const int32_t* c = log_cls + (i * T + task) * V;
            const double* p = log_p + (i * T + task) * V;
            const double pk = p[1 + s], pd = p[1 + S + s];
            a[0] += pk; a[1] += pd; a[2] += p[0] - pd; a[3] += p[0] - pk;
            flips[0] += c[1 + S + s] != c[0] ? 1.0 : 0.0;
            flips[1] += c[1 + s] != c[0] ? 1.0 : 0.0;
        }
        double t[6];
        for (int k = 0; k < 4; ++k) t[k] = fid_block_sum(a[k], sh);
        for (int k = 0; k < 2; ++k) t[4 + k] = fid_block_sum(flips[k], sh);
        if (threadIdx.x == 0) {
            out[A + (int64_t)task * S + s] = (int64_t)t[4];
            out[A + ((int64_t)T + task) * S + s] = (int64_t)t[5];
            for (int k = 0; k < 4; ++k) out[D + T + ((int64_t)k * T + task) * S + s] = __double_as_longlong(t[k]);
        }
    }
}

}  // namespace gsat

using namespace gsat;

extern "C" {

int gsat_fidelity_append(const float* logits_full, const float* logits_keep, const float* logits_drop, int64_t graph_rows, int64_t classes,
                         const int32_t* valid, int32_t* log_cls, double* log_p, int64_t* log_state, int64_t max_graphs, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(graph_rows >= 0 && classes >= 1 && max_graphs >= 0, GSAT_ERR_ARG, "gsat_fidelity_append: bad extent");
    GSAT_REQUIRE(graph_rows < (1ll << 31) && classes < (1ll << 31) && max_graphs < (1ll << 31), GSAT_ERR_UNSUPPORTED,
                 "gsat_fidelity_append: >2^31 entries");
    GSAT_REQUIRE(log_state && (graph_rows == 0 || (logits_full && logits_keep && logits_drop)) && (max_graphs == 0 || (log_cls && log_p)),
                 GSAT_ERR_ARG, "gsat_fidelity_append: null pointer");
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(graph_rows, FID_BLOCK), 1), FID_MAX_BLOCKS);
    k_fid_rows<<<blocks, FID_BLOCK, 0, stream>>>(logits_full, logits_keep, logits_drop, graph_rows, (int)classes, valid, log_cls, log_p,
                                                 log_state, max_graphs);
    GSAT_LAUNCH_CHECK();
    k_fid_commit<<<1, 64, 0, stream>>>(graph_rows, valid, log_state, max_graphs);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_fidelity_reduce(const int32_t* log_cls, const double* log_p, const int64_t* log_state, int64_t max_graphs, int64_t* out,
                         void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(max_graphs >= 0 && log_state && out && (max_graphs == 0 || (log_cls && log_p)), GSAT_ERR_ARG,
                 "gsat_fidelity_reduce: bad argument");
    k_fid_reduce<<<1, FID_BLOCK, 0, stream>>>(log_cls, log_p, log_state, max_graphs, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_fidelity_reset(int64_t* log_state, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(log_state, GSAT_ERR_ARG, "gsat_fidelity_reset: null pointer");
    k_fid_reset<<<1, 64, 0, stream>>>(log_state);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_fidelity_curve_append(const float* logits, int64_t graphs_per_variant, int64_t classes, int64_t levels, const int32_t* valid,
                               const int32_t* stack_valid, int32_t* log_cls, double* log_p, int64_t* log_state, int64_t max_graphs,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(graphs_per_variant >= 0 && classes >= 1 && max_graphs >= 0 && levels >= 1 && levels <= FIDC_MAX_LEVELS, GSAT_ERR_ARG,
                 "gsat_fidelity_curve_append: bad extent (1..16 levels)");
    const int V = 2 * (int)levels + 1;
    GSAT_REQUIRE(graphs_per_variant < (1ll << 31) / V && classes < (1ll << 31) && max_graphs < (1ll << 31) / V, GSAT_ERR_UNSUPPORTED,
                 "gsat_fidelity_curve_append: >2^31 entries");
    GSAT_REQUIRE(log_state && stack_valid && (graphs_per_variant == 0 || logits) && (max_graphs == 0 || (log_cls && log_p)), GSAT_ERR_ARG,
                 "gsat_fidelity_curve_append: null pointer");
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(graphs_per_variant * V, FID_BLOCK), 1), FID_MAX_BLOCKS);
    k_fidc_rows<<<blocks, FID_BLOCK, 0, stream>>>(logits, graphs_per_variant, (int)classes, V, valid, stack_valid, log_cls, log_p, log_state,
                                                  max_graphs);
    GSAT_LAUNCH_CHECK();
    k_fidc_commit<<<1, 64, 0, stream>>>(graphs_per_variant, V, valid, stack_valid, log_state, max_graphs);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_fidelity_curve_reduce(const int32_t* log_cls, const double* log_p, const int64_t* log_state, int64_t max_graphs, int64_t levels,
                               int64_t* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(max_graphs >= 0 && levels >= 1 && levels <= FIDC_MAX_LEVELS && log_state && out && (max_graphs == 0 || (log_cls && log_p)),
                 GSAT_ERR_ARG, "gsat_fidelity_curve_reduce: bad argument");
    k_fidc_reduce<<<1, FID_BLOCK, 0, stream>>>(log_cls, log_p, log_state, max_graphs, (int)levels, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_fidelity_curve_append_tasks(const float* logits, int64_t graphs_per_variant, int64_t tasks, int64_t levels, const int32_t* valid,
                                     const int32_t* stack_valid, int32_t* log_cls, double* log_p, int64_t* log_state, int64_t max_graphs,
                                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(graphs_per_variant >= 0 && tasks >= 1 && max_graphs >= 0 && levels >= 1 && levels <= FIDC_MAX_LEVELS, GSAT_ERR_ARG,
                 "gsat_fidelity_curve_append_tasks: bad extent (1..16 levels)");
    GSAT_REQUIRE(tasks <= 1024, GSAT_ERR_UNSUPPORTED, "gsat_fidelity_curve_append_tasks: more than 1024 tasks");
    const int V = 2 * (int)levels + 1;
    const int64_t per_graph = tasks * V;                                     // at most 1024 * 33
    GSAT_REQUIRE(graphs_per_variant < (1ll << 31) / per_graph && max_graphs < (1ll << 31) / per_graph, GSAT_ERR_UNSUPPORTED,
                 "gsat_fidelity_curve_append_tasks: >2^31 entries");
    GSAT_REQUIRE(log_state && stack_valid && (graphs_per_variant == 0 || logits) && (max_graphs == 0 || (log_cls && log_p)), GSAT_ERR_ARG,
                 "gsat_fidelity_curve_append_tasks: null pointer");
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(graphs_per_variant * tasks, FID_BLOCK), 1), FID_MAX_BLOCKS);
    k_fidt_rows<<<blocks, FID_BLOCK, 0, stream>>>(logits, graphs_per_variant, (int)tasks, V, valid, stack_valid, log_cls, log_p, log_state,
                                                  max_graphs);
    GSAT_LAUNCH_CHECK();
    k_fidc_commit<<<1, 64, 0, stream>>>(graphs_per_variant, V, valid, stack_valid, log_state, max_graphs);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_fidelity_curve_reduce_tasks(const int32_t* log_cls, const double* log_p, const int64_t* log_state, int64_t max_graphs, int64_t levels,
                                     int64_t tasks, int64_t* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(max_graphs >= 0 && levels >= 1 && levels <= FIDC_MAX_LEVELS && tasks >= 1 && log_state && out &&
                 (max_graphs == 0 || (log_cls && log_p)), GSAT_ERR_ARG, "gsat_fidelity_curve_reduce_tasks: bad argument");
    GSAT_REQUIRE(tasks <= 1024 && max_graphs < (1ll << 31) / (tasks * (2 * levels + 1)), GSAT_ERR_UNSUPPORTED,
                 "gsat_fidelity_curve_reduce_tasks: more than 1024 tasks or >2^31 entries");
    k_fidt_reduce<<<(unsigned)tasks, FID_BLOCK, 0, stream>>>(log_cls, log_p, log_state, max_graphs, (int)levels, (int)tasks, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_fidelity_curve_reset(int64_t* log_state, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(log_state, GSAT_ERR_ARG, "gsat_fidelity_curve_reset: null pointer");
    k_fidc_reset<<<1, 64, 0, stream>>>(log_state);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
