// Device log of one classifier epoch (dp_gsat_amd/eval_log.py: ClfLog) -- what the ERM pre-training loop of src/pretrain_clf.py keeps
// per batch: the logits, the labels and the loss -- and the integer counts its accuracy is made of.
//
//   gsat_clf_log_append : appends the real rows of one batch's logits and labels at the offsets held in `state` ON THE DEVICE.  Two
//                         launches, as in eval_log.hip: the copies, then ONE thread that adds the loss and advances `state`.  The
//                         stream orders the second after the first, so whoever finds a count in `state` finds every row below it
//                         written, and rows below the count are never written again.
//   gsat_clf_log_counts : the confusion matrix (single label) or the per-task (tn, fp, fn, tp, unlabelled) counts (multi-label) of
//                         the first state[0] logged rows.  Comparisons only; counters per workgroup in LDS, non-zero ones flushed
//                         with 64-bit integer atomics: the result does not depend on the order and is bitwise repeatable.  The
//                         counters of `out` are zeroed by a launch of their own ahead of it: a grid that adds into `out` across
//                         workgroups cannot also zero it without a grid-wide barrier.
#include "common.h"

namespace gsat {

constexpr int CLF_BLOCK = 256;
constexpr int CLF_MAX_BLOCKS = 1024;
constexpr int CLF_MAX_CLASSES = 32;
constexpr int CLF_MAX_TASKS = 256;
constexpr int CLF_TASK_WORDS = 5;                                  // tn, fp, fn, tp, unlabelled
constexpr int CLF_SLOTS = CLF_MAX_TASKS * CLF_TASK_WORDS;          // >= 32 * 32 + 1
constexpr int CLF_FLAG_OVERFLOW = 1;                               // a padded batch that did not fit its capacity (valid[3])
constexpr int CLF_FLAG_FULL = 2;                                   // a count outside [0, G_cap], or more than max_graphs / max_batches

static_assert(CLF_MAX_CLASSES * CLF_MAX_CLASSES + 1 <= CLF_SLOTS, "the confusion matrix fits the counter block");

struct ClfBatch {                                                  // the batch being appended
    const float* logits;                                           // fp32[G_cap, logit_cols]
    const float* y;                                                // fp32[G_cap, y_cols]
    const int32_t* valid;                                          // int32[4] (N_real, E_real, B, overflow) or null: every row is real
    const float* loss;                                             // fp32[1] or null
    int64_t G_cap, logit_cols, y_cols;
};

struct ClfArrays {
    float* logits;
    float* y;
    double* loss_sum;
    int64_t* state;                                                // graphs, batches, flags, 0
    int64_t max_graphs, max_batches;
};

struct ClfPlan { int64_t G, g0, b0; int flag; };

// What this append does, from device memory alone; the copy kernel and the commit kernel both evaluate it on the same, unchanged state.
__device__ __forceinline__ ClfPlan clf_plan(const ClfBatch& b, const ClfArrays& l) {
    ClfPlan p;
    p.g0 = l.state[0]; p.b0 = l.state[1];
    p.G = 0;
    p.flag = 0;
    if (b.valid != nullptr && b.valid[3] != 0) { p.flag = CLF_FLAG_OVERFLOW; return p; }
    const int64_t G = b.valid != nullptr ? (int64_t)b.valid[2] : b.G_cap;
    if (G < 0 || G > b.G_cap) { p.flag = CLF_FLAG_FULL; return p; }
    if (p.g0 < 0 || p.b0 < 0 || p.g0 + G > l.max_graphs || p.b0 + 1 > l.max_batches) { p.flag = CLF_FLAG_FULL; return p; }
    p.G = G;
    return p;
}

// The launch geometry comes from G_cap; the count is read here, and no row at or beyond it is loaded.  Stores of element width: the
// destination starts at an arbitrary row.
__global__ void __launch_bounds__(CLF_BLOCK)
k_clf_copy(ClfBatch b, ClfArrays l) {
    const ClfPlan p = clf_plan(b, l);
    if (p.flag) return;
    const int64_t stride = (int64_t)gridDim.x * CLF_BLOCK;
    const int64_t t0 = (int64_t)blockIdx.x * CLF_BLOCK + threadIdx.x;
    for (int64_t i = t0; i < p.G * b.logit_cols; i += stride) l.logits[p.g0 * b.logit_cols + i] = b.logits[i];
    for (int64_t i = t0; i < p.G * b.y_cols; i += stride) l.y[p.g0 * b.y_cols + i] = b.y[i];
}

__global__ void k_clf_commit(ClfBatch b, ClfArrays l) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const ClfPlan p = clf_plan(b, l);
    if (p.flag) { l.state[2] |= (int64_t)p.flag; return; }
    // no loss given: the sum turns NaN, and so does the mean compute() reports
    l.loss_sum[0] += b.loss != nullptr ? (double)b.loss[0] : __longlong_as_double(0x7FF8000000000000ll);
    l.state[0] = p.g0 + p.G;
    l.state[1] = p.b0 + 1;
}

// ---- counts -------------------------------------------------------------------------------------------------------------------------
__global__ void k_clf_zero(unsigned long long* __restrict__ out, int words) {
    for (int s = threadIdx.x; s < words; s += blockDim.x) out[s] = 0ull;
}

// mode 0 / 1: one thread per logged row, slot = label * C + predicted class, or C * C for a row that matches nothing.
// mode 2    : one thread per (row, task) entry, slot = task * 5 + (2 * label + prediction), or task * 5 + 4 for an unlabelled entry.
// A workgroup counts fewer than 2^31 entries per counter (max_graphs < 2^31), so 32-bit LDS counters hold them.
__global__ void __launch_bounds__(CLF_BLOCK)
k_clf_count(const float* __restrict__ logits, const float* __restrict__ y, const int64_t* __restrict__ state, int64_t max_graphs,
            int C, int mode, int words, unsigned long long* __restrict__ out) {
    __shared__ uint32_t cnt[CLF_SLOTS];
    for (int s = threadIdx.x; s < words; s += CLF_BLOCK) cnt[s] = 0;
    __syncthreads();
    int64_t n = state[0];
    n = n < 0 ? 0 : (n > max_graphs ? max_graphs : n);             // never beyond the arrays, whatever the counter block holds
    const int64_t stride = (int64_t)gridDim.x * CLF_BLOCK;
    const int64_t t0 = (int64_t)blockIdx.x * CLF_BLOCK + threadIdx.x;
    if (mode == 2) {
        for (int64_t i = t0; i < n * C; i += stride) {
            const int t = (int)(i % C);
            const float label = y[i], z = logits[i];
            int slot = t * CLF_TASK_WORDS + 4;
            if (label == label) slot = t * CLF_TASK_WORDS + (label != 0.f ? 2 : 0) + (z > 0.f ? 1 : 0);
            atomicAdd(&cnt[slot], 1u);
        }
    } else {
        const int classes = mode == 0 ? 2 : C;
        for (int64_t row = t0; row < n; row += stride) {
            const float* z = logits + row * C;
            bool bad = false;
            int pred = 0;
            if (mode == 0) {
                const float v = z[0];
                bad = v != v;
                pred = v > 0.f ? 1 : 0;
            } else {
                float best = z[0];
                bad = best != best;
                for (int c = 1; c < C; ++c) {
                    const float v = z[c];
                    bad = bad || v != v;
                    if (v > best) { best = v; pred = c; }          // strict: the lowest index wins a tie
                }
            }
            const float label = y[row];
            int cls = -1;
            if (label >= 0.f && label < (float)classes) {          // false for NaN
                cls = (int)label;
                if ((float)cls != label) cls = -1;                 // not an integer
            }
            atomicAdd(&cnt[(bad || cls < 0) ? classes * classes : cls * classes + pred], 1u);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < words; s += CLF_BLOCK) {
        const uint32_t c = cnt[s];
        if (c) atomicAdd(&out[s], (unsigned long long)c);          // 64-bit integer vector atomic: the sum does not depend on the order
    }
}

static int64_t clf_count_words(int64_t logit_cols, int64_t y_cols, int mode) {
    if (mode == 0) return logit_cols == 1 && y_cols == 1 ? 5 : -1;
    if (mode == 1) return logit_cols >= 2 && logit_cols <= CLF_MAX_CLASSES && y_cols == 1 ? logit_cols * logit_cols + 1 : -1;
    if (mode == 2) return logit_cols >= 1 && logit_cols <= CLF_MAX_TASKS && y_cols == logit_cols ? logit_cols * CLF_TASK_WORDS : -1;
    return -1;
}

}  // namespace gsat

using namespace gsat;

extern "C" {

int gsat_clf_log_append(const float* logits, const float* y, const int32_t* valid, const float* loss, int64_t graph_cap,
                        int64_t logit_cols, int64_t y_cols, float* log_logits, float* log_y, double* log_loss_sum, int64_t* log_state,
                        int64_t max_graphs, int64_t max_batches, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(graph_cap >= 0 && logit_cols >= 0 && y_cols >= 0 && max_graphs >= 0 && max_batches >= 0, GSAT_ERR_ARG,
                 "gsat_clf_log_append: negative extent");
    GSAT_REQUIRE(graph_cap < (1ll << 31) && max_graphs < (1ll << 31), GSAT_ERR_UNSUPPORTED, "gsat_clf_log_append: >2^31 rows");
    GSAT_REQUIRE(log_loss_sum && log_state, GSAT_ERR_ARG, "gsat_clf_log_append: null pointer");
    GSAT_REQUIRE(graph_cap == 0 || max_graphs == 0 || ((logit_cols == 0 || (logits && log_logits)) && (y_cols == 0 || (y && log_y))),
                 GSAT_ERR_ARG, "gsat_clf_log_append: null graph array");
    const ClfBatch b{logits, y, valid, loss, graph_cap, logit_cols, y_cols};
    const ClfArrays l{log_logits, log_y, log_loss_sum, log_state, max_graphs, max_batches};
    const int64_t work = graph_cap * std::max<int64_t>(logit_cols, y_cols);
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(work, CLF_BLOCK), 1), CLF_MAX_BLOCKS);
    k_clf_copy<<<blocks, CLF_BLOCK, 0, stream>>>(b, l);
    GSAT_LAUNCH_CHECK();
    k_clf_commit<<<1, 64, 0, stream>>>(b, l);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int64_t gsat_clf_log_counts_words(int64_t logit_cols, int64_t y_cols, int mode) { return clf_count_words(logit_cols, y_cols, mode); }

int gsat_clf_log_counts(const float* log_logits, const float* log_y, const int64_t* log_state, int64_t max_graphs, int64_t logit_cols,
                        int64_t y_cols, int mode, int64_t* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(mode >= 0 && mode <= 2 && max_graphs >= 0 && logit_cols >= 1 && y_cols >= 1, GSAT_ERR_ARG,
                 "gsat_clf_log_counts: bad argument");
    GSAT_REQUIRE(max_graphs < (1ll << 31), GSAT_ERR_UNSUPPORTED, "gsat_clf_log_counts: >2^31 rows");
    GSAT_REQUIRE(mode != 1 || logit_cols <= CLF_MAX_CLASSES, GSAT_ERR_UNSUPPORTED, "gsat_clf_log_counts: more than %d classes",
                 CLF_MAX_CLASSES);
    GSAT_REQUIRE(mode != 2 || logit_cols <= CLF_MAX_TASKS, GSAT_ERR_UNSUPPORTED, "gsat_clf_log_counts: more than %d tasks", CLF_MAX_TASKS);
    const int64_t words = clf_count_words(logit_cols, y_cols, mode);
    GSAT_REQUIRE(words > 0, GSAT_ERR_ARG, "gsat_clf_log_counts: mode %d does not take %lld logit and %lld label columns", mode,
                 (long long)logit_cols, (long long)y_cols);
    GSAT_REQUIRE(log_state && out && (max_graphs == 0 || (log_logits && log_y)), GSAT_ERR_ARG, "gsat_clf_log_counts: null pointer");
    const int64_t work = max_graphs * (mode == 2 ? logit_cols : 1);
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(work, CLF_BLOCK), 1), CLF_MAX_BLOCKS);
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
    k_clf_zero<<<1, CLF_BLOCK, 0, stream>>>(o, (int)words);
    GSAT_LAUNCH_CHECK();
    k_clf_count<<<blocks, CLF_BLOCK, 0, stream>>>(log_logits, log_y, log_state, max_graphs, (int)logit_cols, mode, (int)words, o);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
