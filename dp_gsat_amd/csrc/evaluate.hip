// Evaluation scores on the device: the exact, tie-aware ROC-AUC of every task of a multi-task classifier (the ogb Evaluator's rocauc:
// src/run_gsat.py:756-759, src/pretrain_clf.py:104) and the two-class attention histogram behind add_histogram / add_pr_curve
// (src/run_gsat.py:767-776).  Integer arithmetic only: both results are bitwise repeatable.
//
//   task AUROC : gsat_auroc (explain.hip) with the task id in front of the score: 64-bit keys (task << 32) | ascending score bits, an
//                unlabelled (NaN) entry under the sentinel task T so that it sorts behind every real task; ONE stable rocPRIM radix
//                sort over 32 + bits(T) key bits carrying the class byte, ONE exclusive scan of the negatives, the segment bounds of the
//                T tasks by binary search, and the pass of k_auroc_sum on the 64-bit keys -- a tie run never crosses a task because the
//                task is part of the key.
//   histogram  : per-workgroup counters in LDS (2 B bins + 2 outside counters, uint32), a grid-stride loop, LDS integer atomics, and a
//                flush of the non-zero counters with 64-bit global integer atomics.  Attention after the sigmoid piles into a few bins,
//                and same-address LDS atomics of one wavefront serialise, so lanes with equal counters are combined BEFORE the atomic:
//                up to HIST_PEEL rounds of (first pending lane's counter, ballot of the lanes that share it, one atomic of the
//                popcount); what is still pending afterwards -- a spread-out input, where conflicts are rare -- adds 1 per lane.
#include "common.h"
#include <algorithm>
#include <rocprim/rocprim.hpp>

namespace gsat {

// ascending-score sort word, -0.0 == +0.0 (the complement of explain.hip's att_desc_bits)
__device__ __forceinline__ uint32_t score_asc_bits(float a) {
    uint32_t b = __float_as_uint(a);
    if (b == 0x80000000u) b = 0u;
    return b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}

// ---- task AUROC ---------------------------------------------------------------------------------------------------------------------
constexpr int TASK_BLOCK = 256;
constexpr uint8_t CLS_NEG = 0, CLS_POS = 1, CLS_NONE = 2;

__global__ void k_task_keys(const float* __restrict__ score, const float* __restrict__ label, int64_t n, int T, uint64_t* __restrict__ keys,
                            uint8_t* __restrict__ cls) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float l = label[i];
    const bool none = l != l;
    const uint32_t task = none ? (uint32_t)T : (uint32_t)(i % T);
    keys[i] = ((uint64_t)task << 32) | score_asc_bits(score[i]);
    cls[i] = none ? CLS_NONE : (l != 0.f ? CLS_POS : CLS_NEG);
}

struct IsNegativeClass {
    const uint8_t* cls;
    int64_t n;
    __host__ __device__ int operator()(int i) const { return (i < n && cls[i] == CLS_NEG) ? 1 : 0; }
};

// first position whose key is >= `key` in keys[lo, hi)
__device__ __forceinline__ int64_t lower_bound(const uint64_t* __restrict__ keys, int64_t lo, int64_t hi, uint64_t key) {
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}

// seg[t] = first sorted position of task t, t = 0 .. T (seg[T]: where the unlabelled entries begin); out[t] = (0, P_t, Nn_t)
__global__ void k_task_bounds(const uint64_t* __restrict__ keys, const int32_t* __restrict__ cneg, int64_t n, int T, int32_t* __restrict__ seg,
                              unsigned long long* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > T) return;
    const int64_t s = lower_bound(keys, 0, n, (uint64_t)t << 32);
    seg[t] = (int32_t)s;
    if (t == T) return;
    const int64_t e = lower_bound(keys, s, n, (uint64_t)(t + 1) << 32);
    const unsigned long long nn = (unsigned long long)(cneg[e] - cneg[s]);
    out[3 * t + 0] = 0;
    out[3 * t + 1] = (unsigned long long)(e - s) - nn;
    out[3 * t + 2] = nn;
}

// keys ascending, cls in the same order, cneg[i] = negatives among positions < i.  A positive of task t whose tie group is [s, e) adds
// (cneg[s] - base) + (cneg[e] - base), base = cneg[seg[t]] = the negatives in front of the task's segment.  One position per thread; a
// wavefront whose positives all belong to one task (all but the <= T waves that straddle a boundary) adds once.
__global__ void __launch_bounds__(TASK_BLOCK)
k_task_sum(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ cls, const int32_t* __restrict__ cneg, const int32_t* __restrict__ seg,
           int64_t n, int T, unsigned long long* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * TASK_BLOCK + threadIdx.x;
    unsigned long long acc = 0;
    int task = -1;
    if (q < n && cls[q] == CLS_POS) {
        const uint64_t key = keys[q];
        const int t = (int)(key >> 32);
        if (t >= 0 && t < T) {                   // always, for keys k_task_keys wrote
            const int64_t s0 = seg[t], e0 = seg[t + 1];
            const int64_t s = lower_bound(keys, s0, q, key);                 // first position with this key (it is <= q)
            const int64_t e = lower_bound(keys, q + 1, e0, key + 1);         // first position behind its tie group
            const unsigned long long base = (unsigned long long)cneg[s0];
            acc = ((unsigned long long)cneg[s] - base) + ((unsigned long long)cneg[e] - base);
            task = t;
        }
    }
    const uint64_t have = __ballot(task >= 0);
    if (have == 0) return;                       // uniform over the wavefront
    const int first = __builtin_amdgcn_readlane(task, __ffsll((unsigned long long)have) - 1);
    if (__ballot(task >= 0 && task != first) == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&out[3 * first], acc);
    } else if (task >= 0 && acc) {
        atomicAdd(&out[3 * task], acc);          // 64-bit integer vector atomic: the sum does not depend on the order
    }
}

static unsigned task_key_bits(int64_t T) {
    unsigned b = 1;
    while (b < 31 && (T >> b) != 0) ++b;         // the task field holds 0 .. T
    return 32u + b;
}
static size_t task_sort_temp_bytes(int64_t n, int64_t T) {
    size_t tb = 0;
    uint64_t* kk = nullptr;
    uint8_t* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, tb, kk, kk, v, v, (size_t)(n > 0 ? n : 1), 0, task_key_bits(T), (hipStream_t)0);
    return align_up(tb, 256) + 256;
}
static size_t task_scan_temp_bytes(int64_t n) {
    size_t tb = 0;
    auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int>(0), IsNegativeClass{nullptr, 0});
    int32_t* out = nullptr;
    (void)rocprim::exclusive_scan(nullptr, tb, in, out, 0, (size_t)(n + 1), rocprim::plus<int>(), (hipStream_t)0);
    return align_up(tb, 256) + 256;
}

// ---- histogram ----------------------------------------------------------------------------------------------------------------------
constexpr int HIST_BLOCK = 256;
constexpr int HIST_MAX_BINS = 4096;
constexpr int HIST_MAX_BLOCKS = 1024;
constexpr int HIST_PEEL = 4;

// counter of this lane (-1 = none) += 1, equal counters of the wavefront combined first; every lane of the wavefront calls it
__device__ __forceinline__ void wave_count(uint32_t* __restrict__ cnt, int slot) {
    uint64_t todo = __ballot(slot >= 0);
    for (int r = 0; r < HIST_PEEL && todo != 0; ++r) {                      // `todo` is uniform over the wavefront
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int s = __builtin_amdgcn_readlane(slot, leader);
        const uint64_t same = __ballot(slot == s);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&cnt[s], (uint32_t)__popcll(same));
        if (slot == s) slot = -1;
        todo &= ~same;
    }
    if (slot >= 0) atomicAdd(&cnt[slot], 1u);
}

// cnt: [2 B] bins (class-major) then [2] outside.  A workgroup counts at most 2^32 - 1 entries (the host bounds E / gridDim.x).
__global__ void __launch_bounds__(HIST_BLOCK)
k_att_hist(const float* __restrict__ att, const uint8_t* __restrict__ label, int64_t E, int B, double lo, double hi, double scale,
           unsigned long long* __restrict__ hist, unsigned long long* __restrict__ outside) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cnt[];
    const int slots = 2 * B + 2;
    for (int s = threadIdx.x; s < slots; s += HIST_BLOCK) cnt[s] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * HIST_BLOCK;
    const int64_t rounds = (E + stride - 1) / stride;                       // every lane runs every round: the ballots see whole waves
    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t i = r * stride + (int64_t)blockIdx.x * HIST_BLOCK + threadIdx.x;
        int slot = -1;
        if (i < E) {
            const double a = (double)att[i];
            const int c = (label != nullptr && label[i] != 0) ? 1 : 0;
            if (a >= lo && a <= hi) {                                       // false for NaN
                const double t = (a - lo) * scale;
                int bin = (int)floor(t);
                bin = bin < 0 ? 0 : (bin > B - 1 ? B - 1 : bin);            // a == hi (t == B) -> the closed last bin
                slot = c * B + bin;
            } else {
                slot = 2 * B + c;
            }
        }
        wave_count(cnt, slot);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < slots; s += HIST_BLOCK) {
        const uint32_t c = cnt[s];
        if (c) atomicAdd(s < 2 * B ? &hist[s] : &outside[s - 2 * B], (unsigned long long)c);
    }
}

}  // namespace gsat

using namespace gsat;

extern "C" {

size_t gsat_auroc_tasks_workspace_bytes(int64_t R, int64_t T) {
    const bool ok = R > 0 && T > 0 && R <= ((1ll << 31) - 1) / T;
    const size_t n = ok ? (size_t)(R * T) : 1, t = ok ? (size_t)T : 1;
    return 256 + 2 * align_up(n * 8, 256) + 2 * align_up(n, 256) + align_up((n + 1) * 4, 256) + align_up((t + 1) * 4, 256) +
           std::max(task_sort_temp_bytes((int64_t)n, (int64_t)t), task_scan_temp_bytes((int64_t)n));
}

int gsat_auroc_tasks(const float* score, const float* label, int64_t R, int64_t T, uint64_t* out, void* workspace, size_t ws_bytes,
                     void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(R >= 0 && T >= 0, GSAT_ERR_ARG, "gsat_auroc_tasks: bad argument");
    GSAT_REQUIRE(T == 0 || R <= ((1ll << 31) - 1) / T, GSAT_ERR_UNSUPPORTED, "gsat_auroc_tasks: R * T >= 2^31");
    if (T == 0) return GSAT_OK;
    GSAT_REQUIRE(out, GSAT_ERR_ARG, "gsat_auroc_tasks: null output");
    const int64_t n = R * T;
    if (n == 0) {
        GSAT_CHECK_HIP(gsat::zero_async(out, (size_t)T * 3 * sizeof(uint64_t), stream));
        return GSAT_OK;
    }
    GSAT_REQUIRE(score && label, GSAT_ERR_ARG, "gsat_auroc_tasks: null pointer");
    Arena ar(workspace, ws_bytes);
    uint64_t* keys_in = ar.take<uint64_t>(n);
    uint64_t* keys_out = ar.take<uint64_t>(n);
    uint8_t* cls_in = ar.take<uint8_t>(n);
    uint8_t* cls_out = ar.take<uint8_t>(n);
    int32_t* cneg = ar.take<int32_t>(n + 1);
    int32_t* seg = ar.take<int32_t>(T + 1);
    size_t ts = task_sort_temp_bytes(n, T), tc = task_scan_temp_bytes(n);
    char* temp = ar.take<char>(std::max(ts, tc));
    GSAT_REQUIRE(ar.ok() && temp, GSAT_ERR_WORKSPACE, "gsat_auroc_tasks: workspace %zu < %zu", ws_bytes, ar.off);
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
    k_task_keys<<<(unsigned)ceil_div(n, TASK_BLOCK), TASK_BLOCK, 0, stream>>>(score, label, n, (int)T, keys_in, cls_in);
    GSAT_LAUNCH_CHECK();
    GSAT_CHECK_HIP(rocprim::radix_sort_pairs(temp, ts, keys_in, keys_out, cls_in, cls_out, (size_t)n, 0, task_key_bits(T), stream));
    auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int>(0), IsNegativeClass{cls_out, n});
    GSAT_CHECK_HIP(rocprim::exclusive_scan(temp, tc, in, cneg, 0, (size_t)(n + 1), rocprim::plus<int>(), stream));
    k_task_bounds<<<(unsigned)ceil_div(T + 1, TASK_BLOCK), TASK_BLOCK, 0, stream>>>(keys_out, cneg, n, (int)T, seg, o);
    GSAT_LAUNCH_CHECK();
    k_task_sum<<<(unsigned)ceil_div(n, TASK_BLOCK), TASK_BLOCK, 0, stream>>>(keys_out, cls_out, cneg, seg, n, (int)T, o);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_att_histogram(const float* att, const uint8_t* label, int64_t E, int64_t bins, double lo, double hi, uint64_t* hist,
                       uint64_t* outside, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && bins >= 1 && bins <= HIST_MAX_BINS && lo < hi, GSAT_ERR_ARG,
                 "gsat_att_histogram: bad argument (1 <= bins <= %d, lo < hi)", HIST_MAX_BINS);
    GSAT_REQUIRE(E < (1ll << 40), GSAT_ERR_UNSUPPORTED, "gsat_att_histogram: >= 2^40 entries");
    if (E == 0) return GSAT_OK;
    GSAT_REQUIRE(att && hist && outside, GSAT_ERR_ARG, "gsat_att_histogram: null pointer");
    // a workgroup zeroes and flushes 2 B + 2 counters: give it at least as many entries to count (and 1024 at the least)
    const int64_t per = std::max<int64_t>(1024, 2 * bins);
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(E, per), HIST_MAX_BLOCKS);
    const size_t lds = (size_t)(2 * bins + 2) * sizeof(uint32_t);           // <= 32 KiB + 8 B: below the default dynamic-LDS limit
    k_att_hist<<<blocks, HIST_BLOCK, lds, stream>>>(att, label, E, (int)bins, lo, hi, (double)bins / (hi - lo),
                                                     reinterpret_cast<unsigned long long*>(hist),
                                                     reinterpret_cast<unsigned long long*>(outside));
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
