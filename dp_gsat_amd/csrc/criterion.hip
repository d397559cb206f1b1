// The classification criterion (src/utils/get_model.py:19-34) over the first b rows of a fixed-capacity [G, C] logit tensor, b read on
// the device: binary cross entropy with logits (mode 0), cross entropy (mode 1), BCE over the labelled entries (mode 2, NaN target =
// unlabelled).  Forward: one pass of per-block partials (sum, count), one final block (fixed order, no float atomics: the result is
// bitwise repeatable); backward: one elementwise / row-wise launch.  Rows at or beyond b are never loaded.
#include "common.h"

#include <cmath>

namespace gsat {

constexpr int CRB = 256;               // threads per block
constexpr int CR_MAX_BLOCKS = 256;     // partials: one per thread of the final block
constexpr int CR_ROW_TRIPS = 4;        // mode 1: rows a lane group takes before another block is opened
constexpr int64_t CR_MAX_ROWS = 1ll << 20, CR_MAX_COLS = 1024;

__device__ __forceinline__ int64_t cr_rows(const int32_t* __restrict__ g_valid, int64_t G) {
    return g_valid ? min<int64_t>(max<int64_t>(*g_valid, 0), G) : G;
}

// max(z, 0) - z y + log1p(exp(-|z|)): no overflow for any finite z
__device__ __forceinline__ float cr_bce(float z, float y) { return fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float cr_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// block totals of a float sum and an entry count in every thread: DPP / swizzle inside the wave (common.h), then the waves in order
// through LDS.  The count is summed as an integer: exact for every supported size (G C <= 2^30).
__device__ __forceinline__ void cr_block_sum(float& s, uint32_t& n, float* sm_s, uint32_t* sm_n) {
    s = group_sum<64>(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) { sm_s[threadIdx.x >> 6] = s; sm_n[threadIdx.x >> 6] = n; }
    __syncthreads();
    s = sm_s[0]; n = sm_n[0];
#pragma unroll
    for (int w = 1; w < CRB / 64; ++w) { s += sm_s[w]; n += sm_n[w]; }
}

// modes 0 and 2.  partial[k] = sum of the terms over the entries [k * per_block, min(b C, (k + 1) * per_block)), partial[CR_MAX_BLOCKS +
// k] = how many of them are labelled (the bits of a uint32)
template <bool MULTI>
__global__ __launch_bounds__(CRB) void k_crit_bce_partial(const float* __restrict__ z, const float* __restrict__ y, int64_t G, int64_t C,
                                                          int64_t per_block, const int32_t* __restrict__ g_valid,
                                                          float* __restrict__ partial) {
    __shared__ float sm_s[CRB / 64];
    __shared__ uint32_t sm_n[CRB / 64];
    const int64_t beg = (int64_t)blockIdx.x * per_block, end = min(cr_rows(g_valid, G) * C, beg + per_block);
    float s = 0.f;
    uint32_t n = 0;
    for (int64_t i = beg + threadIdx.x; i < end; i += CRB) {
        const float t = y[i];
        if (MULTI && t != t) continue;
        s += cr_bce(z[i], t);
        ++n;
    }
    cr_block_sum(s, n, sm_s, sm_n);
    if (threadIdx.x == 0) { partial[blockIdx.x] = s; partial[CR_MAX_BLOCKS + blockIdx.x] = __uint_as_float(n); }
}

template <int LPR> __device__ __forceinline__ float cr_group_max(float v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// (max, sum exp(z - max)) of one row in every lane of its group of LPR lanes
template <int LPR> __device__ __forceinline__ void cr_row_softmax(const float* __restrict__ zr, int C, int lane, float& m, float& se) {
    m = -INFINITY;
    for (int c = lane; c < C; c += LPR) m = fmaxf(m, zr[c]);
    m = cr_group_max<LPR>(m);
    se = 0.f;
    for (int c = lane; c < C; c += LPR) se += expf(zr[c] - m);
    se = group_sum<LPR>(se);
}

// the class of a row, or -1 when the label is no index into [0, C) (NaN included)
__device__ __forceinline__ int cr_label(float t, int C) { return (t >= 0.f && t < (float)C) ? (int)t : -1; }

// mode 1.  LPR lanes own a row; block k takes the rows [k * per_block, min(b, (k + 1) * per_block)) and partial[k] is the sum of their
// logsumexp(z) - z[label]; a label outside [0, C) contributes NaN and reads nothing
template <int LPR>
__global__ __launch_bounds__(CRB) void k_crit_ce_partial(const float* __restrict__ z, const float* __restrict__ y, int64_t G, int C,
                                                         int64_t per_block, const int32_t* __restrict__ g_valid,
                                                         float* __restrict__ partial) {
    __shared__ float sm_s[CRB / 64];
    __shared__ uint32_t sm_n[CRB / 64];
    constexpr int GPB = CRB / LPR;
    const int grp = threadIdx.x / LPR, lane = threadIdx.x % LPR;
    const int64_t beg = (int64_t)blockIdx.x * per_block, end = min(cr_rows(g_valid, G), beg + per_block);
    float s = 0.f;
    uint32_t n = 0;
    for (int64_t r = beg + grp; r < end; r += GPB) {       // uniform over the group: its lanes stay together in the reductions
        const float* zr = z + r * C;
        float m, se;
        cr_row_softmax<LPR>(zr, C, lane, m, se);
        if (lane == 0) {
            const int k = cr_label(y[r], C);
            s += k >= 0 ? (m + logf(se)) - zr[k] : NAN;
            ++n;
        }
    }
    cr_block_sum(s, n, sm_s, sm_n);
    if (threadIdx.x == 0) { partial[blockIdx.x] = s; partial[CR_MAX_BLOCKS + blockIdx.x] = __uint_as_float(n); }
}

// loss[0] = sum / div and stats[4] = (sum, div, 1 / div, 0) with div = max(count, 1): count = b C (mode 0), b (mode 1) or the number of
// labelled entries (mode 2).  An empty selection gives the loss 0.
__global__ __launch_bounds__(CRB) void k_crit_final(const float* __restrict__ partial, int nb, float* __restrict__ loss,
                                                    float* __restrict__ stats) {
    __shared__ float sm_s[CRB / 64];
    __shared__ uint32_t sm_n[CRB / 64];
    const bool has = (int)threadIdx.x < nb;
    float s = has ? partial[threadIdx.x] : 0.f;
    uint32_t n = has ? __float_as_uint(partial[CR_MAX_BLOCKS + threadIdx.x]) : 0u;
    cr_block_sum(s, n, sm_s, sm_n);
    if (threadIdx.x != 0) return;
    const float div = (float)max(n, 1u);
    loss[0] = s / div;
    stats[0] = s; stats[1] = div; stats[2] = 1.f / div; stats[3] = 0.f;
}

// modes 0 and 2: dz = gout (sigmoid(z) - y) / div, 0 on unlabelled entries and exactly 0 (without a load) at or beyond row b
template <bool MULTI>
__global__ __launch_bounds__(CRB) void k_crit_bce_bwd(const float* __restrict__ z, const float* __restrict__ y,
                                                      const float* __restrict__ stats, const float* __restrict__ gout, int64_t G, int64_t C,
                                                      const int32_t* __restrict__ g_valid, float* __restrict__ dz) {
    const int64_t i = (int64_t)blockIdx.x * CRB + threadIdx.x;
    if (i >= G * C) return;
    float d = 0.f;
    if (i < cr_rows(g_valid, G) * C) {
        const float t = y[i];
        if (!(MULTI && t != t)) d = gout[0] * stats[2] * (cr_sigmoid(z[i]) - t);
    }
    dz[i] = d;
}

// mode 1: dz[r, c] = gout (softmax(z[r])[c] - [c == label]) / div; a row whose label is no class gets NaN (its loss is NaN), a row at
// or beyond b exactly 0 without a load
template <int LPR>
__global__ __launch_bounds__(CRB) void k_crit_ce_bwd(const float* __restrict__ z, const float* __restrict__ y,
                                                     const float* __restrict__ stats, const float* __restrict__ gout, int64_t G, int C,
                                                     const int32_t* __restrict__ g_valid, float* __restrict__ dz) {
    constexpr int GPB = CRB / LPR;
    const int lane = threadIdx.x % LPR;
    const int64_t r = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;          // uniform over the group
    if (r >= G) return;
    float* dr = dz + r * C;
    if (r >= cr_rows(g_valid, G)) {
        for (int c = lane; c < C; c += LPR) dr[c] = 0.f;
        return;
    }
    const float* zr = z + r * C;
    float m, se;
    cr_row_softmax<LPR>(zr, C, lane, m, se);
    const int k = cr_label(y[r], C);
    const float w = gout[0] * stats[2], inv = 1.f / se;
    for (int c = lane; c < C; c += LPR) dr[c] = k >= 0 ? w * (expf(zr[c] - m) * inv - (c == k ? 1.f : 0.f)) : NAN;
}

static inline int cr_ce_lanes(int64_t C) { return C <= 16 ? 4 : 64; }

// rows (mode 1) or entries (modes 0, 2) of one first-stage block while fewer than CR_MAX_BLOCKS blocks are in use
static inline int64_t cr_block_items(int64_t C, int mode) { return mode == 1 ? (int64_t)(CRB / cr_ce_lanes(C)) * CR_ROW_TRIPS : 4 * CRB; }

static inline const char* cr_check(const void* logits, const void* target, int64_t G, int64_t C, int mode) {
    if (!logits || !target) return "null pointer";
    if (mode < 0 || mode > 2) return "mode must be 0 (binary), 1 (cross entropy) or 2 (multi-label)";
    if (G < 1 || C < 1) return "needs at least one row and one column";
    return nullptr;
}

}  // namespace gsat

using namespace gsat;

extern "C" {

int64_t gsat_criterion_block_items(int64_t C, int mode) { return cr_block_items(C, mode); }
int64_t gsat_criterion_max_blocks(void) { return CR_MAX_BLOCKS; }

int gsat_criterion_fwd(const float* logits, const float* target, int64_t G, int64_t C, int mode, const int32_t* g_valid_dev,
                       float* partial /* [512] */, float* loss, float* stats /* [4] */, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* bad = cr_check(logits, target, G, C, mode);
    GSAT_REQUIRE(!bad && partial && loss && stats, GSAT_ERR_ARG, "gsat_criterion_fwd: %s", bad ? bad : "null pointer");
    GSAT_REQUIRE(G <= CR_MAX_ROWS && C <= CR_MAX_COLS, GSAT_ERR_UNSUPPORTED, "gsat_criterion_fwd: at most 2^20 rows of 1024 columns");
    const int64_t items = mode == 1 ? G : G * C, chunk = cr_block_items(C, mode);
    int nb = (int)std::min<int64_t>(CR_MAX_BLOCKS, ceil_div(items, chunk));
    const int64_t per_block = ceil_div(items, nb);
    nb = (int)ceil_div(items, per_block);
    if (mode == 0) k_crit_bce_partial<false><<<nb, CRB, 0, stream>>>(logits, target, G, C, per_block, g_valid_dev, partial);
    else if (mode == 2) k_crit_bce_partial<true><<<nb, CRB, 0, stream>>>(logits, target, G, C, per_block, g_valid_dev, partial);
    else if (cr_ce_lanes(C) == 4) k_crit_ce_partial<4><<<nb, CRB, 0, stream>>>(logits, target, G, (int)C, per_block, g_valid_dev, partial);
    else k_crit_ce_partial<64><<<nb, CRB, 0, stream>>>(logits, target, G, (int)C, per_block, g_valid_dev, partial);
    k_crit_final<<<1, CRB, 0, stream>>>(partial, nb, loss, stats);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_criterion_bwd(const float* logits, const float* target, const float* stats, const float* gout, int64_t G, int64_t C, int mode,
                       const int32_t* g_valid_dev, float* dlogits, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* bad = cr_check(logits, target, G, C, mode);
    GSAT_REQUIRE(!bad && stats && gout && dlogits, GSAT_ERR_ARG, "gsat_criterion_bwd: %s", bad ? bad : "null pointer");
    GSAT_REQUIRE(G <= CR_MAX_ROWS && C <= CR_MAX_COLS, GSAT_ERR_UNSUPPORTED, "gsat_criterion_bwd: at most 2^20 rows of 1024 columns");
    if (mode != 1) {
        const unsigned grid = (unsigned)ceil_div(G * C, CRB);
        if (mode == 0) k_crit_bce_bwd<false><<<grid, CRB, 0, stream>>>(logits, target, stats, gout, G, C, g_valid_dev, dlogits);
        else k_crit_bce_bwd<true><<<grid, CRB, 0, stream>>>(logits, target, stats, gout, G, C, g_valid_dev, dlogits);
    } else if (cr_ce_lanes(C) == 4) {
        k_crit_ce_bwd<4><<<(unsigned)ceil_div(G, CRB / 4), CRB, 0, stream>>>(logits, target, stats, gout, G, (int)C, g_valid_dev, dlogits);
    } else {
        k_crit_ce_bwd<64><<<(unsigned)ceil_div(G, CRB / 64), CRB, 0, stream>>>(logits, target, stats, gout, G, (int)C, g_valid_dev, dlogits);
    }
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
