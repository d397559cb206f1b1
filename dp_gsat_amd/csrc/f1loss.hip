// Soft-F1 sparsity loss of the dual/primal step (src/run_gsat.py:151-180): (1 - softF1(p, y)) + mean|p| over the first m entries of a
// fixed-capacity tensor.  Forward: one pass of per-block partials of the four sums, one final block (fixed order, no float atomics: the
// result is bitwise repeatable); backward: one elementwise launch.  Entries at or beyond m are never loaded.
#include "common.h"

namespace gsat {

constexpr int F1B = 256;              // threads per block
constexpr int F1_MAX_BLOCKS = 256;    // partials: one per thread of the final block
constexpr float F1_EPS = 1e-6f;

__device__ __forceinline__ int64_t f1_counted(const int32_t* __restrict__ m_valid, int64_t M) {
    return m_valid ? min<int64_t>(max<int64_t>(*m_valid, 0), M) : M;
}

__device__ __forceinline__ void f1_acc(float4& s, float p, float y) {       // (sum p*y, sum p, sum y, sum |p|)
    s.x += p * y; s.y += p; s.z += y; s.w += fabsf(p);
}

// sums of the block's four accumulators in thread 0: DPP / swizzle inside the wave (common.h), then the waves in order through LDS
__device__ __forceinline__ float4 f1_block_sum(float4 s, float4* sm) {
    s.x = group_sum<64>(s.x); s.y = group_sum<64>(s.y); s.z = group_sum<64>(s.z); s.w = group_sum<64>(s.w);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    float4 t = sm[0];
#pragma unroll
    for (int w = 1; w < F1B / 64; ++w) { t.x += sm[w].x; t.y += sm[w].y; t.z += sm[w].z; t.w += sm[w].w; }
    return t;
}

// partial[b] = the four sums over [b * per_block, min(m, (b + 1) * per_block)); per_block is a multiple of 4, so with VEC (p and y 16-byte
// aligned) every float4 load is aligned, and it is issued only when all four entries are counted
template <bool VEC>
__global__ __launch_bounds__(F1B) void k_f1_partial(const float* __restrict__ p, const float* __restrict__ y, int64_t M, int64_t per_block,
                                                    const int32_t* __restrict__ m_valid, float4* __restrict__ partial) {
    __shared__ float4 sm[F1B / 64];
    const int64_t beg = (int64_t)blockIdx.x * per_block, end = min(f1_counted(m_valid, M), beg + per_block);
    float4 s = f4zero();
    for (int64_t i = beg + 4 * (int64_t)threadIdx.x; i < end; i += 4 * F1B) {
        if (VEC && i + 4 <= end) {
            const float4 a = ld4(p + i), b = ld4(y + i);
            f1_acc(s, a.x, b.x); f1_acc(s, a.y, b.y); f1_acc(s, a.z, b.z); f1_acc(s, a.w, b.w);
        } else {
            for (int64_t k = i; k < min(i + 4, end); ++k) f1_acc(s, p[k], y[k]);
        }
    }
    const float4 t = f1_block_sum(s, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// loss[0] and stats[8] = (TP, P, G, sum|p|, dloss/dTP, dloss/dP, 1 / max(m, 1), 0): the backward is dp = gout * (stats[4] * y + stats[5] +
// sign(p) * stats[6]).  m = 0: every sum is 0, f1 = 0 / eps = 0 and the loss is 1.
__global__ __launch_bounds__(F1B) void k_f1_final(const float4* __restrict__ partial, int nb, int64_t M, const int32_t* __restrict__ m_valid,
                                                  float* __restrict__ loss, float* __restrict__ stats) {
    __shared__ float4 sm[F1B / 64];
    const float4 s = f1_block_sum((int)threadIdx.x < nb ? partial[threadIdx.x] : f4zero(), sm);
    if (threadIdx.x != 0) return;
    const float inv_m = 1.f / (float)max<int64_t>(f1_counted(m_valid, M), 1);
    const float TP = s.x, P = s.y, G = s.z;
    const float qp = P + F1_EPS, qg = G + F1_EPS;
    const float prec = TP / qp, rec = TP / qg;
    const float D = prec + rec + F1_EPS;
    const float f1 = 2.f * prec * rec / D;
    const float df_dprec = 2.f * rec * (rec + F1_EPS) / (D * D), df_drec = 2.f * prec * (prec + F1_EPS) / (D * D);
    loss[0] = (1.f - f1) + s.w * inv_m;
    stats[0] = TP; stats[1] = P; stats[2] = G; stats[3] = s.w;
    stats[4] = -(df_dprec / qp + df_drec / qg);
    stats[5] = df_dprec * TP / (qp * qp);
    stats[6] = inv_m;
    stats[7] = 0.f;
}

__device__ __forceinline__ float f1_grad(float p, float y, float g, float c_tp, float c_p, float inv_m) {
    const float sgn = p > 0.f ? 1.f : (p < 0.f ? -1.f : 0.f);
    return g * (c_tp * y + c_p + sgn * inv_m);
}

// four entries per thread; entries at or beyond m get an exact 0 and are not loaded
template <bool VEC>
__global__ __launch_bounds__(F1B) void k_f1_bwd(const float* __restrict__ p, const float* __restrict__ y, const float* __restrict__ stats,
                                                const float* __restrict__ gout, int64_t M, const int32_t* __restrict__ m_valid,
                                                float* __restrict__ dp) {
    const int64_t i = 4 * ((int64_t)blockIdx.x * F1B + threadIdx.x);
    if (i >= M) return;
    const int64_t m = f1_counted(m_valid, M);
    const float g = gout[0], c_tp = stats[4], c_p = stats[5], inv_m = stats[6];
    if (VEC && i + 4 <= M) {
        float4 d = f4zero();
        if (i + 4 <= m) {
            const float4 a = ld4(p + i), b = ld4(y + i);
            d = make_float4(f1_grad(a.x, b.x, g, c_tp, c_p, inv_m), f1_grad(a.y, b.y, g, c_tp, c_p, inv_m),
                            f1_grad(a.z, b.z, g, c_tp, c_p, inv_m), f1_grad(a.w, b.w, g, c_tp, c_p, inv_m));
        } else {
            if (i < m) d.x = f1_grad(p[i], y[i], g, c_tp, c_p, inv_m);
            if (i + 1 < m) d.y = f1_grad(p[i + 1], y[i + 1], g, c_tp, c_p, inv_m);
            if (i + 2 < m) d.z = f1_grad(p[i + 2], y[i + 2], g, c_tp, c_p, inv_m);
        }
        st4(dp + i, d);
    } else {
        for (int64_t k = i; k < min(i + 4, M); ++k) dp[k] = k < m ? f1_grad(p[k], y[k], g, c_tp, c_p, inv_m) : 0.f;
    }
}

static inline bool f1_aligned(const void* a, const void* b, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace gsat

using namespace gsat;

extern "C" {

int64_t gsat_f1_sparsity_block_entries(void) { return 4 * F1B; }
int64_t gsat_f1_sparsity_max_blocks(void) { return F1_MAX_BLOCKS; }

int gsat_f1_sparsity_fwd(const float* p, const float* y, int64_t M, const int32_t* m_valid_dev, float* partial /* [1024] */, float* loss,
                         float* stats /* [8] */, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M > 0 && p && y && partial && loss && stats, GSAT_ERR_ARG, "gsat_f1_sparsity_fwd: bad argument (mean over an empty set)");
    GSAT_REQUIRE(f1_aligned(partial, nullptr), GSAT_ERR_ARG, "gsat_f1_sparsity_fwd: partial must be 16-byte aligned");
    int nb = (int)std::min<int64_t>(F1_MAX_BLOCKS, ceil_div(M, 4 * F1B));
    const int64_t per_block = ceil_div(ceil_div(M, nb), 4) * 4;
    nb = (int)ceil_div(M, per_block);
    if (f1_aligned(p, y)) k_f1_partial<true><<<nb, F1B, 0, stream>>>(p, y, M, per_block, m_valid_dev, (float4*)partial);
    else k_f1_partial<false><<<nb, F1B, 0, stream>>>(p, y, M, per_block, m_valid_dev, (float4*)partial);
    k_f1_final<<<1, F1B, 0, stream>>>((const float4*)partial, nb, M, m_valid_dev, loss, stats);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_f1_sparsity_bwd(const float* p, const float* y, const float* stats, const float* gout, int64_t M, const int32_t* m_valid_dev,
                         float* dp, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M > 0 && p && y && stats && gout && dp, GSAT_ERR_ARG, "gsat_f1_sparsity_bwd: bad argument");
    const unsigned grid = (unsigned)ceil_div(M, 4 * F1B);
    if (f1_aligned(p, y, dp)) k_f1_bwd<true><<<grid, F1B, 0, stream>>>(p, y, stats, gout, M, m_valid_dev, dp);
    else k_f1_bwd<false><<<grid, F1B, 0, stream>>>(p, y, stats, gout, M, m_valid_dev, dp);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
