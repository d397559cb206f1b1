// Post-hoc edge-mask explainer (PyG's GNNExplainer, edge_reduction 'sum' for the size term, a mean for the entropy) around the
// mask-weighted message passing: one mask logit m per edge slot, a = sigmoid(m), and per optimisation step ONE elementwise launch that
// turns the gradient the backbone's backward left for a into the gradient of the objective, takes torch's Adam step and writes the next
// a, plus one single-thread launch that advances the step counter.  Entries at or beyond the real edge count of a padded batch are
// never loaded or written.  The per-graph objective terms and the per-graph min-max normalisation of a score vector (the reference's
// visualize_a_graph(norm=True), src/utils/utils.py:105-107) reduce in a fixed order.  No atomics anywhere: bitwise repeatable.
#include "common.h"

#include <cmath>

namespace gsat {

constexpr int MEB = 256;                 // threads per block
constexpr float ME_LOG_EPS = 1e-15f;     // PyG's EPS inside the entropy's logarithms

__device__ __forceinline__ float me_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }       // 1 / inf = 0: no NaN at any finite z

// entries that count: none of an overflowing batch
__device__ __forceinline__ int64_t me_counted(const int32_t* __restrict__ valid, int64_t E) {
    if (!valid) return E;
    return valid[3] ? 0 : min<int64_t>(max<int64_t>(valid[1], 0), E);
}
__device__ __forceinline__ int64_t me_graphs(const int32_t* __restrict__ valid, int64_t G) {
    if (!valid) return G;
    return valid[3] ? 0 : min<int64_t>(max<int64_t>(valid[2], 0), G);
}

// H(a) = -a ln(a + 1e-15) - (1 - a) ln(1 - a + 1e-15) and its derivative; both finite for every a in [0, 1]
__device__ __forceinline__ float me_entropy(float a) {
    const float c = 1.f - a;
    return -a * logf(a + ME_LOG_EPS) - c * logf(c + ME_LOG_EPS);
}
__device__ __forceinline__ float me_dentropy(float a) {
    const float c = 1.f - a;
    return -logf(a + ME_LOG_EPS) - a / (a + ME_LOG_EPS) + logf(c + ME_LOG_EPS) + c / (c + ME_LOG_EPS);
}

// 1 / (1 - b1^t) and 1 / sqrt(1 - b2^t) of step t >= 1, in fp64 from fp64 betas as torch's (non-capturable) Adam has them: with
// b2 = 0.999 rounded to fp32 first, 1 - b2^t would be off by 1e-5 of itself in the first steps
__device__ __forceinline__ void me_bias(float* __restrict__ state, int t, double b1, double b2) {
    state[0] = (float)t - 1.f;
    state[1] = (float)(1.0 / (1.0 - pow(b1, (double)t)));
    state[2] = (float)(1.0 / sqrt(1.0 - pow(b2, (double)t)));
    state[3] = 0.f;
}

// 1 / E_g of the graph of edge e's source, 1 for an edge whose ids are out of range (it is then no real edge)
__device__ __forceinline__ float me_inv_count(const int32_t* __restrict__ src32, const int32_t* __restrict__ node_seg32,
                                              const int32_t* __restrict__ edge_ptr, int64_t N, int64_t G, int64_t e) {
    const int s = src32[e];
    if (s < 0 || s >= N) return 1.f;
    const int g = node_seg32[s];
    if (g < 0 || g >= G) return 1.f;
    return 1.f / (float)max(edge_ptr[g + 1] - edge_ptr[g], 1);
}

// every slot of the capacity: m <- init or the constant, mu = nu = 0, a = sigmoid(m), inv_eg = 1 / E_g; thread 0 writes the state word
template <bool VEC>
__global__ __launch_bounds__(MEB) void k_mask_init(const float* __restrict__ init, float value, const int32_t* __restrict__ src32,
                                                   const int32_t* __restrict__ node_seg32, const int32_t* __restrict__ edge_ptr, int64_t N,
                                                   int64_t G, int64_t E, double b1, double b2, float* __restrict__ m, float* __restrict__ mu,
                                                   float* __restrict__ nu, float* __restrict__ a, float* __restrict__ inv_eg,
                                                   float* __restrict__ state) {
    if (blockIdx.x == 0 && threadIdx.x == 0) me_bias(state, 1, b1, b2);
    const int64_t i = 4 * ((int64_t)blockIdx.x * MEB + threadIdx.x);
    if (i >= E) return;
    if (VEC && i + 4 <= E) {
        const float4 v = init ? ld4(init + i) : make_float4(value, value, value, value);
        st4(m + i, v);
        st4(mu + i, f4zero());
        st4(nu + i, f4zero());
        st4(a + i, make_float4(me_sigmoid(v.x), me_sigmoid(v.y), me_sigmoid(v.z), me_sigmoid(v.w)));
        st4(inv_eg + i, make_float4(me_inv_count(src32, node_seg32, edge_ptr, N, G, i), me_inv_count(src32, node_seg32, edge_ptr, N, G, i + 1),
                                    me_inv_count(src32, node_seg32, edge_ptr, N, G, i + 2), me_inv_count(src32, node_seg32, edge_ptr, N, G, i + 3)));
    } else {
        for (int64_t k = i; k < min(i + 4, E); ++k) {
            const float v = init ? init[k] : value;
            m[k] = v; mu[k] = 0.f; nu[k] = 0.f; a[k] = me_sigmoid(v);
            inv_eg[k] = me_inv_count(src32, node_seg32, edge_ptr, N, G, k);
        }
    }
}

struct MaskHyper { float lr, b1, b2, one_minus_b1, one_minus_b2, eps, size_coef, ent_coef; };          // 1 - beta rounded once, from fp64

// one entry: the objective's gradient through the sigmoid, Adam, the next a
__device__ __forceinline__ void me_update(float& m, float& mu, float& nu, float& a, float g_a, float inv_eg, float b, float step_size,
                                          float inv_sqrt_bc2, const MaskHyper& h) {
    const float G = a * (1.f - a) * (b * g_a + h.size_coef + h.ent_coef * me_dentropy(a) * inv_eg);
    mu = h.b1 * mu + h.one_minus_b1 * G;
    nu = h.b2 * nu + h.one_minus_b2 * G * G;
    m -= step_size * mu / (sqrtf(nu) * inv_sqrt_bc2 + h.eps);
    a = me_sigmoid(m);
}

// four entries per thread; the state word is only READ here (k_mask_commit advances it in a launch of its own)
template <bool VEC>
__global__ __launch_bounds__(MEB) void k_mask_step(float* __restrict__ m, float* __restrict__ mu, float* __restrict__ nu, float* __restrict__ a,
                                                   const float* __restrict__ g_a, const float* __restrict__ inv_eg, int64_t E, int64_t G,
                                                   const int32_t* __restrict__ valid, const float* __restrict__ state, MaskHyper h) {
    const int64_t i = 4 * ((int64_t)blockIdx.x * MEB + threadIdx.x);
    if (i >= E) return;
    const int64_t mv = me_counted(valid, E);
    if (i >= mv) return;
    const float b = (float)me_graphs(valid, G), step_size = h.lr * state[1], inv_sqrt_bc2 = state[2];
    if (VEC && i + 4 <= mv) {
        float4 vm = ld4(m + i), vmu = ld4(mu + i), vnu = ld4(nu + i), va = ld4(a + i);
        const float4 vg = ld4(g_a + i), vw = ld4(inv_eg + i);
        me_update(vm.x, vmu.x, vnu.x, va.x, vg.x, vw.x, b, step_size, inv_sqrt_bc2, h);
        me_update(vm.y, vmu.y, vnu.y, va.y, vg.y, vw.y, b, step_size, inv_sqrt_bc2, h);
        me_update(vm.z, vmu.z, vnu.z, va.z, vg.z, vw.z, b, step_size, inv_sqrt_bc2, h);
        me_update(vm.w, vmu.w, vnu.w, va.w, vg.w, vw.w, b, step_size, inv_sqrt_bc2, h);
        st4(m + i, vm); st4(mu + i, vmu); st4(nu + i, vnu); st4(a + i, va);
    } else {
        for (int64_t k = i; k < min(i + 4, mv); ++k) {
            float sm = m[k], smu = mu[k], snu = nu[k], sa = a[k];
            me_update(sm, smu, snu, sa, g_a[k], inv_eg[k], b, step_size, inv_sqrt_bc2, h);
            m[k] = sm; mu[k] = smu; nu[k] = snu; a[k] = sa;
        }
    }
}

// one thread: t + 1 and the bias corrections of the step after it; an overflowing batch advances nothing
__global__ void k_mask_commit(const int32_t* __restrict__ valid, float* __restrict__ state, double b1, double b2) {
    if (valid && valid[3]) return;
    me_bias(state, (int)state[0] + 2, b1, b2);
}

// One wave per graph, four graphs per block.  Lane l takes the graph's slots l, l + 64, ... in that order, then the wave's fixed tree.
__global__ __launch_bounds__(MEB) void k_mask_objective(const float* __restrict__ a, const int32_t* __restrict__ edge_ptr,
                                                        const int32_t* __restrict__ edge_order, int64_t E, int64_t G,
                                                        const int32_t* __restrict__ valid, float* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * (MEB / 64) + (threadIdx.x >> 6);          // uniform over the wave
    if (g >= G) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f, h = 0.f;
    int n = 0;
    if (g < me_graphs(valid, G)) {
        const int64_t mv = me_counted(valid, E);
        const int beg = max(edge_ptr[g], 0), end = (int)min<int64_t>(edge_ptr[g + 1], E);          // never a slot outside edge_order
        n = max(end - beg, 0);
        for (int k = beg + lane; k < end; k += 64) {
            const int e = edge_order[k];
            if (e < 0 || e >= mv) continue;
            const float v = a[e];
            s += v;
            h += me_entropy(v);
        }
    }
    s = group_sum<64>(s);
    h = group_sum<64>(h);
    if (lane == 0) { out[2 * g] = s; out[2 * g + 1] = h / (float)max(n, 1); }
}

__device__ __forceinline__ float me_group_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float me_group_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float me_pow(float x, float p) { return p == 1.f ? x : powf(x, p); }

// One wave per graph: a pass for (min, max) of att^p over the graph's slots, a pass that writes.  A slot of a graph that does not count,
// or at or beyond the real edge count, gets 0 without a load.
__global__ __launch_bounds__(MEB) void k_segment_minmax_norm(const float* __restrict__ att, const int32_t* __restrict__ edge_ptr,
                                                             const int32_t* __restrict__ edge_order, int64_t E, int64_t G, float p,
                                                             float eps, const int32_t* __restrict__ valid, float* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * (MEB / 64) + (threadIdx.x >> 6);          // uniform over the wave
    if (g >= G) return;
    const int lane = threadIdx.x & 63;
    const int beg = max(edge_ptr[g], 0), end = (int)min<int64_t>(edge_ptr[g + 1], E);              // never a slot outside edge_order
    const int64_t mv = g < me_graphs(valid, G) ? me_counted(valid, E) : 0;
    float lo = INFINITY, hi = -INFINITY;
    for (int k = beg + lane; k < end; k += 64) {
        const int e = edge_order[k];
        if (e < 0 || e >= mv) continue;
        const float v = me_pow(att[e], p);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = me_group_min(lo);
    hi = me_group_max(hi);
    const float inv = 1.f / (hi - lo + eps);
    for (int k = beg + lane; k < end; k += 64) {
        const int e = edge_order[k];
        if (e < 0 || e >= E) continue;
        out[e] = e < mv ? (me_pow(att[e], p) - lo) * inv : 0.f;
    }
}

static inline bool me_aligned(const void* a, const void* b, const void* c, const void* d, const void* e = nullptr, const void* f = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e | (uintptr_t)f) & 15) == 0;
}

static inline const char* me_hyper_check(float lr, double b1, double b2, float eps, float size_coef, float ent_coef) {
    if (!(lr > 0.f)) return "lr must be positive";
    if (!(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0)) return "betas must lie in [0, 1)";
    if (!(eps >= 0.f)) return "eps must not be negative";
    if (!(size_coef >= 0.f && ent_coef >= 0.f)) return "coefficients must not be negative";
    return nullptr;
}

constexpr int64_t ME_MAX = (1ll << 31) - 1;

}  // namespace gsat

using namespace gsat;

extern "C" {

int gsat_mask_init(const float* init, float init_value, const int32_t* src32, const int32_t* node_seg32, const int32_t* edge_ptr, int64_t N,
                   int64_t G, int64_t E, double b1, double b2, float* m, float* mu, float* nu, float* a, float* inv_eg, float* state,
                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && N >= 0 && G >= 0 && state, GSAT_ERR_ARG, "gsat_mask_init: bad argument");
    GSAT_REQUIRE(E == 0 || (src32 && node_seg32 && edge_ptr && m && mu && nu && a && inv_eg), GSAT_ERR_ARG, "gsat_mask_init: null pointer");
    GSAT_REQUIRE(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, GSAT_ERR_ARG, "gsat_mask_init: betas must lie in [0, 1)");
    GSAT_REQUIRE(E <= ME_MAX && N <= ME_MAX && G < ME_MAX, GSAT_ERR_UNSUPPORTED, "gsat_mask_init: extents must be below 2^31");
    const unsigned grid = (unsigned)std::max<int64_t>(ceil_div(E, 4 * MEB), 1);          // E = 0: the state word alone
    if (me_aligned(m, mu, nu, a, inv_eg, init)) k_mask_init<true><<<grid, MEB, 0, stream>>>(init, init_value, src32, node_seg32, edge_ptr, N, G, E, b1, b2, m, mu, nu, a, inv_eg, state);
    else k_mask_init<false><<<grid, MEB, 0, stream>>>(init, init_value, src32, node_seg32, edge_ptr, N, G, E, b1, b2, m, mu, nu, a, inv_eg, state);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_mask_step(float* m, float* mu, float* nu, float* a, const float* g_a, const float* inv_eg, int64_t E, int64_t G,
                   const int32_t* valid, float* state, float lr, double b1, double b2, float eps, float size_coef, float ent_coef,
                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* bad = me_hyper_check(lr, b1, b2, eps, size_coef, ent_coef);
    GSAT_REQUIRE(!bad, GSAT_ERR_ARG, "gsat_mask_step: %s", bad);
    GSAT_REQUIRE(E >= 0 && G >= 0 && state, GSAT_ERR_ARG, "gsat_mask_step: bad argument");
    GSAT_REQUIRE(E == 0 || (m && mu && nu && a && g_a && inv_eg), GSAT_ERR_ARG, "gsat_mask_step: null pointer");
    GSAT_REQUIRE(E <= ME_MAX && G < ME_MAX, GSAT_ERR_UNSUPPORTED, "gsat_mask_step: extents must be below 2^31");
    if (E == 0) return GSAT_OK;
    const MaskHyper h{lr, (float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), eps, size_coef, ent_coef};
    const unsigned grid = (unsigned)ceil_div(E, 4 * MEB);
    if (me_aligned(m, mu, nu, a, g_a, inv_eg)) k_mask_step<true><<<grid, MEB, 0, stream>>>(m, mu, nu, a, g_a, inv_eg, E, G, valid, state, h);
    else k_mask_step<false><<<grid, MEB, 0, stream>>>(m, mu, nu, a, g_a, inv_eg, E, G, valid, state, h);
    k_mask_commit<<<1, 1, 0, stream>>>(valid, state, b1, b2);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_mask_objective(const float* a, const int32_t* edge_ptr, const int32_t* edge_order, int64_t E, int64_t G, const int32_t* valid,
                        float* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && G >= 0, GSAT_ERR_ARG, "gsat_mask_objective: bad argument");
    GSAT_REQUIRE(E <= ME_MAX && G < ME_MAX, GSAT_ERR_UNSUPPORTED, "gsat_mask_objective: extents must be below 2^31");
    if (G == 0) return GSAT_OK;
    GSAT_REQUIRE(edge_ptr && out && (E == 0 || (a && edge_order)), GSAT_ERR_ARG, "gsat_mask_objective: null pointer");
    k_mask_objective<<<(unsigned)ceil_div(G, MEB / 64), MEB, 0, stream>>>(a, edge_ptr, edge_order, E, G, valid, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_segment_minmax_norm(const float* att, const int32_t* edge_ptr, const int32_t* edge_order, int64_t E, int64_t G, float power,
                             float eps, const int32_t* valid, float* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && G >= 0 && power > 0.f && eps >= 0.f, GSAT_ERR_ARG, "gsat_segment_minmax_norm: bad argument (power > 0, eps >= 0)");
    GSAT_REQUIRE(E <= ME_MAX && G < ME_MAX, GSAT_ERR_UNSUPPORTED, "gsat_segment_minmax_norm: extents must be below 2^31");
    if (E == 0 || G == 0) return GSAT_OK;
    GSAT_REQUIRE(att && edge_ptr && edge_order && out, GSAT_ERR_ARG, "gsat_segment_minmax_norm: null pointer");
    k_segment_minmax_norm<<<(unsigned)ceil_div(G, MEB / 64), MEB, 0, stream>>>(att, edge_ptr, edge_order, E, G, power, eps, valid, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
