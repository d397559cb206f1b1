// Small per-edge / per-node operators of the GSAT step: concrete & Gumbel-sigmoid samplers,
// node->edge lift, reverse-edge symmetrisation and the KL "info" loss, forward and backward.
// All are single coalesced passes (4-12 B/edge); reductions are two-stage and order-fixed.
#include "common.h"

namespace gsat {

constexpr int EB = 256;

// mode 0: sigmoid(z/temp); 1: concrete  z + log u - log(1-u); 2: gumbel  z - log(-log(U+eps)+eps)
__global__ void k_sample_fwd(const float* __restrict__ z, const float* __restrict__ noise, int mode, float temp, float eps,
                             int64_t M, float* __restrict__ att) {
    int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float t = z[m];
    if (mode == 1) { float u = noise[m]; t += logf(u) - logf(1.0f - u); }
    else if (mode == 2) { float u = noise[m]; t += -logf(-logf(u + eps) + eps); }
    att[m] = 1.f / (1.f + expf(-t / temp));
}

__global__ void k_sample_bwd(const float* __restrict__ att, const float* __restrict__ datt, float temp, int64_t M, float* __restrict__ dz) {
    int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float a = att[m];
    dz[m] = datt[m] * a * (1.f - a) / temp;
}

// Gumbel-sigmoid whose uniform is drawn here: rows 4q .. 4q+3 take the words x, y, z, w of ONE Philox call (stream 5, counter q), mapped
// to [0, 1) at 24 bits like torch.rand.  gumbel_uniform4 is shared with the reporter kernel, so the two cannot drift apart.
__device__ __forceinline__ float4 gumbel_uniform4(uint64_t seed, int64_t q) {
    const uint4 r = philox4x32(seed, (uint32_t)q, 0u, 5u, 0x5A17u);
    const float k = 1.0f / 16777216.0f;
    return make_float4((float)(r.x >> 8) * k, (float)(r.y >> 8) * k, (float)(r.z >> 8) * k, (float)(r.w >> 8) * k);
}

// the expression of k_sample_fwd mode 2, operation for operation (the results are compared bitwise)
__device__ __forceinline__ float gumbel_sigmoid1(float z, float u, float temp, float eps) {
    float t = z;
    t += -logf(-logf(u + eps) + eps);
    return 1.f / (1.f + expf(-t / temp));
}

// four entries per thread; VEC (z and att 16-byte aligned): one 16-byte load and store when all four are in range
template <bool VEC>
__global__ __launch_bounds__(EB) void k_gumbel_sigmoid_philox(const float* __restrict__ z, int64_t M, float temp, float eps, SeedRef seed,
                                                              float* __restrict__ att) {
    const int64_t q = (int64_t)blockIdx.x * EB + threadIdx.x, m = 4 * q;
    if (m >= M) return;
    const float4 u = gumbel_uniform4(seed.get(), q);
    if (VEC && m + 4 <= M) {
        const float4 a = ld4(z + m);
        st4(att + m, make_float4(gumbel_sigmoid1(a.x, u.x, temp, eps), gumbel_sigmoid1(a.y, u.y, temp, eps),
                                 gumbel_sigmoid1(a.z, u.z, temp, eps), gumbel_sigmoid1(a.w, u.w, temp, eps)));
    } else {
        att[m] = gumbel_sigmoid1(z[m], u.x, temp, eps);
        if (m + 1 < M) att[m + 1] = gumbel_sigmoid1(z[m + 1], u.y, temp, eps);
        if (m + 2 < M) att[m + 2] = gumbel_sigmoid1(z[m + 2], u.z, temp, eps);
        if (m + 3 < M) att[m + 3] = gumbel_sigmoid1(z[m + 3], u.w, temp, eps);
    }
}

__global__ __launch_bounds__(EB) void k_philox_gumbel_noise(uint64_t seed, int64_t M, float* __restrict__ U) {
    const int64_t q = (int64_t)blockIdx.x * EB + threadIdx.x, m = 4 * q;
    if (m >= M) return;
    const float4 u = gumbel_uniform4(seed, q);
    U[m] = u.x;
    if (m + 1 < M) U[m + 1] = u.y;
    if (m + 2 < M) U[m + 2] = u.z;
    if (m + 3 < M) U[m + 3] = u.w;
}

__global__ void k_lift_fwd(const float* __restrict__ a, const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t E,
                           float* __restrict__ out) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) out[e] = a[src[e]] * a[dst[e]];
}

// da[n] = sum_{k in out(n)} dout[eid]*a[dst] + sum_{k in in(n)} dout[eid]*a[src]   (out-edges first, CSR order)
__global__ void k_lift_bwd(const float* __restrict__ a, const float* __restrict__ dout, const int32_t* __restrict__ rp_src,
                           const int32_t* __restrict__ dst_by_src, const int32_t* __restrict__ eid_by_src,
                           const int32_t* __restrict__ rp_dst, const int32_t* __restrict__ src_by_dst,
                           const int32_t* __restrict__ eid_by_dst, int64_t N, float* __restrict__ da) {
    int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float acc = 0.f;
    for (int k = rp_src[n]; k < rp_src[n + 1]; ++k) acc = fmaf(dout[eid_by_src[k]], a[dst_by_src[k]], acc);
    for (int k = rp_dst[n]; k < rp_dst[n + 1]; ++k) acc = fmaf(dout[eid_by_dst[k]], a[src_by_dst[k]], acc);
    da[n] = acc;
}

// out[k] = (a[k] + a[rev[k]]) / 2 ; rev is an involution so the same kernel is its own backward
__global__ void k_symmetrise(const float* __restrict__ a, const int32_t* __restrict__ rev, const int32_t* __restrict__ flag, int64_t E,
                             float* __restrict__ out) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const bool sym = flag == nullptr || flag[0] != 0;       // device-side `if is_undirected(...)`: no host round trip
    out[e] = sym ? (a[e] + a[rev[e]]) / 2.f : a[e];
}

__device__ __forceinline__ float info_term(float a, float r) {
    return a * logf(a / r + 1e-6f) + (1.f - a) * logf((1.f - a) / (1.f - r + 1e-6f) + 1e-6f);
}
__device__ __forceinline__ float info_dterm(float a, float r) {
    const float q = 1.f - r + 1e-6f;
    const float t1 = a / r + 1e-6f, t2 = (1.f - a) / q + 1e-6f;
    return logf(t1) + a / (r * t1) - logf(t2) - (1.f - a) / (q * t2);
}

// entries that count: all M, or the first *m_valid (clamped to [0, M]) of a fixed-capacity batch
__device__ __forceinline__ int64_t counted_entries(const int32_t* __restrict__ m_valid, int64_t M) {
    return m_valid ? min<int64_t>(max<int64_t>(*m_valid, 0), M) : M;
}

// block partial sums of the info-loss terms; partial[b] in block order.  r_dev (one device float) overrides r_scalar.
__global__ __launch_bounds__(EB) void k_info_partial(const float* __restrict__ att, const float* __restrict__ r_vec, float r_scalar,
                                                     int64_t M, int64_t per_block, float* __restrict__ partial,
                                                     const int32_t* __restrict__ m_valid = nullptr, const float* __restrict__ r_dev = nullptr) {
    __shared__ float sm[EB];
    const int64_t beg = (int64_t)blockIdx.x * per_block, end = min(counted_entries(m_valid, M), beg + per_block);
    if (r_dev) r_scalar = *r_dev;
    float acc = 0.f;
    for (int64_t m = beg + threadIdx.x; m < end; m += EB) acc += info_term(att[m], r_vec ? r_vec[m] : r_scalar);
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int s = EB / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sm[0];
}

__global__ __launch_bounds__(EB) void k_info_final(const float* __restrict__ partial, int nb, float inv_m, float* __restrict__ out,
                                                   const int32_t* __restrict__ m_valid = nullptr, int64_t M = 0) {
    __shared__ float sm[EB];
    if (m_valid) inv_m = 1.f / (float)max<int64_t>(counted_entries(m_valid, M), 1);
    float acc = 0.f;
    for (int i = threadIdx.x; i < nb; i += EB) acc += partial[i];
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int s = EB / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sm[0] * inv_m;
}

__global__ void k_info_bwd(const float* __restrict__ att, const float* __restrict__ r_vec, float r_scalar, const float* __restrict__ gout,
                           int64_t M, float inv_m, float* __restrict__ datt, const int32_t* __restrict__ m_valid = nullptr,
                           const float* __restrict__ r_dev = nullptr) {
    int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int64_t counted = counted_entries(m_valid, M);
    if (m_valid) inv_m = 1.f / (float)max<int64_t>(counted, 1);
    if (r_dev) r_scalar = *r_dev;
    datt[m] = m < counted ? gout[0] * inv_m * info_dterm(att[m], r_vec ? r_vec[m] : r_scalar) : 0.f;
}

__global__ void k_narrow(const int64_t* __restrict__ in, int64_t n, int32_t* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int32_t)in[i];
}

}  // namespace gsat

using namespace gsat;
#define GRID1(n) (unsigned)ceil_div((n), EB), EB, 0, stream

extern "C" {

int gsat_sample_fwd(const float* logits, const float* noise, int mode, float temp, float eps, int64_t M, float* att, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M >= 0 && mode >= 0 && mode <= 2 && temp > 0.f, GSAT_ERR_ARG, "gsat_sample_fwd: bad argument");
    if (M == 0) return GSAT_OK;
    GSAT_REQUIRE(logits && att && (mode == 0 || noise), GSAT_ERR_ARG, "gsat_sample_fwd: null pointer");
    k_sample_fwd<<<GRID1(M)>>>(logits, noise, mode, temp, eps, M, att);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_sample_bwd(const float* att, const float* datt, float temp, int64_t M, float* dlogits, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M >= 0 && temp > 0.f, GSAT_ERR_ARG, "gsat_sample_bwd: bad argument");
    if (M == 0) return GSAT_OK;
    GSAT_REQUIRE(att && datt && dlogits, GSAT_ERR_ARG, "gsat_sample_bwd: null pointer");
    k_sample_bwd<<<GRID1(M)>>>(att, datt, temp, M, dlogits);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_gumbel_sigmoid_philox(const float* logits, int64_t M, float tau, float eps, uint64_t seed, const uint64_t* seed_dev, float* att,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M >= 0 && M < (1ll << 31) && tau > 0.f, GSAT_ERR_ARG, "gsat_gumbel_sigmoid_philox: bad argument");
    if (M == 0) return GSAT_OK;
    GSAT_REQUIRE(logits && att, GSAT_ERR_ARG, "gsat_gumbel_sigmoid_philox: null pointer");
    const SeedRef ref{seed, seed_dev};
    if ((((uintptr_t)logits | (uintptr_t)att) & 15) == 0) k_gumbel_sigmoid_philox<true><<<GRID1(ceil_div(M, 4))>>>(logits, M, tau, eps, ref, att);
    else k_gumbel_sigmoid_philox<false><<<GRID1(ceil_div(M, 4))>>>(logits, M, tau, eps, ref, att);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_philox_gumbel_noise(uint64_t seed, int64_t M, float* U, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M >= 0 && M < (1ll << 31), GSAT_ERR_ARG, "gsat_philox_gumbel_noise: bad M");
    if (M == 0) return GSAT_OK;
    GSAT_REQUIRE(U, GSAT_ERR_ARG, "gsat_philox_gumbel_noise: null pointer");
    k_philox_gumbel_noise<<<GRID1(ceil_div(M, 4))>>>(seed, M, U);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_lift_fwd(const float* node_att, const int32_t* src, const int32_t* dst, int64_t E, float* edge_att, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0, GSAT_ERR_ARG, "gsat_lift_fwd: bad E");
    if (E == 0) return GSAT_OK;
    GSAT_REQUIRE(node_att && src && dst && edge_att, GSAT_ERR_ARG, "gsat_lift_fwd: null pointer");
    k_lift_fwd<<<GRID1(E)>>>(node_att, src, dst, E, edge_att);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_lift_bwd(const float* node_att, const float* dedge_att, const int32_t* rowptr_src, const int32_t* dst_by_src,
                  const int32_t* eid_by_src, const int32_t* rowptr_dst, const int32_t* src_by_dst, const int32_t* eid_by_dst,
                  int64_t N, float* dnode_att, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(N >= 0, GSAT_ERR_ARG, "gsat_lift_bwd: bad N");
    if (N == 0) return GSAT_OK;
    GSAT_REQUIRE(node_att && dedge_att && rowptr_src && dst_by_src && eid_by_src && rowptr_dst && src_by_dst && eid_by_dst && dnode_att,
                 GSAT_ERR_ARG, "gsat_lift_bwd: null pointer");
    k_lift_bwd<<<GRID1(N)>>>(node_att, dedge_att, rowptr_src, dst_by_src, eid_by_src, rowptr_dst, src_by_dst, eid_by_dst, N, dnode_att);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_symmetrise(const float* att, const int32_t* rev, const int32_t* undirected_flag, int64_t E, float* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0, GSAT_ERR_ARG, "gsat_symmetrise: bad E");
    if (E == 0) return GSAT_OK;
    GSAT_REQUIRE(att && rev && out, GSAT_ERR_ARG, "gsat_symmetrise: null pointer");
    k_symmetrise<<<GRID1(E)>>>(att, rev, undirected_flag, E, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_info_loss_fwd(const float* att, const float* r_vec, float r_scalar, int64_t M, float* partial /* [1024] */, float* out,
                       void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M > 0 && att && partial && out, GSAT_ERR_ARG, "gsat_info_loss_fwd: bad argument (mean over an empty set)");
    int nb = (int)std::min<int64_t>(1024, ceil_div(M, EB * 4));
    int64_t per_block = ceil_div(M, nb);
    nb = (int)ceil_div(M, per_block);
    k_info_partial<<<nb, EB, 0, stream>>>(att, r_vec, r_scalar, M, per_block, partial);
    k_info_final<<<1, EB, 0, stream>>>(partial, nb, 1.f / (float)M, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_info_loss_bwd(const float* att, const float* r_vec, float r_scalar, const float* gout, int64_t M, float* datt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M > 0 && att && gout && datt, GSAT_ERR_ARG, "gsat_info_loss_bwd: bad argument");
    k_info_bwd<<<GRID1(M)>>>(att, r_vec, r_scalar, gout, M, 1.f / (float)M, datt);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_info_loss_valid_fwd(const float* att, const float* r_vec, float r_scalar, const float* r_dev, int64_t M, const int32_t* m_valid_dev,
                             float* partial /* [1024] */, float* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M > 0 && att && partial && out && m_valid_dev, GSAT_ERR_ARG, "gsat_info_loss_valid_fwd: bad argument");
    int nb = (int)std::min<int64_t>(1024, ceil_div(M, EB * 4));
    int64_t per_block = ceil_div(M, nb);
    nb = (int)ceil_div(M, per_block);
    k_info_partial<<<nb, EB, 0, stream>>>(att, r_vec, r_scalar, M, per_block, partial, m_valid_dev, r_dev);
    k_info_final<<<1, EB, 0, stream>>>(partial, nb, 0.f, out, m_valid_dev, M);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_info_loss_valid_bwd(const float* att, const float* r_vec, float r_scalar, const float* r_dev, const float* gout, int64_t M,
                             const int32_t* m_valid_dev, float* datt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M > 0 && att && gout && datt && m_valid_dev, GSAT_ERR_ARG, "gsat_info_loss_valid_bwd: bad argument");
    k_info_bwd<<<GRID1(M)>>>(att, r_vec, r_scalar, gout, M, 0.f, datt, m_valid_dev, r_dev);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_narrow_i64(const int64_t* in, int64_t n, int32_t* out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(n >= 0, GSAT_ERR_ARG, "gsat_narrow_i64: bad n");
    if (n == 0) return GSAT_OK;
    GSAT_REQUIRE(in && out, GSAT_ERR_ARG, "gsat_narrow_i64: null pointer");
    k_narrow<<<GRID1(n)>>>(in, n, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Device-side batch assembly (PyG Batch.from_data_list, src/utils/get_data_loaders.py:130-145): the dataset stays packed
// in HBM (all graphs' nodes / edges concatenated, local node ids); a batch is a list of graph ids.
// ------------------------------------------------------------------------------------------------
namespace gsat {

__device__ __forceinline__ int seg_of(const int64_t* __restrict__ ptr, int nseg, int64_t i) {   // ptr[s] <= i < ptr[s+1]
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (ptr[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void k_collate_nodes(const int64_t* __restrict__ ids, const int64_t* __restrict__ node_ptr_all,
                                const int64_t* __restrict__ out_node_ptr, int G, int64_t N, int64_t* __restrict__ batch,
                                int64_t* __restrict__ node_src_row) {
    int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int g = seg_of(out_node_ptr, G, n);
    batch[n] = g;
    node_src_row[n] = node_ptr_all[ids[g]] + (n - out_node_ptr[g]);
}

__global__ void k_collate_edges(const int64_t* __restrict__ ids, const int64_t* __restrict__ edge_ptr_all,
                                const int64_t* __restrict__ out_edge_ptr, const int64_t* __restrict__ out_node_ptr,
                                const int64_t* __restrict__ edge_local_all, int64_t E_all, int G, int64_t E,
                                int64_t* __restrict__ edge_index, int64_t* __restrict__ edge_src_slot) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int g = seg_of(out_edge_ptr, G, e);
    const int64_t slot = edge_ptr_all[ids[g]] + (e - out_edge_ptr[g]);
    const int64_t off = out_node_ptr[g];
    edge_src_slot[e] = slot;
    edge_index[e] = edge_local_all[slot] + off;
    edge_index[E + e] = edge_local_all[E_all + slot] + off;
}

// Fixed-capacity batch: the real part as k_collate_*, then padding nodes (graph id G, source row -1) and a symmetric padding edge set
// among them (source slot -1).  Thread i takes node row i and edge slot i; thread 0 writes valid = (N_real, E_real, G, overflow).
// A batch that does not fit (fewer than two padding nodes left, or more edges than slots) becomes all padding with overflow = 1.
// Graphs without rows are skipped by seg_of and their ids never read, which is what lets trailing slots stay empty (k_ragged_scan).
__global__ void k_collate_padded(const int64_t* __restrict__ ids, const int64_t* __restrict__ node_ptr_all,
                                 const int64_t* __restrict__ edge_ptr_all, const int64_t* __restrict__ edge_local_all, int64_t E_all,
                                 const int64_t* __restrict__ out_node_ptr, const int64_t* __restrict__ out_edge_ptr, int G, int64_t N_cap,
                                 int64_t E_cap, int64_t* __restrict__ batch, int64_t* __restrict__ node_src_row,
                                 int64_t* __restrict__ edge_index, int64_t* __restrict__ edge_src_slot, int32_t* __restrict__ valid,
                                 const int64_t* __restrict__ ragged) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t N = out_node_ptr[G], E = out_edge_ptr[G];
    const bool overflow = N + 2 > N_cap || E > E_cap || (ragged && ragged[1] != 0);
    if (overflow) N = E = 0;
    if (i == 0) {
        // a ragged batch (ragged != NULL: filled slots, spoiled) counts its filled slots, none when it overflowed
        const int32_t graphs = ragged ? (overflow ? 0 : (int32_t)min<int64_t>(max<int64_t>(ragged[0], 0), G)) : G;
        valid[0] = (int32_t)N; valid[1] = (int32_t)E; valid[2] = graphs; valid[3] = overflow ? 1 : 0;
    }
    if (i < N_cap) {
        if (i < N) {
            const int g = seg_of(out_node_ptr, G, i);
            batch[i] = g;
            node_src_row[i] = node_ptr_all[ids[g]] + (i - out_node_ptr[g]);
        } else {
            batch[i] = G;
            node_src_row[i] = -1;
        }
    }
    if (i < E_cap) {
        if (i < E) {
            const int g = seg_of(out_edge_ptr, G, i);
            const int64_t slot = edge_ptr_all[ids[g]] + (i - out_edge_ptr[g]);
            const int64_t off = out_node_ptr[g];
            edge_src_slot[i] = slot;
            edge_index[i] = edge_local_all[slot] + off;
            edge_index[E_cap + i] = edge_local_all[E_all + slot] + off;
        } else {
            int64_t src, dst;                        // the padding rule (common.h), shared with gsat_subgraph_padded
            padding_edge(N, N_cap - N, E_cap - E, i - E, src, dst);
            edge_src_slot[i] = -1;
            edge_index[i] = src;
            edge_index[E_cap + i] = dst;
        }
    }
}

// The scans of a ragged batch in ONE block: slot i of ids holds a graph id or, negative, nothing.  out_node_ptr / out_edge_ptr [B + 1]
// are the exclusive scans of the slots' node / edge counts with empty slots counting 0, safe_ids the ids with 0 in the empty slots,
// empty[i] = 1 for an empty slot, state = (filled slots, spoiled): spoiled when a filled slot follows an empty one or an id is not
// below G_all (such a slot counts nothing and is never looked up).  Chunks of RSB slots, a Hillis-Steele scan in LDS per chunk and a
// running carry: integer sums, so the order does not matter.
constexpr int RSB = 256;

__global__ __launch_bounds__(RSB) void k_ragged_scan(const int64_t* __restrict__ ids, int B, const int64_t* __restrict__ node_ptr_all,
                                                     const int64_t* __restrict__ edge_ptr_all, int64_t G_all,
                                                     int64_t* __restrict__ out_node_ptr, int64_t* __restrict__ out_edge_ptr,
                                                     int64_t* __restrict__ state, int64_t* __restrict__ safe_ids,
                                                     uint8_t* __restrict__ empty) {
    __shared__ int64_t sn[RSB], se[RSB];
    __shared__ int s_filled, s_first_empty, s_last_filled, s_bad;
    const int t = threadIdx.x;
    if (t == 0) { s_filled = 0; s_first_empty = 0x7fffffff; s_last_filled = -1; s_bad = 0; }
    int64_t carry_n = 0, carry_e = 0;
    int filled = 0, first_empty = 0x7fffffff, last_filled = -1, bad = 0;
    for (int base = 0; base < B; base += RSB) {
        const int i = base + t;
        int64_t n = 0, e = 0;
        if (i < B) {
            const int64_t id = ids[i];
            const bool ok = id >= 0 && id < G_all;
            if (ok) {
                n = node_ptr_all[id + 1] - node_ptr_all[id];
                e = edge_ptr_all[id + 1] - edge_ptr_all[id];
            }
            if (id >= 0) { ++filled; last_filled = i; } else { first_empty = min(first_empty, i); }
            if (id >= G_all) bad = 1;
            safe_ids[i] = ok ? id : 0;
            empty[i] = id < 0 ? 1 : 0;
        }
        __syncthreads();                                    // the previous chunk's totals have been read
        sn[t] = n; se[t] = e;
        __syncthreads();
        for (int o = 1; o < RSB; o <<= 1) {
            const int64_t a = t >= o ? sn[t - o] : 0, b = t >= o ? se[t - o] : 0;
            __syncthreads();
            sn[t] += a; se[t] += b;
            __syncthreads();
        }
        if (i < B) { out_node_ptr[i + 1] = carry_n + sn[t]; out_edge_ptr[i + 1] = carry_e + se[t]; }
        carry_n += sn[RSB - 1]; carry_e += se[RSB - 1];
    }
    __syncthreads();
    atomicAdd(&s_filled, filled);                           // integer LDS atomics: any order gives the same result
    atomicMin(&s_first_empty, first_empty);
    atomicMax(&s_last_filled, last_filled);
    atomicOr(&s_bad, bad);
    __syncthreads();
    if (t == 0) {
        out_node_ptr[0] = 0; out_edge_ptr[0] = 0;
        state[0] = s_filled;
        state[1] = (s_bad || s_last_filled > s_first_empty) ? 1 : 0;
    }
}

// k_ragged_scan for a primal / dual pair: a third scan (the slots' dual edge counts) and the JOINT verdict.  spoiled is also set when
// the totals break N + 2 <= N_cap, E <= E_cap or E_dual <= E_dual_cap, so both collations of the pair -- the dual side's node scan is
// out_edge_ptr -- read one state and overflow together.  Every thread ends the loop with the three totals in its carries.
__global__ __launch_bounds__(RSB) void k_ragged_pair_scan(const int64_t* __restrict__ ids, int B, const int64_t* __restrict__ node_ptr_all,
                                                          const int64_t* __restrict__ edge_ptr_all,
                                                          const int64_t* __restrict__ dual_edge_ptr_all, int64_t G_all, int64_t N_cap,
                                                          int64_t E_cap, int64_t Ed_cap, int64_t* __restrict__ out_node_ptr,
                                                          int64_t* __restrict__ out_edge_ptr, int64_t* __restrict__ out_dual_edge_ptr,
                                                          int64_t* __restrict__ state, int64_t* __restrict__ safe_ids,
                                                          uint8_t* __restrict__ empty) {
    __shared__ int64_t sn[RSB], se[RSB], sd[RSB];
    __shared__ int s_filled, s_first_empty, s_last_filled, s_bad;
    const int t = threadIdx.x;
    if (t == 0) { s_filled = 0; s_first_empty = 0x7fffffff; s_last_filled = -1; s_bad = 0; }
    int64_t carry_n = 0, carry_e = 0, carry_d = 0;
    int filled = 0, first_empty = 0x7fffffff, last_filled = -1, bad = 0;
    for (int base = 0; base < B; base += RSB) {
        const int i = base + t;
        int64_t n = 0, e = 0, d = 0;
        if (i < B) {
            const int64_t id = ids[i];
            const bool ok = id >= 0 && id < G_all;
            if (ok) {
                n = node_ptr_all[id + 1] - node_ptr_all[id];
                e = edge_ptr_all[id + 1] - edge_ptr_all[id];
                d = dual_edge_ptr_all[id + 1] - dual_edge_ptr_all[id];
            }
            if (id >= 0) { ++filled; last_filled = i; } else { first_empty = min(first_empty, i); }
            if (id >= G_all) bad = 1;
            safe_ids[i] = ok ? id : 0;
            empty[i] = id < 0 ? 1 : 0;
        }
        __syncthreads();                                    // the previous chunk's totals have been read
        sn[t] = n; se[t] = e; sd[t] = d;
        __syncthreads();
        for (int o = 1; o < RSB; o <<= 1) {
            const int64_t a = t >= o ? sn[t - o] : 0, b = t >= o ? se[t - o] : 0, c = t >= o ? sd[t - o] : 0;
            __syncthreads();
            sn[t] += a; se[t] += b; sd[t] += c;
            __syncthreads();
        }
        if (i < B) {
            out_node_ptr[i + 1] = carry_n + sn[t]; out_edge_ptr[i + 1] = carry_e + se[t]; out_dual_edge_ptr[i + 1] = carry_d + sd[t];
        }
        carry_n += sn[RSB - 1]; carry_e += se[RSB - 1]; carry_d += sd[RSB - 1];
    }
    __syncthreads();
    atomicAdd(&s_filled, filled);                           // integer LDS atomics: any order gives the same result
    atomicMin(&s_first_empty, first_empty);
    atomicMax(&s_last_filled, last_filled);
    atomicOr(&s_bad, bad);
    __syncthreads();
    if (t == 0) {
        out_node_ptr[0] = 0; out_edge_ptr[0] = 0; out_dual_edge_ptr[0] = 0;
        const bool fits = carry_n + 2 <= N_cap && carry_e <= E_cap && carry_d <= Ed_cap;
        state[0] = s_filled;
        state[1] = (s_bad || s_last_filled > s_first_empty || !fits) ? 1 : 0;
    }
}

}  // namespace gsat

extern "C" {

int gsat_ragged_scan(const int64_t* graph_ids, int64_t num_slots, const int64_t* node_ptr_all, const int64_t* edge_ptr_all,
                     int64_t num_graphs_all, int64_t* out_node_ptr, int64_t* out_edge_ptr, int64_t* state, int64_t* safe_ids,
                     uint8_t* empty, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(num_slots >= 1 && num_slots < (1ll << 31) - 1 && num_graphs_all >= 0, GSAT_ERR_ARG, "gsat_ragged_scan: bad extents");
    GSAT_REQUIRE(graph_ids && node_ptr_all && edge_ptr_all && out_node_ptr && out_edge_ptr && state && safe_ids && empty, GSAT_ERR_ARG,
                 "gsat_ragged_scan: null pointer");
    gsat::k_ragged_scan<<<1, gsat::RSB, 0, stream>>>(graph_ids, (int)num_slots, node_ptr_all, edge_ptr_all, num_graphs_all, out_node_ptr,
                                                     out_edge_ptr, state, safe_ids, empty);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_ragged_pair_scan(const int64_t* graph_ids, int64_t num_slots, const int64_t* node_ptr_all, const int64_t* edge_ptr_all,
                          const int64_t* dual_edge_ptr_all, int64_t num_graphs_all, int64_t N_cap, int64_t E_cap, int64_t E_dual_cap,
                          int64_t* out_node_ptr, int64_t* out_edge_ptr, int64_t* out_dual_edge_ptr, int64_t* state, int64_t* safe_ids,
                          uint8_t* empty, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(num_slots >= 1 && num_slots < (1ll << 31) - 1 && num_graphs_all >= 0, GSAT_ERR_ARG, "gsat_ragged_pair_scan: bad extents");
    GSAT_REQUIRE(N_cap >= 2 && N_cap < (1ll << 31) && E_cap >= 0 && E_cap < (1ll << 31) - 2 && E_dual_cap >= 0 && E_dual_cap < (1ll << 31),
                 GSAT_ERR_ARG, "gsat_ragged_pair_scan: bad capacity (two padding nodes; the dual node capacity E_cap + 2 stays below 2^31)");
    GSAT_REQUIRE(graph_ids && node_ptr_all && edge_ptr_all && dual_edge_ptr_all && out_node_ptr && out_edge_ptr && out_dual_edge_ptr &&
                 state && safe_ids && empty, GSAT_ERR_ARG, "gsat_ragged_pair_scan: null pointer");
    gsat::k_ragged_pair_scan<<<1, gsat::RSB, 0, stream>>>(graph_ids, (int)num_slots, node_ptr_all, edge_ptr_all, dual_edge_ptr_all,
                                                          num_graphs_all, N_cap, E_cap, E_dual_cap, out_node_ptr, out_edge_ptr,
                                                          out_dual_edge_ptr, state, safe_ids, empty);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

static int collate_padded_impl(const char* name, const int64_t* graph_ids, int64_t num_graphs, const int64_t* ragged_state,
                               const int64_t* node_ptr_all, const int64_t* edge_ptr_all, const int64_t* edge_local_all, int64_t num_edges_all,
                               const int64_t* out_node_ptr, const int64_t* out_edge_ptr, int64_t N_cap, int64_t E_cap, int64_t* batch,
                               int64_t* node_src_row, int64_t* edge_index, int64_t* edge_src_slot, int32_t* valid, hipStream_t stream) {
    GSAT_REQUIRE(num_graphs >= 1 && num_graphs < (1ll << 31) - 1 && N_cap >= 2 && N_cap < (1ll << 31) && E_cap >= 0 && E_cap < (1ll << 31),
                 GSAT_ERR_ARG, "%s: bad extents (at least one graph, two padding nodes)", name);
    GSAT_REQUIRE(graph_ids && node_ptr_all && edge_ptr_all && out_node_ptr && out_edge_ptr && batch && node_src_row && valid &&
                 (E_cap == 0 || (edge_local_all && edge_index && edge_src_slot)), GSAT_ERR_ARG, "%s: null pointer", name);
    gsat::k_collate_padded<<<GRID1(std::max(N_cap, E_cap))>>>(graph_ids, node_ptr_all, edge_ptr_all, edge_local_all, num_edges_all, out_node_ptr,
                                                              out_edge_ptr, (int)num_graphs, N_cap, E_cap, batch, node_src_row, edge_index,
                                                              edge_src_slot, valid, ragged_state);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_collate_padded(const int64_t* graph_ids, int64_t num_graphs, const int64_t* node_ptr_all, const int64_t* edge_ptr_all,
                        const int64_t* edge_local_all, int64_t num_edges_all, const int64_t* out_node_ptr, const int64_t* out_edge_ptr,
                        int64_t N_cap, int64_t E_cap, int64_t* batch, int64_t* node_src_row, int64_t* edge_index, int64_t* edge_src_slot,
                        int32_t* valid, void* stream_) {
    return collate_padded_impl("gsat_collate_padded", graph_ids, num_graphs, nullptr, node_ptr_all, edge_ptr_all, edge_local_all, num_edges_all,
                               out_node_ptr, out_edge_ptr, N_cap, E_cap, batch, node_src_row, edge_index, edge_src_slot, valid,
                               (hipStream_t)stream_);
}

int gsat_collate_padded_ragged(const int64_t* graph_ids, int64_t num_graphs, const int64_t* ragged_state, const int64_t* node_ptr_all,
                               const int64_t* edge_ptr_all, const int64_t* edge_local_all, int64_t num_edges_all,
                               const int64_t* out_node_ptr, const int64_t* out_edge_ptr, int64_t N_cap, int64_t E_cap, int64_t* batch,
                               int64_t* node_src_row, int64_t* edge_index, int64_t* edge_src_slot, int32_t* valid, void* stream_) {
    GSAT_REQUIRE(ragged_state, GSAT_ERR_ARG, "gsat_collate_padded_ragged: null pointer");
    return collate_padded_impl("gsat_collate_padded_ragged", graph_ids, num_graphs, ragged_state, node_ptr_all, edge_ptr_all, edge_local_all,
                               num_edges_all, out_node_ptr, out_edge_ptr, N_cap, E_cap, batch, node_src_row, edge_index, edge_src_slot, valid,
                               (hipStream_t)stream_);
}

int gsat_collate(const int64_t* graph_ids, int64_t num_graphs, const int64_t* node_ptr_all, const int64_t* edge_ptr_all,
                 const int64_t* edge_local_all, int64_t num_edges_all, const int64_t* out_node_ptr, const int64_t* out_edge_ptr,
                 int64_t N, int64_t E, int64_t* batch, int64_t* node_src_row, int64_t* edge_index, int64_t* edge_src_slot, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(num_graphs >= 0 && num_graphs < (1ll << 31) && N >= 0 && E >= 0, GSAT_ERR_ARG, "gsat_collate: bad extents");
    if (num_graphs == 0) return GSAT_OK;
    GSAT_REQUIRE(graph_ids && node_ptr_all && edge_ptr_all && out_node_ptr && out_edge_ptr, GSAT_ERR_ARG, "gsat_collate: null pointer");
    if (N > 0) {
        GSAT_REQUIRE(batch && node_src_row, GSAT_ERR_ARG, "gsat_collate: null node outputs");
        gsat::k_collate_nodes<<<GRID1(N)>>>(graph_ids, node_ptr_all, out_node_ptr, (int)num_graphs, N, batch, node_src_row);
    }
    if (E > 0) {
        GSAT_REQUIRE(edge_local_all && edge_index && edge_src_slot, GSAT_ERR_ARG, "gsat_collate: null edge outputs");
        gsat::k_collate_edges<<<GRID1(E)>>>(graph_ids, edge_ptr_all, out_edge_ptr, out_node_ptr, edge_local_all, num_edges_all, (int)num_graphs, E,
                                            edge_index, edge_src_slot);
    }
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// Line ("dual") graph of the fork: one dual node per DIRECTED primal edge; two dual nodes are joined, in both
// directions, when their primal edges leave the same node (src/datasets/mutag_dual.py:345-377, `group_by_first`).
// The reference builds it with O(sum deg^2) Python loops per dataset; here one kernel over the by-source CSR.
// Output order = the reference's: source nodes ascending, then pairs (i < j) in edge order, (e_i,e_j) then (e_j,e_i).
// ------------------------------------------------------------------------------------------------
namespace gsat {

__global__ void k_pair_counts(const int32_t* __restrict__ rowptr, int64_t N, int64_t* __restrict__ counts) {
    int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int64_t d = rowptr[n + 1] - rowptr[n];
    counts[n] = d * (d - 1) / 2;                       // unordered pairs of out-edges of node n
}

__global__ void k_line_graph(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ eid, const int64_t* __restrict__ pair_ptr,
                             int64_t N, int64_t num_pairs, int64_t* __restrict__ dual_edge_index) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_pairs) return;
    int64_t lo = 0, hi = N;                             // pair_ptr[lo] <= t < pair_ptr[hi]
    while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (pair_ptr[mid] <= t) lo = mid; else hi = mid;
    }
    const int beg = rowptr[lo];
    const int64_t d = rowptr[lo + 1] - beg;
    int64_t r = t - pair_ptr[lo];                       // r-th pair (i < j) in row-major order of the upper triangle
    int64_t i = 0;
    // rows of the upper triangle have d-1, d-2, ... entries: find i with prefix(i) <= r < prefix(i+1)
    {
        // prefix(i) = i*d - i*(i+1)/2 ; solve by a short binary search (d < 2^31)
        int64_t a = 0, b = d - 1;
        while (b - a > 1) {
            int64_t m = (a + b) >> 1;
            if (m * d - m * (m + 1) / 2 <= r) a = m; else b = m;
        }
        i = a;
    }
    const int64_t j = i + 1 + (r - (i * d - i * (i + 1) / 2));
    const int64_t e1 = eid[beg + i], e2 = eid[beg + j];
    const int64_t E2 = 2 * num_pairs;
    dual_edge_index[2 * t] = e1;          dual_edge_index[E2 + 2 * t] = e2;
    dual_edge_index[2 * t + 1] = e2;      dual_edge_index[E2 + 2 * t + 1] = e1;
}

}  // namespace gsat

extern "C" {

int gsat_line_graph_pair_counts(const int32_t* rowptr_src, int64_t N, int64_t* counts, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(N >= 0, GSAT_ERR_ARG, "gsat_line_graph_pair_counts: bad N");
    if (N == 0) return GSAT_OK;
    GSAT_REQUIRE(rowptr_src && counts, GSAT_ERR_ARG, "gsat_line_graph_pair_counts: null pointer");
    gsat::k_pair_counts<<<GRID1(N)>>>(rowptr_src, N, counts);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

int gsat_line_graph(const int32_t* rowptr_src, const int32_t* eid_by_src, const int64_t* pair_ptr, int64_t N, int64_t num_pairs,
                    int64_t* dual_edge_index, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(N >= 0 && num_pairs >= 0, GSAT_ERR_ARG, "gsat_line_graph: bad extents");
    if (num_pairs == 0) return GSAT_OK;
    GSAT_REQUIRE(rowptr_src && eid_by_src && pair_ptr && dual_edge_index, GSAT_ERR_ARG, "gsat_line_graph: null pointer");
    gsat::k_line_graph<<<GRID1(num_pairs)>>>(rowptr_src, eid_by_src, pair_ptr, N, num_pairs, dual_edge_index);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
