// Explanation metrics on the device: per-graph edge ranking by attention (precision@k, top-k masks), exact tie-aware ROC-AUC of the
// attention against edge labels, and the delta-KL / mean-attention statistics (replaces the host loop of src/run_gsat.py:656-668,
// 761-800).
//
// Total order of the ranking (the contract of both paths): higher attention first; equal attention -> lower edge id first; -0.0 counts
// as +0.0; NaN is unsupported.  A 64-bit key carries it in one comparison: the order-preserving bit flip of the float, inverted for
// descending order, in the high word and the EDGE ID in the low word -- keys are unique, so the result does not depend on the order in
// which `edge_order` lists a graph's edges nor on the sorting network being stable.
//
//   fused path   : one launch.  A graph of <= 64 edges is sorted by one wavefront, one key per lane, with a bitonic network on cross-lane
//                  exchanges (DPP quad permutes for strides 1/2, ds_swizzle for 4/8/16, v_permlane32_swap for 32) and no LDS; a larger
//                  graph (up to gsat_rank_edges_lds_cap() edges) by the whole workgroup with its keys in LDS, where every stage below
//                  stride 64 runs in registers on the same exchanges.
//   general path : stable rocPRIM radix sort of (graph id | inverted attention bits) keys laid out by edge id, then one pass for
//                  rank / topk / hits.  Any graph size.
#include "common.h"
#include <rocprim/rocprim.hpp>

namespace gsat {

constexpr int RANK_BLOCK = 256;                 // 4 waves
constexpr int RANK_GPB = 4;                     // consecutive graphs per workgroup: one per wave
constexpr int RANK_LDS_CAP = 16384;             // keys of the workgroup tier: 128 KiB of the 160 KiB LDS (power of two: bitonic)

// descending-attention sort word: ascending order of the result = descending order of the float, -0.0 == +0.0
__device__ __forceinline__ uint32_t att_desc_bits(float a) {
    uint32_t b = __float_as_uint(a);
    if (b == 0x80000000u) b = 0u;
    const uint32_t asc = b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
    return ~asc;
}

// value of lane (lane ^ J) without LDS
template <int J> __device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
    if constexpr (J == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);        // quad_perm [1,0,3,2]
    else if constexpr (J == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    else if constexpr (J < 32) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (J << 10) | 0x1F);          // bit mode: and 0x1F, xor J
    else {
        // v_permlane32_swap: lanes 32-63 of the first operand trade places with lanes 0-31 of the second.  With both = v the
        // first result holds (own | lower half's) and the second (upper half's | own): each lane picks the foreign one.
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (threadIdx.x & 32) ? r[0] : r[1];
    }
}

// one compare-exchange stage of a bitonic network at stride J (< 64) inside the wave; `i` = index of this lane's key in the sequence
// being sorted, `k` = size of the bitonic blocks being merged
template <int J> __device__ __forceinline__ uint64_t cmpx(uint64_t key, int i, int k) {
    const uint32_t plo = lane_xor<J>((uint32_t)key), phi = lane_xor<J>((uint32_t)(key >> 32));
    const uint64_t other = ((uint64_t)phi << 32) | plo;
    const bool keep_min = ((i & J) == 0) == ((i & k) == 0);
    return (keep_min == (other < key)) ? other : key;
}

// strides 32 .. 1 of the merge of blocks of size k (k >= 64), in registers
__device__ __forceinline__ uint64_t merge_tail(uint64_t key, int i, int k) {
    key = cmpx<32>(key, i, k); key = cmpx<16>(key, i, k); key = cmpx<8>(key, i, k);
    key = cmpx<4>(key, i, k); key = cmpx<2>(key, i, k); key = cmpx<1>(key, i, k);
    return key;
}

// full sort of the 64-key chunk a wave holds (one key per lane); chunk `i >> 6` of a longer sequence ends up ascending when
// (i & 64) == 0 and descending otherwise, as the k = 128 merge expects
__device__ __forceinline__ uint64_t sort64(uint64_t key, int i) {
    key = cmpx<1>(key, i, 2);
    key = cmpx<2>(key, i, 4); key = cmpx<1>(key, i, 4);
    key = cmpx<4>(key, i, 8); key = cmpx<2>(key, i, 8); key = cmpx<1>(key, i, 8);
    key = cmpx<8>(key, i, 16); key = cmpx<4>(key, i, 16); key = cmpx<2>(key, i, 16); key = cmpx<1>(key, i, 16);
    key = cmpx<16>(key, i, 32); key = cmpx<8>(key, i, 32); key = cmpx<4>(key, i, 32); key = cmpx<2>(key, i, 32); key = cmpx<1>(key, i, 32);
    return merge_tail(key, i, 64);
}

constexpr uint64_t KEY_PAD = ~0ull;             // sorts behind every real key (edge ids are < 2^31)

__device__ __forceinline__ uint64_t load_key(const float* __restrict__ att, const int32_t* __restrict__ edge_order, int slot, int E) {
    const int e = edge_order[slot];
    if (e < 0 || e >= E) return KEY_PAD;        // memory-safe on a corrupt permutation
    return ((uint64_t)att_desc_bits(att[e]) << 32) | (uint32_t)e;
}

// position `pos` of graph g (first slot `base`, kk = min(k, E_g)) holds `key`: write the per-edge outputs; returns the label bit of a top-k edge
__device__ __forceinline__ bool emit(uint64_t key, int pos, int base, int k, int kk, const uint8_t* __restrict__ label,
                                     int32_t* __restrict__ order, int32_t* __restrict__ rank, uint8_t* __restrict__ topk) {
    if (key == KEY_PAD) return false;
    const int e = (int)(uint32_t)key;
    if (order) order[base + pos] = e;
    if (rank) rank[e] = pos;
    if (topk) topk[e] = pos < k ? 1 : 0;
    return label != nullptr && pos < kk && label[e] != 0;
}

__global__ void __launch_bounds__(RANK_BLOCK)
k_rank_fused(const float* __restrict__ att, const int32_t* __restrict__ edge_ptr, const int32_t* __restrict__ edge_order,
             const uint8_t* __restrict__ label, int G, int E, int k, int lds_keys, int32_t* __restrict__ order, int32_t* __restrict__ rank,
             uint8_t* __restrict__ topk, int32_t* __restrict__ hits) {
    extern __shared__ uint64_t keys[];           // lds_keys entries (0 when every graph fits a wave)
    __shared__ int hit_count;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = blockIdx.x * RANK_GPB;

    // ---- wave tier: wave w sorts graph g0 + w in registers ----
    {
        const int g = g0 + wave;
        if (g < G) {
            const int lo = edge_ptr[g], n = edge_ptr[g + 1] - lo;
            if (n >= 0 && n <= 64 && lo >= 0 && lo + n <= E) {
                uint64_t key = lane < n ? load_key(att, edge_order, lo + lane, E) : KEY_PAD;
                if (n > 1) key = sort64(key, lane);
                const int kk = k < n ? k : n;
                const bool hit = emit(key, lane, lo, k, kk, label, order, rank, topk);
                const uint64_t m = __ballot(hit);
                if (hits && lane == 0) hits[g] = __popcll(m);
            } else if (n <= 64 && hits && lane == 0) {
                hits[g] = -1;                    // corrupt edge_ptr: skipped whole, marked like an oversized graph below
            }
        }
    }

    // ---- workgroup tier: graphs of this workgroup with more than 64 edges, one after the other, keys in LDS ----
    for (int w = 0; w < RANK_GPB; ++w) {
        const int g = g0 + w;
        if (g >= G) break;
        const int lo = edge_ptr[g], n = edge_ptr[g + 1] - lo;       // uniform over the workgroup
        if (n <= 64) continue;
        if (lo < 0 || lo + n > E || n > lds_keys) {                 // larger than the caller's bound (a contract violation): skipped whole,
            if (hits && threadIdx.x == 0) hits[g] = -1;             // never sorted in part; hits = -1 marks it
            continue;
        }
        int P = 128;
        while (P < n) P <<= 1;
        if (threadIdx.x == 0) hit_count = 0;
        // chunks of 64 keys, sorted in registers on the way into LDS (alternating direction)
        for (int c = wave; c < P / 64; c += RANK_BLOCK / 64) {
            const int i = c * 64 + lane;
            uint64_t key = i < n ? load_key(att, edge_order, lo + i, E) : KEY_PAD;
            keys[i] = sort64(key, i);
        }
        __syncthreads();
        for (int kb = 128; kb <= P; kb <<= 1) {
            for (int j = kb >> 1; j >= 64; j >>= 1) {               // strides that cross waves: compare-exchange in LDS
                for (int t = threadIdx.x; t < P / 2; t += RANK_BLOCK) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                    const uint64_t a = keys[i], b = keys[p];
                    if ((b < a) == ((i & kb) == 0)) { keys[i] = b; keys[p] = a; }
                }
                __syncthreads();
            }
            for (int c = wave; c < P / 64; c += RANK_BLOCK / 64) {  // strides 32 .. 1: in registers
                const int i = c * 64 + lane;
                keys[i] = merge_tail(keys[i], i, kb);
            }
            __syncthreads();
        }
        const int kk = k < n ? k : n;
        int mine = 0;
        for (int i0 = 0; i0 < n; i0 += RANK_BLOCK) {                // every wave runs whole iterations: the ballot sees 64 lanes
            const int i = i0 + threadIdx.x;
            const bool hit = i < n && emit(keys[i], i, lo, k, kk, label, order, rank, topk);
            mine += __popcll(__ballot(hit));
        }
        if (lane == 0 && mine) atomicAdd(&hit_count, mine);
        __syncthreads();
        if (hits && threadIdx.x == 0) hits[g] = hit_count;
        __syncthreads();
    }
}

// ---- general path ---------------------------------------------------------------------------------------------------------------
// slot p of the grouped edge list -> key (graph id | inverted attention bits) stored AT THE EDGE'S ID, so the stable sort breaks
// ties by edge id
__global__ void k_rank_keys(const float* __restrict__ att, const int32_t* __restrict__ edge_ptr, const int32_t* __restrict__ edge_order,
                            int G, int E, uint64_t* __restrict__ keys, int32_t* __restrict__ ids) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    int lo = 0, hi = G;                          // last g with edge_ptr[g] <= p
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (edge_ptr[mid] <= p) lo = mid; else hi = mid;
    }
    const int e = edge_order[p];
    if (e < 0 || e >= E) return;
    keys[e] = ((uint64_t)(uint32_t)lo << 32) | att_desc_bits(att[e]);
    ids[e] = e;
}

__global__ void k_rank_finish(const uint64_t* __restrict__ keys, const int32_t* __restrict__ sorted_ids, const int32_t* __restrict__ edge_ptr,
                              const uint8_t* __restrict__ label, int G, int E, int k, int32_t* __restrict__ rank, uint8_t* __restrict__ topk,
                              int32_t* __restrict__ hits) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= E) return;
    const int g = (int)(keys[q] >> 32), e = sorted_ids[q];
    if (g < 0 || g >= G || e < 0 || e >= E) return;
    const int pos = q - edge_ptr[g];
    if (rank) rank[e] = pos;
    if (topk) topk[e] = pos < k ? 1 : 0;
    if (hits && label && pos < k && label[e] != 0) atomicAdd(&hits[g], 1);          // integer sum: order independent
}

static size_t rank_sort_temp_bytes(int64_t E) {
    size_t tb = 0;
    uint64_t* kk = nullptr;
    int32_t* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, tb, kk, kk, v, v, (size_t)(E > 0 ? E : 1), 0, 64u, (hipStream_t)0);
    return align_up(tb, 256) + 256;
}

// ---- AUROC ------------------------------------------------------------------------------------------------------------------------
__global__ void k_auroc_keys(const float* __restrict__ att, int64_t E, uint32_t* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < E) keys[i] = ~att_desc_bits(att[i]);            // ascending attention
}

struct IsNegative {
    const uint8_t* lab;
    int64_t E;
    __host__ __device__ int operator()(int i) const { return (i < E && lab[i] == 0) ? 1 : 0; }
};

constexpr int AUROC_BLOCK = 256;

// keys ascending, lab the labels in the same order, cneg[i] = negatives among positions < i (cneg[E] = all of them).  A positive
// whose tie group is [s, t) adds 2 * cneg[s] + (cneg[t] - cneg[s]) = cneg[s] + cneg[t].
__global__ void __launch_bounds__(AUROC_BLOCK)
k_auroc_sum(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ lab, const int32_t* __restrict__ cneg, int64_t E,
            unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[AUROC_BLOCK / 64];
    unsigned long long acc = 0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < E; q += (int64_t)gridDim.x * blockDim.x) {
        if (lab[q] == 0) continue;
        const uint32_t key = keys[q];
        int64_t lo = 0, hi = q;                  // first position with keys[pos] == key (it is <= q)
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
        const int64_t s = lo;
        lo = q + 1; hi = E;                      // first position with keys[pos] > key
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] <= key) lo = mid + 1; else hi = mid; }
        acc += (unsigned long long)cneg[s] + (unsigned long long)cneg[lo];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < AUROC_BLOCK / 64; ++w) s += part[w];
        if (s) atomicAdd(&out[0], s);            // 64-bit integer vector atomic: the sum does not depend on the order
        if (blockIdx.x == 0) {
            const unsigned long long nn = (unsigned long long)cneg[E];
            out[1] = (unsigned long long)E - nn;
            out[2] = nn;
        }
    }
}

static size_t auroc_sort_temp_bytes(int64_t E) {
    size_t tb = 0;
    uint32_t* kk = nullptr;
    uint8_t* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, tb, kk, kk, v, v, (size_t)(E > 0 ? E : 1), 0, 32u, (hipStream_t)0);
    return align_up(tb, 256) + 256;
}
static size_t auroc_scan_temp_bytes(int64_t E) {
    size_t tb = 0;
    auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int>(0), IsNegative{nullptr, 0});
    int32_t* out = nullptr;
    (void)rocprim::exclusive_scan(nullptr, tb, in, out, 0, (size_t)(E + 1), rocprim::plus<int>(), (hipStream_t)0);
    return align_up(tb, 256) + 256;
}

// ---- delta KL -----------------------------------------------------------------------------------------------------------------------
constexpr int KL_BLOCK = 256;
constexpr int KL_MAX_BLOCKS = 256;

// sum over the workgroup in a fixed order (butterfly inside the wave, waves in index order); valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < KL_BLOCK / 64; ++w) s += sh[w];
    return s;
}

__device__ __forceinline__ double clampd(double a, double lo, double hi) { return a < lo ? lo : (a > hi ? hi : a); }

__global__ void __launch_bounds__(KL_BLOCK)
k_kl_mean(const float* __restrict__ att, int64_t E, double eps, double* __restrict__ partial) {
    __shared__ double sh[KL_BLOCK / 64];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * KL_BLOCK + threadIdx.x; i < E; i += (int64_t)gridDim.x * KL_BLOCK)
        acc += clampd((double)att[i], eps, 1.0 - eps);
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// partial[nb .. 5 nb): per workgroup (kl, sum of labelled attention, labelled count, sum of unlabelled attention)
__global__ void __launch_bounds__(KL_BLOCK)
k_kl_terms(const float* __restrict__ att, const uint8_t* __restrict__ label, int64_t E, double eps, double* __restrict__ partial) {
    __shared__ double sh[KL_BLOCK / 64];
    const int nb = gridDim.x;
    double total = 0.0;
    for (int b = 0; b < nb; ++b) total += partial[b];          // every workgroup forms the same mean, in the same order
    const double r = clampd(total / (double)E, eps, 1.0 - eps);
    const double lr = log(r), l1r = log(1.0 - r);
    double kl = 0.0, sig = 0.0, cnt = 0.0, bkg = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * KL_BLOCK + threadIdx.x; i < E; i += (int64_t)gridDim.x * KL_BLOCK) {
        const double raw = (double)att[i];
        const double a = clampd(raw, eps, 1.0 - eps);
        const bool pos = label[i] != 0;
        const double p = pos ? 1.0 - eps : eps;
        kl += p * (log(a) - lr) + (1.0 - p) * (log(1.0 - a) - l1r);
        if (pos) { sig += raw; cnt += 1.0; } else bkg += raw;
    }
    double* out = partial + nb + 4 * blockIdx.x;
    const double s0 = block_sum(kl, sh), s1 = block_sum(sig, sh), s2 = block_sum(cnt, sh), s3 = block_sum(bkg, sh);
    if (threadIdx.x == 0) { out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3; }
}

__global__ void k_kl_finish(const double* __restrict__ partial, int nb, int64_t E, float* __restrict__ out) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nb; ++b)
        for (int c = 0; c < 4; ++c) s[c] += partial[nb + 4 * b + c];
    const double nneg = (double)E - s[2];
    out[0] = (float)s[0];
    out[1] = s[2] > 0.0 ? (float)(s[1] / s[2]) : 0.f;
    out[2] = nneg > 0.0 ? (float)(s[3] / nneg) : 0.f;
}

}  // namespace gsat

using namespace gsat;

extern "C" {

int64_t gsat_rank_edges_lds_cap(void) { return RANK_LDS_CAP; }

size_t gsat_rank_edges_workspace_bytes(int64_t E) {
    const size_t e = (size_t)(E > 0 ? E : 1);
    return 256 + 2 * align_up(e * 8, 256) + 2 * align_up(e * 4, 256) + rank_sort_temp_bytes(E);
}

int gsat_rank_edges(const float* att, const int32_t* edge_ptr, const int32_t* edge_order, const uint8_t* label, int64_t E, int64_t G,
                    int64_t k, int64_t max_seg_edges, int path, int32_t* order, int32_t* rank, uint8_t* topk, int32_t* hits,
                    void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && G >= 0 && k >= 0 && path >= 0 && path <= 2, GSAT_ERR_ARG, "gsat_rank_edges: bad argument");
    GSAT_REQUIRE(E < (1ll << 31) && G < (1ll << 31), GSAT_ERR_UNSUPPORTED, "gsat_rank_edges: >2^31 entries");
    GSAT_REQUIRE(!hits || label, GSAT_ERR_ARG, "gsat_rank_edges: hits needs label");
    if (G == 0) return GSAT_OK;
    GSAT_REQUIRE(edge_ptr && (E == 0 || (att && edge_order)), GSAT_ERR_ARG, "gsat_rank_edges: null pointer");
    const bool fits = max_seg_edges >= 0 && max_seg_edges <= RANK_LDS_CAP;
    GSAT_REQUIRE(path != 1 || fits, GSAT_ERR_ARG,
                 "gsat_rank_edges: fused path forced with max_seg_edges = %lld (cap %d, -1 = unknown)", (long long)max_seg_edges, RANK_LDS_CAP);
    const int kc = (int)std::min<int64_t>(k, (int64_t)1 << 30);
    if (path == 1 || (path == 0 && fits)) {
        int lds_keys = 0;
        if (max_seg_edges > 64) { lds_keys = 128; while (lds_keys < max_seg_edges) lds_keys <<= 1; }
        const size_t lds_bytes = (size_t)lds_keys * sizeof(uint64_t);
        if (lds_bytes > 48 * 1024)                // above the default dynamic-LDS limit: raised on the current device (a host-side
            GSAT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rank_fused), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               RANK_LDS_CAP * (int)sizeof(uint64_t)));      // attribute, cheap, no stream work)
        k_rank_fused<<<(unsigned)ceil_div(G, RANK_GPB), RANK_BLOCK, lds_bytes, stream>>>(att, edge_ptr, edge_order, label, (int)G, (int)E, kc,
                                                                                          lds_keys, order, rank, topk, hits);
        GSAT_LAUNCH_CHECK();
        return GSAT_OK;
    }
    if (hits) GSAT_CHECK_HIP(gsat::zero_async(hits, (size_t)G * sizeof(int32_t), stream));
    if (E == 0) return GSAT_OK;
    Arena ar(workspace, ws_bytes);
    uint64_t* keys_in = ar.take<uint64_t>(E);
    uint64_t* keys_out = ar.take<uint64_t>(E);
    int32_t* ids = ar.take<int32_t>(E);
    int32_t* ids_out = ar.take<int32_t>(E);
    const size_t tb = rank_sort_temp_bytes(E);
    char* temp = ar.take<char>(tb);
    GSAT_REQUIRE(ar.ok() && temp, GSAT_ERR_WORKSPACE, "gsat_rank_edges: workspace %zu < %zu", ws_bytes, ar.off);
    const int B = 256;
    k_rank_keys<<<(unsigned)ceil_div(E, B), B, 0, stream>>>(att, edge_ptr, edge_order, (int)G, (int)E, keys_in, ids);
    GSAT_LAUNCH_CHECK();
    int gbits = 1;
    while (gbits < 31 && ((G - 1) >> gbits) != 0) ++gbits;
    int32_t* sorted_ids = order ? order : ids_out;
    size_t tbq = tb;
    GSAT_CHECK_HIP(rocprim::radix_sort_pairs(temp, tbq, keys_in, keys_out, ids, sorted_ids, (size_t)E, 0, (unsigned)(32 + gbits), stream));
    k_rank_finish<<<(unsigned)ceil_div(E, B), B, 0, stream>>>(keys_out, sorted_ids, edge_ptr, label, (int)G, (int)E, kc, rank, topk, hits);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

size_t gsat_auroc_workspace_bytes(int64_t E) {
    const size_t e = (size_t)(E > 0 ? E : 1);
    return 256 + 2 * align_up(e * 4, 256) + align_up(e, 256) + align_up((e + 1) * 4, 256) + std::max(auroc_sort_temp_bytes(E), auroc_scan_temp_bytes(E));
}

int gsat_auroc(const float* att, const uint8_t* label, int64_t E, uint64_t* out, void* workspace, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && out, GSAT_ERR_ARG, "gsat_auroc: bad argument");
    GSAT_REQUIRE(E < (1ll << 31) - 1, GSAT_ERR_UNSUPPORTED, "gsat_auroc: >2^31 entries");
    GSAT_CHECK_HIP(gsat::zero_async(out, 3 * sizeof(uint64_t), stream));
    if (E == 0) return GSAT_OK;
    GSAT_REQUIRE(att && label, GSAT_ERR_ARG, "gsat_auroc: null pointer");
    Arena ar(workspace, ws_bytes);
    uint32_t* keys_in = ar.take<uint32_t>(E);
    uint32_t* keys_out = ar.take<uint32_t>(E);
    uint8_t* lab_out = ar.take<uint8_t>(E);
    int32_t* cneg = ar.take<int32_t>(E + 1);
    size_t ts = auroc_sort_temp_bytes(E), tc = auroc_scan_temp_bytes(E);
    char* temp = ar.take<char>(std::max(ts, tc));
    GSAT_REQUIRE(ar.ok() && temp, GSAT_ERR_WORKSPACE, "gsat_auroc: workspace %zu < %zu", ws_bytes, ar.off);
    const int B = 256;
    k_auroc_keys<<<(unsigned)ceil_div(E, B), B, 0, stream>>>(att, E, keys_in);
    GSAT_LAUNCH_CHECK();
    GSAT_CHECK_HIP(rocprim::radix_sort_pairs(temp, ts, keys_in, keys_out, label, lab_out, (size_t)E, 0, 32u, stream));
    auto in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<int>(0), IsNegative{lab_out, E});
    GSAT_CHECK_HIP(rocprim::exclusive_scan(temp, tc, in, cneg, 0, (size_t)(E + 1), rocprim::plus<int>(), stream));
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(E, AUROC_BLOCK), 1024);
    k_auroc_sum<<<blocks, AUROC_BLOCK, 0, stream>>>(keys_out, lab_out, cneg, E, reinterpret_cast<unsigned long long*>(out));
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

size_t gsat_delta_kl_workspace_bytes(int64_t E) {
    (void)E;
    return 256 + 5 * KL_MAX_BLOCKS * sizeof(double);
}

int gsat_delta_kl(const float* att, const uint8_t* label, int64_t E, double eps, float* out, void* workspace, size_t ws_bytes,
                  void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(E >= 0 && out && eps > 0.0 && eps < 0.5, GSAT_ERR_ARG, "gsat_delta_kl: bad argument");
    if (E == 0) {
        GSAT_CHECK_HIP(gsat::zero_async(out, 3 * sizeof(float), stream));
        return GSAT_OK;
    }
    GSAT_REQUIRE(att && label, GSAT_ERR_ARG, "gsat_delta_kl: null pointer");
    Arena ar(workspace, ws_bytes);
    double* partial = ar.take<double>(5 * KL_MAX_BLOCKS);
    GSAT_REQUIRE(ar.ok() && partial, GSAT_ERR_WORKSPACE, "gsat_delta_kl: workspace %zu < %zu", ws_bytes, ar.off);
    const int nb = (int)std::min<int64_t>(ceil_div(E, KL_BLOCK * 4), KL_MAX_BLOCKS);     // a function of E alone: the combine order is fixed
    k_kl_mean<<<nb, KL_BLOCK, 0, stream>>>(att, E, eps, partial);
    GSAT_LAUNCH_CHECK();
    k_kl_terms<<<nb, KL_BLOCK, 0, stream>>>(att, label, E, eps, partial);
    GSAT_LAUNCH_CHECK();
    k_kl_finish<<<1, 1, 0, stream>>>(partial, nb, E, out);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

}  // extern "C"
