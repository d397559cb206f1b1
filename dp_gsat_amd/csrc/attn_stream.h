// Memory-bounded edge-mode extractor (included by attn.hip, which holds the kernels and helpers it shares with the staged pipeline).
//
// The staged pipeline keeps two [M, C1] tensors, a1 = dropout(relu(norm(h1))) (saved by the forward) and da1 -> dh1 (backward workspace).
// The per-graph InstanceNorm makes the graphs of a batch independent everywhere except in the weight-gradient sums, so the junction of
// layer 1 and layer 2 runs here GROUP OF WHOLE GRAPHS by group, through a scratch of `scratch_rows` rows:
//   forward   per group: layer-1 statistics + a1 of its rows into the scratch, h2[r0:r1] = a1 W2^T; then layer 2, head, sampler as staged
//   backward  head as staged (dh2 [M, C2]); per group: a1 again from P, Q, b1, the saved statistics and the keep decisions,
//             dW2 += dh2[r0:r1]^T a1, da1 = dh2[r0:r1] W2, dh1 in place, dP / dQ of the group's nodes; then demb, dW1 as staged
// Two things must hold and are checked once per batch by gsat_attn_stream_check: rows are grouped by graph in row order (a group's rows
// are one range [r0, r1)), and no edge joins two graphs (the CSR rows of a group's nodes hold edge ids of [r0, r1) only).
// Every kernel takes the group's bases (graph g0, row r0, node n0) and the scratch capacity as parameters and indexes the scratch by
// (row - r0) under a bound check: a wrong base reads a wrong row of the scratch, never memory outside it.  Philox draws and explicit masks
// stay keyed by the GLOBAL row.  No float atomics: groups run in order on one stream, dW2 accumulates in that order.
#pragma once

namespace gsat {

constexpr int ST_CH = GSAT_LONG_ROW_EDGES;

// verdict bits of gsat_attn_stream_check
constexpr int ST_BAD_ORDER = GSAT_ATTN_STREAM_BAD_ORDER, ST_BAD_CROSS = GSAT_ATTN_STREAM_BAD_CROSS;

// One workgroup walks all rows and STORES the verdict (nothing has to be zeroed first, so the check is one launch).  Runs once per batch.
__global__ __launch_bounds__(1024) void k_st_check(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                   const int32_t* __restrict__ node_seg, const int32_t* __restrict__ seg_ptr,
                                                   const int32_t* __restrict__ row_seg, int M, int N, int G, int32_t* __restrict__ verdict) {
    __shared__ int bits;
    if (threadIdx.x == 0) bits = 0;
    __syncthreads();
    int v = 0;
    // branch-free body (ids clamped before they index), so that the loads of several rows are in flight per thread
#pragma unroll 4
    for (int m = threadIdx.x; m < M; m += blockDim.x) {
        const int g = row_seg[m], s = src[m], d = dst[m];
        const bool gok = (unsigned)g < (unsigned)G, nok = (unsigned)s < (unsigned)N && (unsigned)d < (unsigned)N;
        const int gc = gok ? g : 0;
        const int beg = seg_ptr[gc], end = seg_ptr[gc + 1], gs = node_seg[nok ? s : 0], gd = node_seg[nok ? d : 0];
        v |= (!gok || m < beg || m >= end) ? ST_BAD_ORDER : 0;
        v |= (!nok || gs != gd || gs != g) ? ST_BAD_CROSS : 0;
    }
    if (v) atomicOr(&bits, v);
    __syncthreads();
    if (threadIdx.x == 0) verdict[0] = bits;
}

// Layer-1 statistics of graphs [g0, g0 + gridDim.x) and their activation into the scratch: k_seg_stats<true, true> with bases.
// grid (graphs of the group, ceil(C/64)); mean / rstd are the batch's [G, C] arrays, indexed by the global graph.
__global__ __launch_bounds__(SB) void k_st_l1_fwd(PreAct<true> pre, const int32_t* __restrict__ seg_ptr, int g0, int r0, int cap,
                                                  float* __restrict__ mean_out, float* __restrict__ rstd_out, const float* __restrict__ mask,
                                                  SeedRef seed, float p, int training, float* __restrict__ act) {
    __shared__ float4 sm[SB_SLOTS][SB_LANES];
    __shared__ float4 bc[SB_LANES];
    const int g = g0 + blockIdx.x;
    const int lane = threadIdx.x % SB_LANES, slot = threadIdx.x / SB_LANES;
    const int c = (blockIdx.y * SB_LANES + lane) * 4;
    const int C = pre.C;
    const bool on = c < C;
    const int beg = seg_ptr[g], end = seg_ptr[g + 1];
    const float inv_n = 1.f / (float)max(end - beg, 1);
    float4 acc = f4zero();
    if (on)
        for (int r = beg + slot; r < end; r += SB_SLOTS) {
            const float4 h = pre.load(r, c);
            acc.x += h.x; acc.y += h.y; acc.z += h.z; acc.w += h.w;
        }
    float4 tot = slot_reduce(acc, sm, slot, lane);
    if (slot == 0) bc[lane] = make_float4(tot.x * inv_n, tot.y * inv_n, tot.z * inv_n, tot.w * inv_n);
    __syncthreads();
    const float4 mu = bc[lane];
    acc = f4zero();
    if (on)
        for (int r = beg + slot; r < end; r += SB_SLOTS) {          // second and third pass: the segment's rows are cache-hot
            const float4 h = pre.load(r, c);
            const float dx = h.x - mu.x, dy = h.y - mu.y, dz = h.z - mu.z, dw = h.w - mu.w;
            acc.x = fmaf(dx, dx, acc.x); acc.y = fmaf(dy, dy, acc.y); acc.z = fmaf(dz, dz, acc.z); acc.w = fmaf(dw, dw, acc.w);
        }
    tot = slot_reduce(acc, sm, slot, lane);
    float4 rs = make_float4(1.f / sqrtf(tot.x * inv_n + IN_EPS), 1.f / sqrtf(tot.y * inv_n + IN_EPS),
                            1.f / sqrtf(tot.z * inv_n + IN_EPS), 1.f / sqrtf(tot.w * inv_n + IN_EPS));
    if (slot == 0 && on) {
        st4(mean_out + (size_t)g * C + c, mu);
        st4(rstd_out + (size_t)g * C + c, rs);
    }
    if (slot == 0) bc[lane] = rs;              // every thread took `mu` out of bc before slot_reduce's barriers
    __syncthreads();
    rs = bc[lane];
    const float sc = (training && p > 0.f) ? 1.f / (1.f - p) : 1.f;
    if (on)
        for (int r = beg + slot; r < end; r += SB_SLOTS) {
            const int lr = r - r0;
            if ((unsigned)lr >= (unsigned)cap) continue;
            const float4 h = pre.load(r, c);
            const float4 k = keep4(mask, seed, 1, r, c, C, p, training != 0);
            st4(act + (size_t)lr * C + c,
                make_float4(fmaxf((h.x - mu.x) * rs.x, 0.f) * k.x * sc, fmaxf((h.y - mu.y) * rs.y, 0.f) * k.y * sc,
                            fmaxf((h.z - mu.z) * rs.z, 0.f) * k.z * sc, fmaxf((h.w - mu.w) * rs.w, 0.f) * k.w * sc));
        }
}

// Long graphs (gridDim.z slices per graph): k_seg_partial<true> with a graph base; part is indexed by the graph WITHIN the group
__global__ __launch_bounds__(SB) void k_st_l1_partial(PreAct<true> pre, const int32_t* __restrict__ seg_ptr, int g0,
                                                      const float* __restrict__ mean /* null: plain sum */, float* __restrict__ part) {
    __shared__ float4 sm[SB_SLOTS][SB_LANES];
    const int g = g0 + blockIdx.x;
    const int lane = threadIdx.x % SB_LANES, slot = threadIdx.x / SB_LANES;
    const int c = (blockIdx.y * SB_LANES + lane) * 4;
    const int C = pre.C;
    const bool on = c < C;
    int beg, end; float inv_n;
    seg_slice(seg_ptr, g, &beg, &end, &inv_n);
    float4 acc = f4zero();
    if (on) {
        const float4 mu = mean ? ld4(mean + (size_t)g * C + c) : f4zero();
        for (int r = beg + slot; r < end; r += SB_SLOTS) {
            const float4 h = pre.load(r, c);
            if (mean) {
                const float dx = h.x - mu.x, dy = h.y - mu.y, dz = h.z - mu.z, dw = h.w - mu.w;
                acc.x = fmaf(dx, dx, acc.x); acc.y = fmaf(dy, dy, acc.y); acc.z = fmaf(dz, dz, acc.z); acc.w = fmaf(dw, dw, acc.w);
            } else {
                acc.x += h.x; acc.y += h.y; acc.z += h.z; acc.w += h.w;
            }
        }
    }
    const float4 tot = slot_reduce(acc, sm, slot, lane);
    if (slot == 0 && on) st4(part + ((size_t)blockIdx.x * gridDim.z + blockIdx.z) * C + c, tot);
}

// k_zcombine for the graphs [g0, g0 + ng) of a group: out[(og0 + j), c] = f(sum_z part[j, z, c]), j the graph within the group
__global__ void k_st_zcombine(const float* __restrict__ part, const int32_t* __restrict__ seg_ptr, int g0, int og0, int ng, int Z, int C, int mode,
                              float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)ng * C) return;
    const int j = (int)(i / C), c = (int)(i % C);
    float acc = 0.f;
    for (int z = 0; z < Z; ++z) acc += part[((size_t)j * Z + z) * C + c];
    const float inv_n = 1.f / (float)max(seg_ptr[g0 + j + 1] - seg_ptr[g0 + j], 1);
    out[(size_t)(og0 + j) * C + c] = mode == 0 ? acc : mode == 1 ? acc * inv_n : 1.f / sqrtf(acc * inv_n + IN_EPS);
}

// a1 of rows [r0, r0 + rows) into the scratch from the statistics: k_norm_apply<true, true> with a row base.  The forward of sliced
// graphs and EVERY backward (the recompute) run it; mask and Philox are keyed by the global row m.
__global__ void k_st_l1_apply(PreAct<true> pre, const int32_t* __restrict__ row_seg, const float* __restrict__ mean,
                              const float* __restrict__ rstd, const float* __restrict__ mask, SeedRef seed, float p, int training,
                              int r0, int rows, int cap, float* __restrict__ out) {
    const int C = pre.C, C4 = C >> 2;
    const float sc = (training && p > 0.f) ? 1.f / (1.f - p) : 1.f;
    const int64_t total = (int64_t)min(rows, cap) * C4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int lr = (int)(i / C4), c = (int)(i % C4) * 4;
        const int m = r0 + lr;
        const int g = row_seg[m];
        const float4 h = pre.load(m, c);
        const float4 mu = ld4(mean + (size_t)g * C + c), rs = ld4(rstd + (size_t)g * C + c);
        const float4 k = keep4(mask, seed, 1, m, c, C, p, training != 0);
        st4(out + (size_t)lr * C + c,
            make_float4(fmaxf((h.x - mu.x) * rs.x, 0.f) * k.x * sc, fmaxf((h.y - mu.y) * rs.y, 0.f) * k.y * sc,
                        fmaxf((h.z - mu.z) * rs.z, 0.f) * k.z * sc, fmaxf((h.w - mu.w) * rs.w, 0.f) * k.w * sc));
    }
}

// Backward statistics of layer 1 of the group's graphs from the two scratches (k_l1_bwd_stats with bases):
//   dy1 = da1 * [a1 > 0] * sc, yhat1 * [a1 > 0] = a1 / sc;  S1 = mean dy1, S2 = mean dy1 * yhat1, both indexed by the graph WITHIN the group.
// APPLY (gridDim.z == 1): a second pass writes dh1 = rstd1 * (dy1 - S1 - yhat1 * S2) in place over da1.
template <bool APPLY>
__global__ __launch_bounds__(SB) void k_st_l1_bwd(float* __restrict__ da1, const float* __restrict__ a1, const int32_t* __restrict__ seg_ptr,
                                                  int g0, int r0, int cap, float sc, float* __restrict__ S1, float* __restrict__ S2,
                                                  PreAct<true> pre, const float* __restrict__ mean, const float* __restrict__ rstd) {
    __shared__ float4 sm[SB_SLOTS][SB_LANES];
    __shared__ float4 bc1[SB_LANES], bc2[SB_LANES];
    const int g = g0 + blockIdx.x;
    const int lane = threadIdx.x % SB_LANES, slot = threadIdx.x / SB_LANES;
    const int c = (blockIdx.y * SB_LANES + lane) * 4;
    const int C = pre.C;
    const bool on = c < C;
    int beg, end; float inv_n;
    seg_slice(seg_ptr, g, &beg, &end, &inv_n);
    if (gridDim.z > 1) inv_n = 1.f;                         // raw partial sums, scaled by k_st_zcombine
    const size_t orow = (size_t)blockIdx.x * gridDim.z + blockIdx.z;
    const float inv_sc = 1.f / sc;
    float4 s1 = f4zero(), s2 = f4zero();
    if (on)
        for (int r = beg + slot; r < end; r += SB_SLOTS) {
            const int lr = r - r0;
            if ((unsigned)lr >= (unsigned)cap) continue;
            const float4 d = ld4(da1 + (size_t)lr * C + c), a = ld4(a1 + (size_t)lr * C + c);
            const float4 dy = make_float4(a.x > 0.f ? d.x * sc : 0.f, a.y > 0.f ? d.y * sc : 0.f, a.z > 0.f ? d.z * sc : 0.f, a.w > 0.f ? d.w * sc : 0.f);
            s1.x += dy.x; s1.y += dy.y; s1.z += dy.z; s1.w += dy.w;
            s2.x = fmaf(dy.x, a.x * inv_sc, s2.x); s2.y = fmaf(dy.y, a.y * inv_sc, s2.y);
            s2.z = fmaf(dy.z, a.z * inv_sc, s2.z); s2.w = fmaf(dy.w, a.w * inv_sc, s2.w);
        }
    float4 t1 = slot_reduce(s1, sm, slot, lane);
    float4 t2 = slot_reduce(s2, sm, slot, lane);
    t1 = make_float4(t1.x * inv_n, t1.y * inv_n, t1.z * inv_n, t1.w * inv_n);
    t2 = make_float4(t2.x * inv_n, t2.y * inv_n, t2.z * inv_n, t2.w * inv_n);
    if (slot == 0 && on) {
        st4(S1 + orow * C + c, t1);
        st4(S2 + orow * C + c, t2);
    }
    if (APPLY) {
        if (slot == 0) { bc1[lane] = t1; bc2[lane] = t2; }
        __syncthreads();
        if (!on) return;
        const float4 q1 = bc1[lane], q2 = bc2[lane];
        const float4 mu = ld4(mean + (size_t)g * C + c), rs = ld4(rstd + (size_t)g * C + c);
        for (int r = beg + slot; r < end; r += SB_SLOTS) {
            const int lr = r - r0;
            if ((unsigned)lr >= (unsigned)cap) continue;
            const float4 h = pre.load(r, c);
            const float4 d = ld4(da1 + (size_t)lr * C + c), a = ld4(a1 + (size_t)lr * C + c);
            const float4 y = make_float4((h.x - mu.x) * rs.x, (h.y - mu.y) * rs.y, (h.z - mu.z) * rs.z, (h.w - mu.w) * rs.w);
            const float4 dy = make_float4(a.x > 0.f ? d.x * sc : 0.f, a.y > 0.f ? d.y * sc : 0.f, a.z > 0.f ? d.z * sc : 0.f, a.w > 0.f ? d.w * sc : 0.f);
            st4(da1 + (size_t)lr * C + c, make_float4(rs.x * (dy.x - q1.x - y.x * q2.x), rs.y * (dy.y - q1.y - y.y * q2.y),
                                                       rs.z * (dy.z - q1.z - y.z * q2.z), rs.w * (dy.w - q1.w - y.w * q2.w)));
        }
    }
}

// dh1 of rows [r0, r0 + rows) in place over the da1 scratch (k_dh1 with bases): after the sliced statistics.  S1 / S2 [ng, C] by the
// graph within the group
__global__ void k_st_dh1(PreAct<true> pre, const int32_t* __restrict__ row_seg, const float* __restrict__ mean, const float* __restrict__ rstd,
                         const float* __restrict__ a1, float sc, const float* __restrict__ S1, const float* __restrict__ S2, int g0, int ng,
                         int r0, int rows, int cap, float* __restrict__ da1_inout) {
    const int C = pre.C, C4 = C >> 2;
    const int64_t total = (int64_t)min(rows, cap) * C4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int lr = (int)(i / C4), c = (int)(i % C4) * 4;
        const int m = r0 + lr;
        const int g = row_seg[m], lg = g - g0;
        if ((unsigned)lg >= (unsigned)ng) continue;
        const float4 h = pre.load(m, c);
        const float4 mu = ld4(mean + (size_t)g * C + c), rs = ld4(rstd + (size_t)g * C + c);
        const float4 y = make_float4((h.x - mu.x) * rs.x, (h.y - mu.y) * rs.y, (h.z - mu.z) * rs.z, (h.w - mu.w) * rs.w);
        const float4 d = ld4(da1_inout + (size_t)lr * C + c), a = ld4(a1 + (size_t)lr * C + c);
        const float4 dy = make_float4(a.x > 0.f ? d.x * sc : 0.f, a.y > 0.f ? d.y * sc : 0.f, a.z > 0.f ? d.z * sc : 0.f, a.w > 0.f ? d.w * sc : 0.f);
        const float4 s1 = ld4(S1 + (size_t)lg * C + c), s2 = ld4(S2 + (size_t)lg * C + c);
        st4(da1_inout + (size_t)lr * C + c, make_float4(rs.x * (dy.x - s1.x - y.x * s2.x), rs.y * (dy.y - s1.y - y.y * s2.y),
                                                         rs.z * (dy.z - s1.z - y.z * s2.z), rs.w * (dy.w - s1.w - y.w * s2.w)));
    }
}

// sum over the CSR slots [beg, end) of the scratch rows x[eid[k] - r0, c .. c + 3], in slot order, four rows in flight
__device__ __forceinline__ float4 st_slot_sum(const float* __restrict__ x, const int32_t* __restrict__ eid, int beg, int end, int r0, int cap, int C, int c) {
    float4 acc = f4zero();
    int k = beg;
    for (; k + 4 <= end; k += 4) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int lr = eid[k + j] - r0;
            v[j] = (unsigned)lr < (unsigned)cap ? ld4(x + (size_t)lr * C + c) : f4zero();
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc.x += v[j].x; acc.y += v[j].y; acc.z += v[j].z; acc.w += v[j].w; }
    }
    for (; k < end; ++k) {
        const int lr = eid[k] - r0;
        if ((unsigned)lr < (unsigned)cap) { const float4 v = ld4(x + (size_t)lr * C + c); acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
    }
    return acc;
}

// Hub rows of the group's nodes [n0, n1): chunk_ptr is the batch's table, so the group's items are [chunk_ptr[n0], chunk_ptr[n1]) and
// partial is indexed by (item - chunk_ptr[n0]) < max_items.  One thread per (item, 4 channels).
__global__ __launch_bounds__(256) void k_st_gather_chunk(const float* __restrict__ x, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ eid,
                                                         const int32_t* __restrict__ chunk_ptr, int n0, int n1, int r0, int cap, int C, int max_items,
                                                         float* __restrict__ partial) {
    const int C4 = C >> 2;
    const int base = chunk_ptr[n0];
    const int64_t total = (int64_t)min(chunk_ptr[n1] - base, max_items) * C4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int it = (int)(i / C4), c = (int)(i % C4) * 4;
        const int item = base + it;
        int lo = n0, hi = n1;                        // invariant: chunk_ptr[lo] <= item < chunk_ptr[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (chunk_ptr[mid] <= item) lo = mid; else hi = mid;
        }
        const int beg = rowptr[lo] + (item - chunk_ptr[lo]) * ST_CH;
        const int end = min(beg + ST_CH, rowptr[lo + 1]);
        st4(partial + (size_t)it * C + c, st_slot_sum(x, eid, beg, end, r0, cap, C, c));
    }
}

// out[n, :] = sum over the CSR row of node n in [n0, n1) of the scratch rows; long rows add their chunk partials in chunk order
__global__ __launch_bounds__(256) void k_st_gather(const float* __restrict__ x, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ eid,
                                                   const int32_t* __restrict__ chunk_ptr, const float* __restrict__ partial, int n0, int n1, int r0,
                                                   int cap, int C, int max_items, float* __restrict__ out) {
    const int C4 = C >> 2;
    const int64_t total = (int64_t)(n1 - n0) * C4;
    const int base = chunk_ptr ? chunk_ptr[n0] : 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int n = n0 + (int)(i / C4), c = (int)(i % C4) * 4;
        const int beg = rowptr[n], end = rowptr[n + 1];
        float4 acc;
        if (chunk_ptr != nullptr && end - beg > ST_CH) {
            acc = f4zero();
            for (int q = chunk_ptr[n]; q < chunk_ptr[n + 1]; ++q) {
                const int it = q - base;
                if ((unsigned)it >= (unsigned)max_items) continue;
                const float4 v = ld4(partial + (size_t)it * C + c);
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        } else {
            acc = st_slot_sum(x, eid, beg, end, r0, cap, C, c);
        }
        st4(out + (size_t)n * C + c, acc);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static inline int64_t st_max_items(int64_t rows) { return 2 * (rows / ST_CH) + 1; }          // as aggregate.hip's bound, for a group's rows
// upper bound on (graphs of a group) x (its slices): Zg <= rows / (ng * 4096) + 1
static inline size_t st_group_parts(const gsat_attn_args* a, int64_t scratch_rows) { return (size_t)a->G + (size_t)scratch_rows / 4096 + 1; }
static inline size_t st_part_floats(const gsat_attn_args* a, int64_t scratch_rows) {
    const size_t cmax = std::max(a->C1, a->C2);
    return std::max(st_group_parts(a, scratch_rows), (size_t)a->G * seg_slices(a->M, a->G)) * cmax;
}

struct StPlan { const int32_t* group_ptr; int64_t n_groups; const int32_t* seg; const int32_t* node; int64_t scratch_rows; };

static int st_check(const gsat_attn_args* a, const StPlan& pl, const char* who) {
    GSAT_REQUIRE(a->seg_order == nullptr, GSAT_ERR_ARG, "%s: rows must be grouped by graph in row order (seg_order == NULL)", who);
    if (a->M == 0) return GSAT_OK;
    const int64_t G = a->G;
    GSAT_REQUIRE(pl.group_ptr && pl.seg && pl.node && pl.n_groups >= 1 && pl.n_groups <= G && pl.scratch_rows >= 1, GSAT_ERR_ARG, "%s: null or empty plan", who);
    GSAT_REQUIRE(a->node_ptr, GSAT_ERR_ARG, "%s: needs node_ptr", who);
    GSAT_REQUIRE(pl.seg[0] == 0 && pl.seg[G] == a->M && pl.node[0] == 0 && pl.node[G] == a->N, GSAT_ERR_ARG, "%s: host pointers do not match M / N", who);
    for (int64_t g = 0; g < G; ++g)
        GSAT_REQUIRE(pl.seg[g] <= pl.seg[g + 1] && pl.node[g] <= pl.node[g + 1], GSAT_ERR_ARG, "%s: host pointers are not monotone", who);
    GSAT_REQUIRE(pl.group_ptr[0] == 0 && pl.group_ptr[pl.n_groups] == G, GSAT_ERR_ARG, "%s: the groups do not cover the graphs", who);
    for (int64_t k = 0; k < pl.n_groups; ++k) {
        const int32_t g0 = pl.group_ptr[k], g1 = pl.group_ptr[k + 1];
        GSAT_REQUIRE(g0 < g1 && g1 <= G, GSAT_ERR_ARG, "%s: group %lld is empty or out of range", who, (long long)k);
        GSAT_REQUIRE((int64_t)pl.seg[g1] - pl.seg[g0] <= pl.scratch_rows, GSAT_ERR_ARG, "%s: group %lld has more rows than the scratch", who, (long long)k);
    }
    return GSAT_OK;
}

static size_t st_fwd_bytes(const gsat_attn_args* a, int64_t scratch_rows) {
    return align_up((size_t)scratch_rows * a->C1 * 4, 256) + align_up(st_part_floats(a, scratch_rows) * 4, 256) + 256;
}

}  // namespace gsat

extern "C" {

int gsat_attn_stream_plan(const int32_t* seg_ptr, int64_t G, int64_t budget, int32_t* group_ptr, int64_t* n_groups, int64_t* scratch_rows) {
    GSAT_REQUIRE(G >= 0 && budget >= 1 && group_ptr && n_groups && scratch_rows && (seg_ptr || G == 0), GSAT_ERR_ARG,
                 "gsat_attn_stream_plan: null pointer, G < 0 or budget < 1");
    int64_t n = 0, largest = 0, rows = 0;        // rows of the open group
    group_ptr[0] = 0;
    for (int64_t g = 0; g < G; ++g) {
        const int64_t r = (int64_t)seg_ptr[g + 1] - seg_ptr[g];
        GSAT_REQUIRE(r >= 0, GSAT_ERR_ARG, "gsat_attn_stream_plan: seg_ptr is not monotone at %lld", (long long)g);
        if (r > 0 && rows > 0 && rows + r > budget) {        // close the open group in front of g; empty graphs never open one
            group_ptr[++n] = (int32_t)g;
            largest = std::max(largest, rows);
            rows = 0;
        }
        rows += r;
    }
    if (G > 0) { group_ptr[++n] = (int32_t)G; largest = std::max(largest, rows); }
    *n_groups = n;
    *scratch_rows = std::max<int64_t>(largest, 1);
    return GSAT_OK;
}

int gsat_attn_stream_check(const int32_t* src, const int32_t* dst, const int32_t* node_seg, const int32_t* seg_ptr, const int32_t* row_seg,
                           int64_t M, int64_t N, int64_t G, int32_t* verdict, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(M >= 0 && N >= 0 && G >= 0 && M < (1ll << 31) && N < (1ll << 31) && G < (1ll << 31), GSAT_ERR_ARG, "gsat_attn_stream_check: bad extents");
    GSAT_REQUIRE(verdict && (M == 0 || (src && dst && node_seg && seg_ptr && row_seg && N > 0 && G > 0)), GSAT_ERR_ARG,
                 "gsat_attn_stream_check: null pointer, or rows without nodes or graphs");
    k_st_check<<<1, 1024, 0, stream>>>(src, dst, node_seg, seg_ptr, row_seg, (int)M, (int)N, (int)G, verdict);
    GSAT_LAUNCH_CHECK();
    return GSAT_OK;
}

size_t gsat_attn_stream_fwd_workspace_bytes(const gsat_attn_args* a, int64_t scratch_rows) {
    if (!a || scratch_rows < 1) return 0;
    return st_fwd_bytes(a, scratch_rows);
}

int gsat_attn_stream_fwd(const gsat_attn_args* a, const int32_t* group_ptr, int64_t n_groups, const int32_t* seg_ptr_host,
                         const int32_t* node_ptr_host, int64_t scratch_rows, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(!a || a->edge_mode, GSAT_ERR_UNSUPPORTED, "gsat_attn_stream_fwd: edge mode only (node mode keeps no [M, C1] tensor worth streaming)");
    int rc = check_args(a, "gsat_attn_stream_fwd");
    if (rc) return rc;
    const StPlan pl{group_ptr, n_groups, seg_ptr_host, node_ptr_host, scratch_rows};
    if ((rc = st_check(a, pl, "gsat_attn_stream_fwd"))) return rc;
    if (a->M == 0) return GSAT_OK;
    const int64_t M = a->M, N = a->N, G = a->G;
    const int H = a->H, C1 = a->C1, C2 = a->C2;
    GSAT_REQUIRE(a->fwd_workspace && a->fwd_workspace_bytes >= st_fwd_bytes(a, scratch_rows), GSAT_ERR_WORKSPACE,
                 "gsat_attn_stream_fwd: workspace %zu < %zu", a->fwd_workspace_bytes, st_fwd_bytes(a, scratch_rows));
    Arena ar(a->fwd_workspace, a->fwd_workspace_bytes);
    float* a1s = ar.take<float>((size_t)scratch_rows * C1);
    float* part = ar.take<float>(st_part_floats(a, scratch_rows));
    GSAT_REQUIRE(ar.ok(), GSAT_ERR_WORKSPACE, "gsat_attn_stream_fwd: workspace too small");
    float* mean1 = a->stats;
    float* rstd1 = mean1 + (size_t)G * C1;
    // ---- layer 1 on nodes, as staged ------------------------------------------------------------
    if ((rc = gemm_rm(stream, false, true, N, C1, H, a->emb, H, a->W1, 2 * H, 0.f, a->P, C1))) return rc;
    if ((rc = gemm_rm(stream, false, true, N, C1, H, a->emb, H, a->W1 + H, 2 * H, 0.f, a->Q, C1))) return rc;
    const PreAct<true> pre{a->P, a->Q, a->b1, a->src, a->dst, C1};
    const SeedRef sref{a->seed, a->seed_dev};
    const unsigned ctiles = (unsigned)ceil_div(C1, 4 * SB_LANES);
    const int cap = (int)scratch_rows;
    for (int64_t k = 0; k < n_groups; ++k) {
        const int g0 = group_ptr[k], ng = group_ptr[k + 1] - g0;
        const int r0 = seg_ptr_host[g0], rows = seg_ptr_host[g0 + ng] - r0;
        const int Zg = seg_slices(rows, ng);
        if (Zg == 1) {          // statistics and activation in one launch (graphs without rows get their statistics too)
            k_st_l1_fwd<<<dim3((unsigned)ng, ctiles, 1), SB, 0, stream>>>(pre, a->seg_ptr, g0, r0, cap, mean1, rstd1, a->mask1, sref, a->p_drop, a->training, a1s);
        } else {
            const dim3 grid((unsigned)ng, ctiles, (unsigned)Zg);
            const unsigned cb = (unsigned)ceil_div((int64_t)ng * C1, 256);
            k_st_l1_partial<<<grid, SB, 0, stream>>>(pre, a->seg_ptr, g0, nullptr, part);
            k_st_zcombine<<<cb, 256, 0, stream>>>(part, a->seg_ptr, g0, g0, ng, Zg, C1, 1, mean1);
            k_st_l1_partial<<<grid, SB, 0, stream>>>(pre, a->seg_ptr, g0, mean1, part);
            k_st_zcombine<<<cb, 256, 0, stream>>>(part, a->seg_ptr, g0, g0, ng, Zg, C1, 2, rstd1);
            k_st_l1_apply<<<ew_blocks((int64_t)rows * (C1 / 4)), 256, 0, stream>>>(pre, a->row_seg, mean1, rstd1, a->mask1, sref, a->p_drop, a->training, r0, rows, cap, a1s);
        }
        GSAT_LAUNCH_CHECK();
        if (rows > 0 && (rc = gemm_rm(stream, false, true, rows, C2, C1, a1s, C1, a->W2, C1, 0.f, a->h2 + (size_t)r0 * C2, C2))) return rc;
    }
    // ---- layer 2, head and sampler over the whole batch, as staged -------------------------------
    return attn_fwd_tail(stream, a, seg_slices(M, G), part);
}

size_t gsat_attn_stream_bwd_workspace_bytes(const gsat_attn_args* a, const int32_t* group_ptr, int64_t n_groups, const int32_t* seg_ptr_host,
                                            int64_t scratch_rows) {
    if (!a || scratch_rows < 1 || !group_ptr || !seg_ptr_host || n_groups < 0) return 0;
    const size_t M = (size_t)a->M, N = (size_t)a->N, G = (size_t)a->G, C1 = a->C1, C2 = a->C2, R = (size_t)scratch_rows;
    const size_t cmax = C1 > C2 ? C1 : C2;
    size_t gw2 = 0;                       // split-K slabs of dW2: the largest any group asks for
    for (int64_t k = 0; k < n_groups; ++k)
        gw2 = std::max(gw2, gemm_wgrad_workspace_floats(a->C2, a->C1, (int64_t)seg_ptr_host[group_ptr[k + 1]] - seg_ptr_host[group_ptr[k]]));
    size_t b = 0;
    b += align_up((M > G ? M : G) * 4, 256);   // dz
    b += align_up(M * C2 * 4, 256);            // dh2
    b += 2 * align_up(R * C1 * 4, 256);        // a1 and da1 -> dh1 of ONE group
    b += 2 * align_up(G * C1 * 4, 256);        // S1', S2' of a group's graphs
    b += 3 * align_up(G * C2 * 4, 256);        // S1, S2, dw3 partial
    b += align_up(256 * cmax * 4, 256);        // column-sum scratch
    b += 3 * align_up(st_part_floats(a, scratch_rows) * 4, 256);      // sliced-segment partials
    b += 2 * align_up(N * C1 * 4, 256);        // dP, dQ
    b += align_up((size_t)st_max_items(scratch_rows) * C1 * 4, 256);  // hub partials of one group
    b += align_up(align_up(gw2, 64) * 4, 256) + 2 * align_up(attn_gemm_ws_w1(a) * 4, 256);
    if (dual_gemm_ok(2, a->N, a->C1, a->H, a->H)) b += align_up(dual_gemm_ws_bytes(2, a->C1, a->H, a->H), 256);      // opt-in dual tile GEMM of demb | dW1
    return b + 1024;
}

int gsat_attn_stream_bwd(const gsat_attn_args* a, const gsat_attn_grads* gr, const int32_t* group_ptr, int64_t n_groups,
                         const int32_t* seg_ptr_host, const int32_t* node_ptr_host, int64_t scratch_rows, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GSAT_REQUIRE(!a || a->edge_mode, GSAT_ERR_UNSUPPORTED, "gsat_attn_stream_bwd: edge mode only (node mode keeps no [M, C1] tensor worth streaming)");
    int rc = check_args(a, "gsat_attn_stream_bwd");
    if (rc) return rc;
    GSAT_REQUIRE(gr && gr->demb && gr->dW1 && gr->db1 && gr->dW2 && gr->db2 && gr->dW3 && gr->db3, GSAT_ERR_ARG, "gsat_attn_stream_bwd: null gradient output");
    const StPlan pl{group_ptr, n_groups, seg_ptr_host, node_ptr_host, scratch_rows};
    if ((rc = st_check(a, pl, "gsat_attn_stream_bwd"))) return rc;
    if (a->M == 0) return attn_bwd_zero(stream, a, gr);
    const int64_t M = a->M, N = a->N, G = a->G;
    const int H = a->H, C1 = a->C1, C2 = a->C2;
    GSAT_REQUIRE(gr->dlogits || gr->datt, GSAT_ERR_ARG, "gsat_attn_stream_bwd: need dlogits and/or datt");
    GSAT_REQUIRE(!gr->datt || a->att, GSAT_ERR_ARG, "gsat_attn_stream_bwd: datt given but att was not saved");
    GSAT_REQUIRE(gr->rowptr_src && gr->eid_by_src && gr->rowptr_dst && gr->eid_by_dst, GSAT_ERR_ARG, "gsat_attn_stream_bwd: needs both CSRs");
    size_t gw2 = 0;
    for (int64_t k = 0; k < n_groups; ++k)
        gw2 = std::max(gw2, gemm_wgrad_workspace_floats(C2, C1, (int64_t)seg_ptr_host[group_ptr[k + 1]] - seg_ptr_host[group_ptr[k]]));
    const int max_items = (int)st_max_items(scratch_rows);
    Arena ar(gr->workspace, gr->workspace_bytes);
    float* dz = ar.take<float>(std::max<int64_t>(M, G));
    float* dh2 = ar.take<float>((size_t)M * C2);
    float* a1s = ar.take<float>((size_t)scratch_rows * C1);
    float* da1s = ar.take<float>((size_t)scratch_rows * C1);
    float* S1p = ar.take<float>((size_t)G * C1);
    float* S2p = ar.take<float>((size_t)G * C1);
    float* S1 = ar.take<float>((size_t)G * C2);
    float* S2 = ar.take<float>((size_t)G * C2);
    float* dw3p = ar.take<float>((size_t)G * C2);
    float* scratch = ar.take<float>((size_t)256 * std::max(C1, C2));
    const size_t npart = st_part_floats(a, scratch_rows);
    float *zp1 = ar.take<float>(npart), *zp2 = ar.take<float>(npart), *zp3 = ar.take<float>(npart);
    float* dP = ar.take<float>((size_t)N * C1);
    float* dQ = ar.take<float>((size_t)N * C1);
    float* lpart = ar.take<float>((size_t)max_items * C1);
    GemmWs gws{nullptr, align_up(gw2, 64)}, gws1{nullptr, attn_gemm_ws_w1(a)}, gws1b{nullptr, attn_gemm_ws_w1(a)};
    gws.ptr = ar.take<float>(gws.floats);
    gws1.ptr = ar.take<float>(gws1.floats);
    gws1b.ptr = ar.take<float>(gws1b.floats);
    const bool dual1 = dual_gemm_ok(2, N, C1, H, H);
    const size_t dws_bytes = dual1 ? dual_gemm_ws_bytes(2, C1, H, H) : 0;
    char* dws = dual1 ? ar.take<char>(dws_bytes) : nullptr;
    GSAT_REQUIRE(ar.ok(), GSAT_ERR_WORKSPACE, "gsat_attn_stream_bwd: workspace %zu < %zu", gr->workspace_bytes, ar.off);
    float* mean1 = a->stats;
    float* rstd1 = mean1 + (size_t)G * C1;
    const float sc = (a->training && a->p_drop > 0.f) ? 1.f / (1.f - a->p_drop) : 1.f;
    // ---- dz, db3, dW3, dh2 over the whole batch, as staged ---------------------------------------
    const int Z = seg_slices(M, G);
    if ((rc = attn_bwd_head(stream, a, gr, Z, bwd_merged_ok(a, Z), dz, dh2, S1, S2, dw3p, scratch, zp1, zp2, zp3))) return rc;
    // ---- the junction, group by group ------------------------------------------------------------
    const PreAct<true> pre{a->P, a->Q, a->b1, a->src, a->dst, C1};
    const SeedRef sref{a->seed, a->seed_dev};
    const unsigned ctiles = (unsigned)ceil_div(C1, 4 * SB_LANES);
    const int cap = (int)scratch_rows;
    bool first = true;
    for (int64_t k = 0; k < n_groups; ++k) {
        const int g0 = group_ptr[k], ng = group_ptr[k + 1] - g0;
        const int r0 = seg_ptr_host[g0], rows = seg_ptr_host[g0 + ng] - r0;
        const int n0 = node_ptr_host[g0], n1 = node_ptr_host[g0 + ng];
        if (rows > 0) {
            // (i) a1 of the group again: the same keep decisions, keyed by the global row
            k_st_l1_apply<<<ew_blocks((int64_t)rows * (C1 / 4)), 256, 0, stream>>>(pre, a->row_seg, mean1, rstd1, a->mask1, sref, a->p_drop, a->training, r0, rows, cap, a1s);
            GSAT_LAUNCH_CHECK();
            // (ii) dW2 (+)= dh2[r0:r1]^T a1 (its ordered slab sum is done before the next group reuses the slabs) ; da1 = dh2[r0:r1] W2
            const float* dh2g = dh2 + (size_t)r0 * C2;
            if ((rc = gemm_rm(stream, true, false, C2, C1, rows, dh2g, C2, a1s, C1, first ? 0.f : 1.f, gr->dW2, C1, gws, true))) return rc;
            if ((rc = gemm_rm(stream, false, false, rows, C1, C2, dh2g, C2, a->W2, C1, 0.f, da1s, C1, GemmWs{nullptr, 0}, true))) return rc;
            first = false;
            // (iii) S1', S2' of the group's graphs and dh1 in place over da1
            const int Zg = seg_slices(rows, ng);
            const dim3 grid((unsigned)ng, ctiles, (unsigned)Zg);
            if (Zg == 1) {
                k_st_l1_bwd<true><<<grid, SB, 0, stream>>>(da1s, a1s, a->seg_ptr, g0, r0, cap, sc, S1p, S2p, pre, mean1, rstd1);
            } else {
                const unsigned cb = (unsigned)ceil_div((int64_t)ng * C1, 256);
                k_st_l1_bwd<false><<<grid, SB, 0, stream>>>(da1s, a1s, a->seg_ptr, g0, r0, cap, sc, zp1, zp2, pre, mean1, rstd1);
                k_st_zcombine<<<cb, 256, 0, stream>>>(zp1, a->seg_ptr, g0, 0, ng, Zg, C1, 1, S1p);
                k_st_zcombine<<<cb, 256, 0, stream>>>(zp2, a->seg_ptr, g0, 0, ng, Zg, C1, 1, S2p);
                k_st_dh1<<<ew_blocks((int64_t)rows * (C1 / 4)), 256, 0, stream>>>(pre, a->row_seg, mean1, rstd1, a1s, sc, S1p, S2p, g0, ng, r0, rows, cap, da1s);
            }
            GSAT_LAUNCH_CHECK();
        }
        // (iv) dP, dQ of the group's nodes (nodes of graphs without edges: exact zeros)
        if (n1 > n0) {
            const int nb = ew_blocks((int64_t)(n1 - n0) * (C1 / 4));
            const bool hubs = rows > ST_CH;            // no row of the group can be long otherwise
            const int cbk = ew_blocks((int64_t)max_items * (C1 / 4));
            const int32_t* cps = hubs ? gr->chunk_ptr_src : nullptr;
            const int32_t* cpd = hubs ? gr->chunk_ptr_dst : nullptr;
            if (cps) k_st_gather_chunk<<<cbk, 256, 0, stream>>>(da1s, gr->rowptr_src, gr->eid_by_src, cps, n0, n1, r0, rows, C1, max_items, lpart);
            k_st_gather<<<nb, 256, 0, stream>>>(da1s, gr->rowptr_src, gr->eid_by_src, cps, lpart, n0, n1, r0, rows, C1, max_items, dP);
            if (cpd) k_st_gather_chunk<<<cbk, 256, 0, stream>>>(da1s, gr->rowptr_dst, gr->eid_by_dst, cpd, n0, n1, r0, rows, C1, max_items, lpart);
            k_st_gather<<<nb, 256, 0, stream>>>(da1s, gr->rowptr_dst, gr->eid_by_dst, cpd, lpart, n0, n1, r0, rows, C1, max_items, dQ);
            GSAT_LAUNCH_CHECK();
        }
    }
    if (first) GSAT_CHECK_HIP(gsat::zero_async(gr->dW2, sizeof(float) * C2 * C1, stream));
    // ---- demb, dW1 over all nodes, as staged -----------------------------------------------------
    SlabJob jobs[3] = {};
    if ((rc = attn_bwd_edge_nodes(stream, a, gr, dual1, dP, dQ, dws, dws_bytes, gws1, gws1b, jobs))) return rc;
    return slab_reduce_jobs(stream, jobs, 3);
}

}  // extern "C"
