// Order-preserving stream compaction, the two pieces subgraph.hip and fidelity_stack.hip share: the rank of a thread's items among its
// workgroup's flagged items (wave64 ballots), and the exclusive scan of the workgroups' counts by one workgroup.  No atomics.
#pragma once
#include "common.h"

namespace gsat {

// Rank of this thread's first item among the workgroup's flagged items (items in thread order, IPT per thread, bit j of `bits` = item j
// is flagged), and the workgroup's total.  One ballot per item slot: the flagged items of the lanes below come out of popcounts of the
// masked ballots.  Every thread of the workgroup of BLOCK threads calls it; sh holds BLOCK / 64 ints.
template <int IPT, int BLOCK>
__device__ __forceinline__ int block_rank(uint32_t bits, int* sh, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    int before = 0, wave_total = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const uint64_t m = __ballot((bits >> j) & 1u);
        before += __popcll(m & below);
        wave_total += __popcll(m);
    }
    __syncthreads();
    if (lane == 0) sh[wave] = wave_total;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
        const int c = sh[w];
        if (w < wave) base += c;
        total += c;
    }
    return base + before;
}

// exclusive scan of a[0 .. n) in place by the one workgroup of BLOCK threads; returns the total in every thread; sh holds BLOCK / 64 ints
template <int BLOCK>
__device__ __forceinline__ int scan_counts(int32_t* __restrict__ a, int n, int* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += BLOCK) {
        const int i = base + (int)threadIdx.x;
        const int v = i < n ? a[i] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) sh[wave] = incl;
        __syncthreads();
        int wave_base = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) {
            const int c = sh[w];
            if (w < wave) wave_base += c;
            tot += c;
        }
        if (i < n) a[i] = carry + wave_base + incl - v;
        carry += tot;
        __syncthreads();
    }
    return carry;
}

}  // namespace gsat
