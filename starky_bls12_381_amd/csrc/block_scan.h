// What the kernels over sorted (key, idx) items share (kernels_multiset.hip, kernels_lookup.hip) and, of it, the scan that the
// permutation arguments' prefix product uses too (kernels_permutation.hip): the tile, the workgroup scan, the end of a run of equal keys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gl.h"

namespace starkhip {

// THE tile: a workgroup of TILE_BLOCK lanes owns TILE_ITEMS consecutive items as TILE_SLOTS wave-sized slots.  Slot s belongs to wave
// s % TILE_WAVES in its round s / TILE_WAVES -- tile_slot(round, wave) -- so in every round the workgroup reads TILE_BLOCK adjacent
// items, and slots in ascending order are items in ascending order.
static const unsigned TILE_ITEMS = 1024, TILE_BLOCK = 256, TILE_WAVES = TILE_BLOCK / 64, TILE_SLOTS = TILE_ITEMS / 64, TILE_ROUNDS = TILE_SLOTS / TILE_WAVES;
inline size_t tile_count(size_t items) { return (items + TILE_ITEMS - 1) / TILE_ITEMS; }
__device__ __forceinline__ unsigned tile_slot(unsigned round, unsigned wave) { return round * TILE_WAVES + wave; }

struct ScanAdd { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct ScanMul { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return gl_mul(a, b); } };

// Exclusive scan of v under the associative `op` over the workgroup's TILE_BLOCK lanes, in lane order, and *total = all of them
// combined: wave scans through __shfl_up, the waves' totals through LDS.  lds: TILE_WAVES words.  Every lane of the workgroup calls it.
template <typename T, typename Op>
__device__ __forceinline__ T block_scan(T v, Op op, T identity, T* lds, T* total) {
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(incl, d, 64);
        if (lane >= d) incl = op(t, incl);
    }
    T excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = identity;
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    T before = identity, all = identity;
#pragma unroll
    for (unsigned k = 0; k < TILE_WAVES; k++) {
        const T t = lds[k];
        if (k < w) before = op(before, t);
        all = op(all, t);
    }
    __syncthreads();  // lds is free for the next call
    *total = all;
    return op(before, excl);
}

// keys [items] ascending, j < items, k = keys[j] (the caller holds it: one load): the end of j's run of equal keys -- the first position
// after j whose key is > k
__device__ __forceinline__ uint32_t sorted_run_end(const gl_t* __restrict__ keys, gl_t k, uint32_t j, uint32_t items) {
    uint32_t lo = j + 1, hi = items;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace starkhip
