// The frequencies columns of LogUp lookups on gfx950 (starkhip_logup_frequencies and "fill_frequencies"; logup_frequencies.h has the
// rule, DESIGN.md 14a the arguments).  Only the TABLE of a lookup is sorted -- n items, once per distinct table column of a batch --
// not its m n looked-up cells:
//
//  * logup_freq_keys_kernel: one lane per table row; key = the cell reduced mod p, idx = the row.  The stable sort of
//    kernels_multiset.hip follows, so the first position of a run of equal keys holds the lowest row with that value.
//  * logup_freq_count_kernel: one lane per looked-up cell (grid.y = looked-up column of the batch).  A lower bound in the sorted keys,
//    at most 21 steps; a hit adds 1 to a uint32 count at that position -- always the first of its run, so no other position of a run
//    ever counts.  A miss sets the row's bit: the 64 rows of a wave are one mask word, so the wave's ballot goes out as one 64-bit
//    atomicOr, and its popcount is added to the lookup's and the column's counters.  Integer adds and ors alone: no result depends on
//    the order of arrival, no destination does either, and no workgroup waits for another.
//    A range check whose limbs are mostly one value sends every lane of the chip to one address.  The COMBINE form takes up to
//    LOGUP_FREQ_ROUNDS distinct positions out of a wave, each with one add of its lane count (the first pending lane's position, the
//    ballot of the lanes that share it), before the remaining lanes add alone; the plain form is kept for the measurement.
//  * logup_freq_write_kernel: one lane per sorted position: f[idx[pos]] = count[pos].  idx is a permutation of the rows, so every row
//    is written exactly once and the column needs no zero-fill.  In the caller's trace a lookup with a nonzero missing count on the
//    device returns before writing.
//  * logup_freq_keys_general_kernel, logup_freq_count_general_kernel: the same two for lookups over Columns and Filters (logup.h): a key
//    is the table Column's value on the row, a looked-up value its Column's, both walked from the batch's descriptor through the
//    trace's strides, the next row being (r + 1) & (n - 1).  A cell whose filter is 0 is neither counted nor missing; one whose filter
//    is neither 0 nor 1 is missing whatever its value.  What follows the value -- search, count, ballot -- is the plain kernel's code.
// Every index is bounded by the n the launch is given; the columns come from a validated program (air_validate.cpp) or are staged slots.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kernels_logup_freq.h"
#include "logup.h"

namespace starkhip {

static const unsigned LOGUP_FREQ_ROUNDS = 4;

__global__ __launch_bounds__(TILE_BLOCK) void logup_freq_keys_kernel(LogupFreqTrace t, uint32_t n, const uint32_t* __restrict__ table_cols, gl_t* __restrict__ keys,
                                                                     uint32_t* __restrict__ idx) { STARKHIP_PRIO_ENTRY
    const uint32_t r = blockIdx.x * TILE_BLOCK + threadIdx.x;
    if (r >= n) return;
    const size_t at = (size_t)blockIdx.y * n + r;
    keys[at] = gl_from_u64(t.base[table_cols[blockIdx.y] * t.col_stride + r * t.row_stride]);
    idx[at] = r;
}

// One looked-up cell per lane: `live` lanes search the sorted keys of their slot for v; a hit that is not `flagged` counts, any other
// live lane is missing.  Every lane of the wave comes here (ballots and shuffles).
template <bool COMBINE>
__device__ __forceinline__ void logup_freq_count_cell(bool live, bool flagged, gl_t v, uint32_t r, uint32_t n, uint32_t lk, uint32_t slot, uint32_t lookups,
                                                      const gl_t* __restrict__ keys, uint32_t* __restrict__ count, unsigned long long* __restrict__ mask,
                                                      uint32_t* __restrict__ missing) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t pos = n;
    bool hit = false;
    if (live && !flagged) {
        const gl_t* __restrict__ k = keys + (size_t)slot * n;
        uint32_t lo = 0, hi = n;  // the first position whose key is >= v
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (k[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        pos = lo;
        hit = pos < n && k[pos] == v;
    }
    uint32_t* __restrict__ cnt = count + (size_t)lk * n;
    bool todo = hit;
    if (COMBINE) {
        for (unsigned it = 0; it < LOGUP_FREQ_ROUNDS; it++) {
            const unsigned long long rest = __ballot(todo);
            if (!rest) break;
            const uint32_t first = (uint32_t)__ffsll((long long)rest) - 1;
            const uint32_t lead = (uint32_t)__shfl((int)pos, (int)first, 64);
            const bool same = todo && pos == lead;
            const unsigned long long m = __ballot(same);
            if (lane == first) atomicAdd(&cnt[lead], (uint32_t)__popcll(m));  // (lead < n: a pending lane's own position)
            todo = todo && !same;
        }
    }
    if (todo) atomicAdd(&cnt[pos], 1u);
    const unsigned long long gone = __ballot(live && !hit);  // lane i of a wave is row (r & ~63) + i: the ballot is the rows' mask word
    if (gone && lane == (uint32_t)__ffsll((long long)gone) - 1) {
        const uint32_t c = (uint32_t)__popcll(gone);
        atomicOr(&mask[(size_t)lk * ((n + 63) / 64) + (r >> 6)], gone);
        atomicAdd(&missing[lk], c);
        atomicAdd(&missing[lookups + blockIdx.y], c);
    }
}

template <bool COMBINE>
__global__ __launch_bounds__(TILE_BLOCK) void logup_freq_count_kernel(LogupFreqTrace t, uint32_t n, const uint32_t* __restrict__ cols, uint32_t lookups,
                                                                      const gl_t* __restrict__ keys, uint32_t* __restrict__ count,
                                                                      unsigned long long* __restrict__ mask, uint32_t* __restrict__ missing) { STARKHIP_PRIO_ENTRY
    const uint32_t r = blockIdx.x * TILE_BLOCK + threadIdx.x;
    const uint32_t col = cols[3 * blockIdx.y], lk = cols[3 * blockIdx.y + 1], slot = cols[3 * blockIdx.y + 2];
    const bool valid = r < n;
    const gl_t v = valid ? gl_from_u64(t.base[col * t.col_stride + r * t.row_stride]) : 0;
    logup_freq_count_cell<COMBINE>(valid, false, v, r, n, lk, slot, lookups, keys, count, mask, missing);
}

// desc: the batch's descriptor; offs[y]: where slot y's table COLUMN starts in it
__global__ __launch_bounds__(TILE_BLOCK) void logup_freq_keys_general_kernel(LogupFreqTrace t, uint32_t n, const uint32_t* __restrict__ desc, const uint32_t* __restrict__ offs,
                                                                             gl_t* __restrict__ keys, uint32_t* __restrict__ idx) { STARKHIP_PRIO_ENTRY
    const uint32_t r = blockIdx.x * TILE_BLOCK + threadIdx.x;
    if (r >= n) return;
    const uint32_t rn = (r + 1) & (n - 1);
    auto cell = [&](uint32_t col, bool next) { return gl_from_u64(t.base[col * t.col_stride + (next ? rn : r) * t.row_stride]); };
    const size_t at = (size_t)blockIdx.y * n + r;
    const uint32_t* w = desc + offs[blockIdx.y];
    keys[at] = logup_desc_column(w, cell);
    idx[at] = r;
}

// cols: n_cols x {where the value's COLUMN and FILTER start in desc, lookup of the batch, table slot of the batch}
template <bool COMBINE>
__global__ __launch_bounds__(TILE_BLOCK) void logup_freq_count_general_kernel(LogupFreqTrace t, uint32_t n, const uint32_t* __restrict__ desc,
                                                                              const uint32_t* __restrict__ cols, uint32_t lookups, const gl_t* __restrict__ keys,
                                                                              uint32_t* __restrict__ count, unsigned long long* __restrict__ mask,
                                                                              uint32_t* __restrict__ missing) { STARKHIP_PRIO_ENTRY
    const uint32_t r = blockIdx.x * TILE_BLOCK + threadIdx.x;
    const uint32_t lk = cols[3 * blockIdx.y + 1], slot = cols[3 * blockIdx.y + 2];
    const bool valid = r < n;
    gl_t v = 0, phi = 0;
    if (valid) {
        const uint32_t rn = (r + 1) & (n - 1);
        auto cell = [&](uint32_t col, bool next) { return gl_from_u64(t.base[col * t.col_stride + (next ? rn : r) * t.row_stride]); };
        const uint32_t* w = desc + cols[3 * blockIdx.y];
        v = logup_desc_column(w, cell);
        phi = logup_desc_filter(w, cell);
    }
    logup_freq_count_cell<COMBINE>(valid && phi != 0, phi != 1, v, r, n, lk, slot, lookups, keys, count, mask, missing);
}

__global__ __launch_bounds__(TILE_BLOCK) void logup_freq_write_kernel(LogupFreqTrace t, uint32_t n, const uint32_t* __restrict__ lks, const uint32_t* __restrict__ idx,
                                                                      const uint32_t* __restrict__ count, const uint32_t* __restrict__ gate) { STARKHIP_PRIO_ENTRY
    const uint32_t pos = blockIdx.x * TILE_BLOCK + threadIdx.x, lk = blockIdx.y;
    if (pos >= n) return;
    if (gate && gate[lk]) return;
    const uint32_t slot = lks[2 * lk], fcol = lks[2 * lk + 1];
    const uint32_t row = idx[(size_t)slot * n + pos];
    if (row < n) t.base[fcol * t.col_stride + row * t.row_stride] = count[(size_t)lk * n + pos];
}

hipError_t launch_logup_freq_keys(const LogupFreqTrace& t, size_t n, const uint32_t* table_cols, size_t slots, gl_t* keys, uint32_t* idx, hipStream_t st) {
    hipLaunchKernelGGL(logup_freq_keys_kernel, dim3(nb(n, TILE_BLOCK), (unsigned)slots), dim3(TILE_BLOCK), 0, st, t, (uint32_t)n, table_cols, keys, idx);
    return hipGetLastError();
}

hipError_t launch_logup_freq_count(const LogupFreqTrace& t, size_t n, const uint32_t* cols, size_t n_cols, size_t lookups, const gl_t* keys, uint32_t* count,
                                   unsigned long long* mask, uint32_t* missing, bool combine, hipStream_t st) {
    const dim3 grid(nb(n, TILE_BLOCK), (unsigned)n_cols), block(TILE_BLOCK);
    if (combine) hipLaunchKernelGGL(logup_freq_count_kernel<true>, grid, block, 0, st, t, (uint32_t)n, cols, (uint32_t)lookups, keys, count, mask, missing);
    else hipLaunchKernelGGL(logup_freq_count_kernel<false>, grid, block, 0, st, t, (uint32_t)n, cols, (uint32_t)lookups, keys, count, mask, missing);
    return hipGetLastError();
}

hipError_t launch_logup_freq_keys_general(const LogupFreqTrace& t, size_t n, const uint32_t* desc, const uint32_t* offs, size_t slots, gl_t* keys, uint32_t* idx,
                                          hipStream_t st) {
    hipLaunchKernelGGL(logup_freq_keys_general_kernel, dim3(nb(n, TILE_BLOCK), (unsigned)slots), dim3(TILE_BLOCK), 0, st, t, (uint32_t)n, desc, offs, keys, idx);
    return hipGetLastError();
}

hipError_t launch_logup_freq_count_general(const LogupFreqTrace& t, size_t n, const uint32_t* desc, const uint32_t* cols, size_t n_cols, size_t lookups, const gl_t* keys,
                                           uint32_t* count, unsigned long long* mask, uint32_t* missing, bool combine, hipStream_t st) {
    const dim3 grid(nb(n, TILE_BLOCK), (unsigned)n_cols), block(TILE_BLOCK);
    if (combine) hipLaunchKernelGGL(logup_freq_count_general_kernel<true>, grid, block, 0, st, t, (uint32_t)n, desc, cols, (uint32_t)lookups, keys, count, mask, missing);
    else hipLaunchKernelGGL(logup_freq_count_general_kernel<false>, grid, block, 0, st, t, (uint32_t)n, desc, cols, (uint32_t)lookups, keys, count, mask, missing);
    return hipGetLastError();
}

hipError_t launch_logup_freq_write(const LogupFreqTrace& t, size_t n, const uint32_t* lks, size_t lookups, const uint32_t* idx, const uint32_t* count,
                                   const uint32_t* gate, hipStream_t st) {
    hipLaunchKernelGGL(logup_freq_write_kernel, dim3(nb(n, TILE_BLOCK), (unsigned)lookups), dim3(TILE_BLOCK), 0, st, t, (uint32_t)n, lks, idx, count, gate);
    return hipGetLastError();
}

}  // namespace starkhip
