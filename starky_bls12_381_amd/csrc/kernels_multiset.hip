// Multiset comparison of the two sides of a permutation pair on gfx950 (starkhip_check_trace_permutations; permutation_check.h has
// the rule, DESIGN.md 13a the arguments):
//
//  * multiset_keys_kernel: one lane per item i = side * n + row.  The pair columns are read column-major -- adjacent lanes, adjacent
//    words -- and reduced mod p as every trace reader does; key = sum_t seed^t cell_t, canonical, and idx = i.  The order the sort
//    starts from is therefore: all lhs rows ascending, then all rhs rows ascending.
//  * a STABLE least-significant-digit radix sort of (key, idx) by key: 8-bit digits, eight passes between two buffers, each pass four
//    launches on the caller's stream.  A workgroup owns a tile of MULTISET_TILE consecutive items as 16 slots of 64, slot s of wave
//    s & 3 in its round s >> 2: the tile of block_scan.h, which also has the workgroup scan the table scan is made of.
//      - multiset_histogram_kernel: the tile's digit counts through LDS counters into table[digit][tile];
//      - multiset_scan_sums_kernel + multiset_scan_apply_kernel: the exclusive scan of the table in digit-major order -- the sum of
//        each chunk of MULTISET_SCAN_CHUNK words, then every chunk scanned in place from the sum of the chunks before it (a table
//        of one chunk, up to 8192 rows, needs no sums: three launches);
//      - multiset_scatter_kernel: an item lands at table[digit][tile] + (items of the digit in earlier slots of the tile) + (items of
//        the digit in lower lanes of its slot).  The last comes from eight __ballots -- the lanes whose digit matches bit by bit -- and
//        a popcount of the lower lanes, the middle one from per-slot digit counts in LDS.  Every term counts items that PRECEDE the
//        item in the input among those of its digit, so equal digits keep their order: the pass is stable, and so is the sort.
//    No workgroup waits for another inside a launch, and no global atomic decides where an item lands: the destination is a function
//    of the input order alone.
//  * multiset_classify_kernel: one lane per sorted position.  Binary searches by key for the start and the end (sorted_run_end) of the item's run, and
//    by the side bit of idx -- monotone inside a run because the sort is stable -- for the run's first rhs item; from these L, R and
//    the item's rank on its side: it is unmatched when that rank is >= the other side's count, i.e. the |L - R| highest rows of the
//    larger side are.  An item whose key equals its predecessor's compares its tuple with the predecessor's cell by cell mod p; a
//    difference is a collision of two tuples under this seed and the host reruns the pair under the next.  Mask bits through 64-bit
//    atomicOr and one collision counter: both independent of the order of arrival.
//  * multiset_count_kernel: the popcounts of the two masks.
// Every index is bounded by the item count the launch is given; the columns come from a validated program (air_validate.cpp).
#include <hip/hip_runtime.h>

#include <utility>

#include "block_scan.h"
#include "kernels.h"
#include "kernels_multiset.h"

namespace starkhip {

static const unsigned MS_SCAN_ITEMS = MULTISET_SCAN_CHUNK / TILE_BLOCK;
static_assert(TILE_BLOCK == 256, "one lane per digit in the scatter's slot scan");

// the lanes of the wave that are `valid` and hold the same 8-bit digit as this one
__device__ __forceinline__ unsigned long long ms_match(unsigned d, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (unsigned b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// pair: n_entries, then n_entries x (lhs, rhs) columns of `cols`.  grid.y: the sets of a batch -- set y has its descriptor at
// pair + y * pair_stride and its items at keys / idx + y * 2 n (every kernel of the sort strides by the set's item count alike)
__global__ __launch_bounds__(TILE_BLOCK) void multiset_keys_kernel(const uint32_t* __restrict__ pair, uint32_t pair_stride, const gl_t* __restrict__ cols, size_t stride,
                                                                   uint32_t n, gl_t seed, gl_t* __restrict__ keys, uint32_t* __restrict__ idx) { STARKHIP_PRIO_ENTRY
    const uint32_t i = blockIdx.x * TILE_BLOCK + threadIdx.x;
    if (i >= 2 * n) return;
    pair += (size_t)blockIdx.y * pair_stride;
    keys += (size_t)blockIdx.y * 2 * n;
    idx += (size_t)blockIdx.y * 2 * n;
    const uint32_t side = i >= n, row = i - side * n, ne = pair[0];
    gl_t key = 0, pw = 1;
    for (uint32_t e = 0; e < ne; e++) {
        const gl_t v = gl_from_u64(cols[pair[1 + 2 * e + side] * stride + row]);
        key = gl_add(key, gl_mul(v, pw));
        pw = gl_mul(pw, seed);
    }
    keys[i] = key;
    idx[i] = i;
}

// table[digit][tile] = the tile's items of that digit.  grid: tiles x sets, set y with its own table of 256 tiles words
__global__ __launch_bounds__(TILE_BLOCK) void multiset_histogram_kernel(const gl_t* __restrict__ keys, uint32_t items, unsigned shift, uint32_t* __restrict__ table,
                                                                        uint32_t tiles) { STARKHIP_PRIO_ENTRY
    __shared__ uint32_t hist[256];
    keys += (size_t)blockIdx.y * items;
    table += (size_t)blockIdx.y * 256 * tiles;
    const unsigned lane = threadIdx.x & 63u;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * MULTISET_TILE;
#pragma unroll
    for (unsigned r = 0; r < TILE_ROUNDS; r++) {
        const uint32_t pos = base + r * TILE_BLOCK + threadIdx.x;
        const bool valid = pos < items;
        const unsigned d = valid ? (unsigned)(keys[pos] >> shift) & 255u : 0u;
        const unsigned long long m = ms_match(d, valid);
        if (valid && (m & ((1ull << lane) - 1)) == 0) atomicAdd(&hist[d], (uint32_t)__popcll(m));  // a count: the order of the adds does not matter
    }
    __syncthreads();
    table[(size_t)threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

// sums[chunk] = the sum of the chunk's words.  grid: chunks x sets, set y with its own `words` of table and gridDim.x of sums
__global__ __launch_bounds__(TILE_BLOCK) void multiset_scan_sums_kernel(const uint32_t* __restrict__ table, uint32_t words, uint32_t* __restrict__ sums) { STARKHIP_PRIO_ENTRY
    __shared__ uint32_t lds[TILE_WAVES];
    table += (size_t)blockIdx.y * words;
    sums += (size_t)blockIdx.y * gridDim.x;
    const uint32_t base = blockIdx.x * MULTISET_SCAN_CHUNK;
    uint32_t s = 0;
#pragma unroll
    for (unsigned k = 0; k < MS_SCAN_ITEMS; k++) {
        const uint32_t j = base + k * TILE_BLOCK + threadIdx.x;
        if (j < words) s += table[j];
    }
    uint32_t total;
    (void)block_scan(s, ScanAdd(), 0u, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// table[j] <- the sum of table[0 .. j), chunk by chunk: each lane a run of MS_SCAN_ITEMS consecutive words.  grid: chunks x sets
__global__ __launch_bounds__(TILE_BLOCK) void multiset_scan_apply_kernel(uint32_t* __restrict__ table, uint32_t words, const uint32_t* __restrict__ sums) { STARKHIP_PRIO_ENTRY
    __shared__ uint32_t lds[TILE_WAVES];
    table += (size_t)blockIdx.y * words;
    sums += (size_t)blockIdx.y * gridDim.x;
    uint32_t s = 0, carry;
    for (uint32_t j = threadIdx.x; j < blockIdx.x; j += TILE_BLOCK) s += sums[j];
    (void)block_scan(s, ScanAdd(), 0u, lds, &carry);
    const uint32_t j0 = blockIdx.x * MULTISET_SCAN_CHUNK + threadIdx.x * MS_SCAN_ITEMS;
    uint32_t v[MS_SCAN_ITEMS];
    s = 0;
#pragma unroll
    for (unsigned k = 0; k < MS_SCAN_ITEMS; k++) {
        v[k] = j0 + k < words ? table[j0 + k] : 0u;
        s += v[k];
    }
    uint32_t total;
    uint32_t run = carry + block_scan(s, ScanAdd(), 0u, lds, &total);
#pragma unroll
    for (unsigned k = 0; k < MS_SCAN_ITEMS; k++) {
        if (j0 + k < words) table[j0 + k] = run;
        run += v[k];
    }
}

// table: scanned.  grid: tiles x sets
__global__ __launch_bounds__(TILE_BLOCK) void multiset_scatter_kernel(const gl_t* __restrict__ keys_in, const uint32_t* __restrict__ idx_in, gl_t* __restrict__ keys_out,
                                                                      uint32_t* __restrict__ idx_out, uint32_t items, unsigned shift,
                                                                      const uint32_t* __restrict__ table, uint32_t tiles) { STARKHIP_PRIO_ENTRY
    __shared__ uint32_t cnt[TILE_SLOTS][256];  // the slot's items of each digit, then where the slot's first item of the digit lands
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    {
        const size_t at = (size_t)blockIdx.y * items;
        keys_in += at, idx_in += at, keys_out += at, idx_out += at;
        table += (size_t)blockIdx.y * 256 * tiles;
    }
#pragma unroll
    for (unsigned s = 0; s < TILE_SLOTS; s++) cnt[s][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * MULTISET_TILE;
    gl_t key[TILE_ROUNDS];
    uint32_t id[TILE_ROUNDS], dr[TILE_ROUNDS];  // digit | rank inside the slot << 8
#pragma unroll
    for (unsigned r = 0; r < TILE_ROUNDS; r++) {
        const unsigned slot = tile_slot(r, w);
        const uint32_t pos = base + slot * 64 + lane;
        const bool valid = pos < items;
        key[r] = valid ? keys_in[pos] : 0;
        id[r] = valid ? idx_in[pos] : 0u;
        const unsigned d = (unsigned)(key[r] >> shift) & 255u;
        const unsigned long long m = ms_match(d, valid);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (valid && rank == 0) cnt[slot][d] = (uint32_t)__popcll(m);
        dr[r] = d | rank << 8;
    }
    __syncthreads();
    {
        uint32_t run = table[(size_t)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
        for (unsigned s = 0; s < TILE_SLOTS; s++) {
            const uint32_t c = cnt[s][threadIdx.x];
            cnt[s][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (unsigned r = 0; r < TILE_ROUNDS; r++) {
        const unsigned slot = tile_slot(r, w);
        const uint32_t pos = base + slot * 64 + lane;
        const uint32_t dst = cnt[slot][dr[r] & 255u] + (dr[r] >> 8);
        if (pos < items && dst < items) {
            keys_out[dst] = key[r];
            idx_out[dst] = id[r];
        }
    }
}

__global__ __launch_bounds__(TILE_BLOCK) void multiset_classify_kernel(const uint32_t* __restrict__ pair, const gl_t* __restrict__ cols, size_t stride, uint32_t n,
                                                                       const gl_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                                       unsigned long long* __restrict__ masks, unsigned long long* __restrict__ counters) { STARKHIP_PRIO_ENTRY
    const uint32_t items = 2 * n, j = blockIdx.x * TILE_BLOCK + threadIdx.x;
    const bool valid = j < items;
    bool collision = false;
    if (valid) {
        const gl_t k = keys[j];
        uint32_t lo = 0, hi = j;  // the run's start: the first position whose key is >= k
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (keys[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t a = lo;
        const uint32_t b = sorted_run_end(keys, k, j, items);
        lo = a, hi = b;  // the run's first rhs item
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (idx[mid] < n) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t m = lo, L = m - a, R = b - m;
        const uint32_t id = idx[j], side = id >= n, row = id - side * n;
        const uint32_t rank = side ? j - m : j - a, other = side ? L : R;
        if (rank >= other) atomicOr(&masks[(size_t)side * ((n + 63) / 64) + (row >> 6)], 1ull << (row & 63u));
        const uint32_t ne = pair[0];
        if (j > a && ne > 1) {  // (one entry: the key is the cell)
            const uint32_t pid = idx[j - 1], pside = pid >= n, prow = pid - pside * n;
            for (uint32_t e = 0; e < ne && !collision; e++)
                collision = gl_from_u64(cols[pair[1 + 2 * e + side] * stride + row]) != gl_from_u64(cols[pair[1 + 2 * e + pside] * stride + prow]);
        }
    }
    const unsigned long long hit = __ballot(collision);
    if (collision && (hit & ((1ull << (threadIdx.x & 63u)) - 1)) == 0) atomicAdd(&counters[0], (unsigned long long)__popcll(hit));
}

__global__ __launch_bounds__(TILE_BLOCK) void multiset_count_kernel(const unsigned long long* __restrict__ masks, uint32_t words_per_side,
                                                                    unsigned long long* __restrict__ counters) { STARKHIP_PRIO_ENTRY
    const uint32_t j = blockIdx.x * TILE_BLOCK + threadIdx.x;
    const uint32_t c = j < 2 * words_per_side ? (uint32_t)__popcll(masks[j]) : 0u;
    uint32_t c0 = j < words_per_side ? c : 0u, c1 = c - c0;
#pragma unroll
    for (unsigned d = 32; d; d >>= 1) {
        c0 += __shfl_down(c0, d, 64);
        c1 += __shfl_down(c1, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (c0) atomicAdd(&counters[1], (unsigned long long)c0);
        if (c1) atomicAdd(&counters[2], (unsigned long long)c1);
    }
}

hipError_t launch_multiset_keys_batch(const uint32_t* pair, uint32_t pair_stride, size_t sets, const gl_t* cols, size_t stride, size_t n, gl_t seed, gl_t* keys,
                                      uint32_t* idx, hipStream_t st) {
    hipLaunchKernelGGL(multiset_keys_kernel, dim3(nb(2 * n, TILE_BLOCK), (unsigned)sets), dim3(TILE_BLOCK), 0, st, pair, pair_stride, cols, stride, (uint32_t)n, seed,
                       keys, idx);
    return hipGetLastError();
}

hipError_t launch_multiset_keys(const uint32_t* pair, const gl_t* cols, size_t stride, size_t n, gl_t seed, gl_t* keys, uint32_t* idx, hipStream_t st) {
    return launch_multiset_keys_batch(pair, 0, 1, cols, stride, n, seed, keys, idx, st);
}

hipError_t launch_multiset_sort_batch(gl_t* keys, uint32_t* idx, gl_t* keys_alt, uint32_t* idx_alt, size_t items, size_t sets, uint32_t* table, uint32_t* sums,
                                      hipStream_t st) {
    const uint32_t tiles = (uint32_t)multiset_tiles(items), words = (uint32_t)multiset_table_words(items), chunks = (uint32_t)multiset_scan_chunks(items);
    const unsigned G = (unsigned)sets;
    for (unsigned pass = 0; pass < 8; pass++) {
        const unsigned shift = 8 * pass;
        hipLaunchKernelGGL(multiset_histogram_kernel, dim3(tiles, G), dim3(TILE_BLOCK), 0, st, keys, (uint32_t)items, shift, table, tiles);
        if (chunks > 1) hipLaunchKernelGGL(multiset_scan_sums_kernel, dim3(chunks, G), dim3(TILE_BLOCK), 0, st, table, words, sums);  // (chunk 0 reads no sum)
        hipLaunchKernelGGL(multiset_scan_apply_kernel, dim3(chunks, G), dim3(TILE_BLOCK), 0, st, table, words, sums);
        hipLaunchKernelGGL(multiset_scatter_kernel, dim3(tiles, G), dim3(TILE_BLOCK), 0, st, keys, idx, keys_alt, idx_alt, (uint32_t)items, shift, table, tiles);
        std::swap(keys, keys_alt);
        std::swap(idx, idx_alt);
    }
    return hipGetLastError();
}

hipError_t launch_multiset_sort(gl_t* keys, uint32_t* idx, gl_t* keys_alt, uint32_t* idx_alt, size_t items, uint32_t* table, uint32_t* sums, hipStream_t st) {
    return launch_multiset_sort_batch(keys, idx, keys_alt, idx_alt, items, 1, table, sums, st);
}

hipError_t launch_multiset_classify(const uint32_t* pair, const gl_t* cols, size_t stride, size_t n, const gl_t* keys, const uint32_t* idx,
                                    unsigned long long* masks, unsigned long long* counters, hipStream_t st) {
    hipLaunchKernelGGL(multiset_classify_kernel, dim3(nb(2 * n, TILE_BLOCK)), dim3(TILE_BLOCK), 0, st, pair, cols, stride, (uint32_t)n, keys, idx, masks, counters);
    return hipGetLastError();
}

hipError_t launch_multiset_count(const unsigned long long* masks, size_t n, unsigned long long* counters, hipStream_t st) {
    const uint32_t W = (uint32_t)((n + 63) / 64);
    hipLaunchKernelGGL(multiset_count_kernel, dim3(nb(2 * (size_t)W, TILE_BLOCK)), dim3(TILE_BLOCK), 0, st, masks, W, counters);
    return hipGetLastError();
}

}  // namespace starkhip
