// The permuted columns of a lookup on gfx950 (starkhip_lookup_columns; lookup_columns.h has the rule, DESIGN.md 13b the arguments).
// The items of one lookup -- the n cells of its input column, then the n cells of its table column -- come sorted by
// launch_multiset_keys and launch_multiset_sort (kernels_multiset.hip): ascending by cell, and inside a run of equal cells the input
// items, rows ascending, before the table items, because that sort is stable.  Over the 2 n sorted positions:
//
//  * lookup_mark_kernel: one lane per position.  An INPUT item (idx < n) is a HEAD when it starts its run; a table item is USED when
//    its predecessor is an input item of its run -- the first table item of a run that has inputs; an input item is MISSING when the
//    last item of its run, found by binary search for the run's end (sorted_run_end), is an input item too: the run holds no table
//    item.  The flags kept per position are the three things the placement counts -- input, non-head input, unused table item -- and
//    each workgroup leaves the totals of its tile of LOOKUP_TILE positions (the sort's tile: block_scan.h) in sums[count][tile].
//    Missing rows go into the mask through 64-bit atomicOr and into one counter: both independent of the order of arrival.
//  * lookup_scan_kernel: the exclusive prefix sums of the three rows of tile totals, one workgroup per row walking its row in pieces
//    of TILE_BLOCK with a carry: any number of tiles.
//  * lookup_place_inputs_kernel, lookup_place_table_kernel: a position's rank among the inputs, the non-head inputs or the unused
//    table items = the scanned total of the tiles before its own + the counts of the earlier slots of its tile (LDS) + the lower
//    lanes of its slot (a __ballot and a popcount).  The inputs in sorted order ARE permuted_input, so an input item writes its key
//    at its rank; a head writes permuted_table there too; the k-th non-head leaves its rank in slot[k], and in the second launch
//    the k-th unused table item writes its key to permuted_table[slot[k]].
// No workgroup waits for another inside a launch and no global atomic decides where anything lands: every destination is a function
// of the sorted order alone, so the columns are the same bytes on every run.  Every index is bounded by the item count the launch
// is given.
//
// Every launch has a batch dimension: grid.y = a lookup of the batch, whose buffers lie strided by lookup -- its sorted items at keys /
// idx + y * 2 n (the sort's own stride), flags + y * 2 n, sums + y * 3 tiles, slot + y * n, its mask at mask + y * (n + 63) / 64 and
// its missing count at missing[y].  Nothing of one lookup reads or writes anything of another, so what holds for one launch holds
// for the batch; a batch of one is the launch it was.  The placements find their two output columns in out_cols[y] and, given a
// gate, leave a lookup alone whose gate[y] is not zero: its missing count, so a failed lookup keeps its columns.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "kernels.h"
#include "kernels_lookup.h"

namespace starkhip {

enum : uint32_t { LK_INPUT = 1, LK_NONHEAD = 2, LK_UNUSED = 4 };  // the flags of a position: bit c = it counts towards sums[c]

struct LkCounts { uint32_t c[3]; };

// The flags f[r] of this lane's TILE_ROUNDS positions -- position base + slot * 64 + lane with slot = tile_slot(r, wave), 0 for a
// position past the items -- give before[r] = how many positions of the tile BEFORE that one carry each flag, and the tile's totals.
// cnt: [3][TILE_SLOTS] words of LDS.  Every lane of the workgroup calls it.
__device__ __forceinline__ void lk_tile_ranks(const uint32_t f[TILE_ROUNDS], uint32_t (*cnt)[TILE_SLOTS], LkCounts before[TILE_ROUNDS], LkCounts* total) {
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned long long lower = (1ull << lane) - 1;
#pragma unroll
    for (unsigned r = 0; r < TILE_ROUNDS; r++) {
        const unsigned slot = tile_slot(r, w);
#pragma unroll
        for (unsigned c = 0; c < 3; c++) {
            const unsigned long long m = __ballot((f[r] >> c) & 1u);
            before[r].c[c] = (uint32_t)__popcll(m & lower);
            if (lane == 0) cnt[c][slot] = (uint32_t)__popcll(m);
        }
    }
    __syncthreads();
#pragma unroll
    for (unsigned c = 0; c < 3; c++) {
        uint32_t run = 0;
#pragma unroll
        for (unsigned s = 0; s < TILE_SLOTS; s++) {
            const uint32_t v = cnt[c][s];
#pragma unroll
            for (unsigned r = 0; r < TILE_ROUNDS; r++)
                if (s < tile_slot(r, w)) before[r].c[c] += v;
            run += v;
        }
        total->c[c] = run;
    }
}

// desc: per lookup of the batch {1, input, table}; out: [batch][4][n], of which this fills the first two columns
__global__ __launch_bounds__(TILE_BLOCK) void lookup_gather_kernel(const gl_t* __restrict__ trace, size_t n_cols, uint32_t n, const uint32_t* __restrict__ desc,
                                                                   gl_t* __restrict__ out) { STARKHIP_PRIO_ENTRY
    const uint32_t i = blockIdx.x * TILE_BLOCK + threadIdx.x;
    if (i >= 2 * n) return;
    const uint32_t side = i >= n, row = i - side * n;
    out[(size_t)blockIdx.y * 4 * n + i] = trace[(size_t)row * n_cols + desc[3 * blockIdx.y + 1 + side]];
}

// grid: tiles x lookups
__global__ __launch_bounds__(TILE_BLOCK) void lookup_mark_kernel(const gl_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint32_t n, uint8_t* __restrict__ flags,
                                                                 uint32_t* __restrict__ sums, uint32_t tiles, unsigned long long* __restrict__ mask,
                                                                 unsigned long long* __restrict__ missing) { STARKHIP_PRIO_ENTRY
    __shared__ uint32_t cnt[3][TILE_SLOTS];
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t items = 2 * n, base = blockIdx.x * LOOKUP_TILE;
    keys += (size_t)blockIdx.y * items;
    idx += (size_t)blockIdx.y * items;
    flags += (size_t)blockIdx.y * items;
    sums += (size_t)blockIdx.y * 3 * tiles;
    mask += (size_t)blockIdx.y * ((n + 63) / 64);
    missing += blockIdx.y;
    uint32_t f[TILE_ROUNDS];
#pragma unroll
    for (unsigned r = 0; r < TILE_ROUNDS; r++) {
        const uint32_t j = base + tile_slot(r, w) * 64 + lane;
        f[r] = 0;
        bool miss = false;
        uint32_t row = 0;
        if (j < items) {
            const gl_t k = keys[j];
            const uint32_t id = idx[j];
            const bool input = id < n, same = j > 0 && keys[j - 1] == k;  // continues the run of its predecessor
            if (input) {
                f[r] = same ? LK_INPUT | LK_NONHEAD : LK_INPUT;
                miss = idx[sorted_run_end(keys, k, j, items) - 1] < n;  // the run's last item is an input item: inputs come first, so it holds no table item
                row = id;
            } else if (!(same && idx[j - 1] < n)) f[r] = LK_UNUSED;
            flags[j] = (uint8_t)f[r];
        }
        if (miss) atomicOr(&mask[row >> 6], 1ull << (row & 63u));
        const unsigned long long hit = __ballot(miss);
        if (lane == 0 && hit) atomicAdd(missing, (unsigned long long)__popcll(hit));  // a count: the order of the adds does not matter
    }
    LkCounts before[TILE_ROUNDS], total;
    lk_tile_ranks(f, cnt, before, &total);
    if (threadIdx.x < 3) sums[(size_t)threadIdx.x * tiles + blockIdx.x] = threadIdx.x == 0 ? total.c[0] : threadIdx.x == 1 ? total.c[1] : total.c[2];
}

// grid: 3 x lookups, one workgroup per row of sums
__global__ __launch_bounds__(TILE_BLOCK) void lookup_scan_kernel(uint32_t* __restrict__ sums, uint32_t tiles) { STARKHIP_PRIO_ENTRY
    __shared__ uint32_t lds[TILE_WAVES];
    uint32_t* row = sums + ((size_t)blockIdx.y * 3 + blockIdx.x) * tiles;
    uint32_t carry = 0;
    for (uint32_t at = 0; at < tiles; at += TILE_BLOCK) {  // the same trip count on every lane
        const uint32_t j = at + threadIdx.x;
        const uint32_t v = j < tiles ? row[j] : 0u;
        uint32_t total;
        const uint32_t excl = block_scan(v, ScanAdd(), 0u, lds, &total);
        if (j < tiles) row[j] = carry + excl;
        carry += total;
    }
}

// Where the placements write: element r of column c is base[c * col_stride + r * row_stride]
struct LkOut { gl_t* base; size_t col_stride, row_stride; };

// sums: scanned.  out_cols: per lookup {permuted_input, permuted_table}.  grid: tiles x lookups
__global__ __launch_bounds__(TILE_BLOCK) void lookup_place_inputs_kernel(const gl_t* __restrict__ keys, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ sums,
                                                                         uint32_t tiles, uint32_t n, LkOut out, const uint32_t* __restrict__ out_cols,
                                                                         const unsigned long long* __restrict__ gate, uint32_t* __restrict__ slot) { STARKHIP_PRIO_ENTRY
    __shared__ uint32_t cnt[3][TILE_SLOTS];
    if (gate && gate[blockIdx.y]) return;  // the same for every lane of the workgroup
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t items = 2 * n, base = blockIdx.x * LOOKUP_TILE;
    keys += (size_t)blockIdx.y * items;
    flags += (size_t)blockIdx.y * items;
    sums += (size_t)blockIdx.y * 3 * tiles;
    slot += (size_t)blockIdx.y * n;
    const size_t stride = out.row_stride;
    gl_t* permuted_input = out.base + out_cols[2 * blockIdx.y] * out.col_stride;
    gl_t* permuted_table = out.base + out_cols[2 * blockIdx.y + 1] * out.col_stride;
    uint32_t f[TILE_ROUNDS];
#pragma unroll
    for (unsigned r = 0; r < TILE_ROUNDS; r++) {
        const uint32_t j = base + tile_slot(r, w) * 64 + lane;
        f[r] = j < items ? flags[j] : 0u;
    }
    LkCounts before[TILE_ROUNDS], total;
    lk_tile_ranks(f, cnt, before, &total);
    const uint32_t inputs0 = sums[blockIdx.x], nonheads0 = sums[(size_t)tiles + blockIdx.x];
#pragma unroll
    for (unsigned r = 0; r < TILE_ROUNDS; r++) {
        const uint32_t j = base + tile_slot(r, w) * 64 + lane;
        if (!(f[r] & LK_INPUT)) continue;  // (a position past the items has no flag)
        const uint32_t rank = inputs0 + before[r].c[0];
        if (rank >= n) continue;
        const gl_t k = keys[j];
        permuted_input[(size_t)rank * stride] = k;
        if (!(f[r] & LK_NONHEAD)) permuted_table[(size_t)rank * stride] = k;
        else {
            const uint32_t nh = nonheads0 + before[r].c[1];
            if (nh < n) slot[nh] = rank;
        }
    }
}

// sums: scanned; slot: as lookup_place_inputs_kernel left it.  grid: tiles x lookups
__global__ __launch_bounds__(TILE_BLOCK) void lookup_place_table_kernel(const gl_t* __restrict__ keys, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ sums,
                                                                        uint32_t tiles, uint32_t n, LkOut out, const uint32_t* __restrict__ out_cols,
                                                                        const unsigned long long* __restrict__ gate, const uint32_t* __restrict__ slot) { STARKHIP_PRIO_ENTRY
    __shared__ uint32_t cnt[3][TILE_SLOTS];
    if (gate && gate[blockIdx.y]) return;  // the same for every lane of the workgroup
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t items = 2 * n, base = blockIdx.x * LOOKUP_TILE;
    keys += (size_t)blockIdx.y * items;
    flags += (size_t)blockIdx.y * items;
    sums += (size_t)blockIdx.y * 3 * tiles;
    slot += (size_t)blockIdx.y * n;
    const size_t stride = out.row_stride;
    gl_t* permuted_table = out.base + out_cols[2 * blockIdx.y + 1] * out.col_stride;
    uint32_t f[TILE_ROUNDS];
#pragma unroll
    for (unsigned r = 0; r < TILE_ROUNDS; r++) {
        const uint32_t j = base + tile_slot(r, w) * 64 + lane;
        f[r] = j < items ? flags[j] : 0u;
    }
    LkCounts before[TILE_ROUNDS], total;
    lk_tile_ranks(f, cnt, before, &total);
    const uint32_t unused0 = sums[2 * (size_t)tiles + blockIdx.x];
#pragma unroll
    for (unsigned r = 0; r < TILE_ROUNDS; r++) {
        const uint32_t j = base + tile_slot(r, w) * 64 + lane;
        if (!(f[r] & LK_UNUSED)) continue;
        const uint32_t un = unused0 + before[r].c[2];
        if (un >= n) continue;
        const uint32_t dst = slot[un];  // 0xFFFFFFFF where no non-head left its rank
        if (dst < n) permuted_table[(size_t)dst * stride] = keys[j];
    }
}

hipError_t launch_lookup_gather(const gl_t* trace, size_t n_cols, size_t n, const uint32_t* desc, size_t batch, gl_t* out, hipStream_t st) {
    hipLaunchKernelGGL(lookup_gather_kernel, dim3(nb(2 * n, TILE_BLOCK), (unsigned)batch), dim3(TILE_BLOCK), 0, st, trace, n_cols, (uint32_t)n, desc, out);
    return hipGetLastError();
}

hipError_t launch_lookup_mark(const gl_t* keys, const uint32_t* idx, size_t n, size_t batch, uint8_t* flags, uint32_t* sums, unsigned long long* mask,
                              unsigned long long* missing, hipStream_t st) {
    const uint32_t tiles = (uint32_t)lookup_tiles(2 * n);
    hipLaunchKernelGGL(lookup_mark_kernel, dim3(tiles, (unsigned)batch), dim3(TILE_BLOCK), 0, st, keys, idx, (uint32_t)n, flags, sums, tiles, mask, missing);
    return hipGetLastError();
}

hipError_t launch_lookup_scan(uint32_t* sums, size_t n, size_t batch, hipStream_t st) {
    hipLaunchKernelGGL(lookup_scan_kernel, dim3(3, (unsigned)batch), dim3(TILE_BLOCK), 0, st, sums, (uint32_t)lookup_tiles(2 * n));
    return hipGetLastError();
}

hipError_t launch_lookup_place(const gl_t* keys, const uint8_t* flags, const uint32_t* sums, size_t n, size_t batch, const LookupOut& out, const uint32_t* out_cols,
                               const unsigned long long* gate, uint32_t* slot, hipStream_t st) {
    const uint32_t tiles = (uint32_t)lookup_tiles(2 * n);
    const LkOut o = {out.base, out.col_stride, out.row_stride};
    hipLaunchKernelGGL(lookup_place_inputs_kernel, dim3(tiles, (unsigned)batch), dim3(TILE_BLOCK), 0, st, keys, flags, sums, tiles, (uint32_t)n, o, out_cols, gate, slot);
    hipLaunchKernelGGL(lookup_place_table_kernel, dim3(tiles, (unsigned)batch), dim3(TILE_BLOCK), 0, st, keys, flags, sums, tiles, (uint32_t)n, o, out_cols, gate,
                       (const uint32_t*)slot);
    return hipGetLastError();
}

}  // namespace starkhip
