// Launchers of kernels_multiset.hip: the multiset comparison behind starkhip_check_trace_permutations (permutation_check.h has the
// rule).  Host code reaches keys and sort through sorted_items_run (ctx.hip), which owns their buffers.  All launches are asynchronous on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.h"
#include "gl.h"

namespace starkhip {

// items one workgroup of the sort handles in a pass: the tile of block_scan.h
static const unsigned MULTISET_TILE = TILE_ITEMS;
// words of the digit table one workgroup of its scan handles
static const unsigned MULTISET_SCAN_CHUNK = 4096;
inline size_t multiset_tiles(size_t items) { return tile_count(items); }
inline size_t multiset_table_words(size_t items) { return 256 * multiset_tiles(items); }                                       // uint32 [256][tiles]
inline size_t multiset_scan_chunks(size_t items) { return (multiset_table_words(items) + MULTISET_SCAN_CHUNK - 1) / MULTISET_SCAN_CHUNK; }

// One pair of an AIR: `pair` on the device is n_entries followed by n_entries x (lhs, rhs) indices into `cols` (column c at
// cols + c * stride, n words each, any word of a cell's class).  Item i = side * n + row, 2 n items.
//   keys [2 n], idx [2 n]: key(i) = sum_t seed^t cell_t mod p, canonical, and i itself.
hipError_t launch_multiset_keys(const uint32_t* pair, const gl_t* cols, size_t stride, size_t n, gl_t seed, gl_t* keys, uint32_t* idx, hipStream_t st);
// Stable ascending sort of (key, idx) by key: eight passes of 8-bit digits between (keys, idx) and (keys_alt, idx_alt); the result is
// back in (keys, idx).  table: multiset_table_words(items) uint32, sums: multiset_scan_chunks(items) uint32.
hipError_t launch_multiset_sort(gl_t* keys, uint32_t* idx, gl_t* keys_alt, uint32_t* idx_alt, size_t items, uint32_t* table, uint32_t* sums, hipStream_t st);
// The same for `sets` sets of 2 n items each in one set of launches (grid.y = set): set y has its descriptor at pair + y * pair_stride,
// its items at keys / idx / keys_alt / idx_alt + y * items, its table at table + y * multiset_table_words(items) and its chunk sums at
// sums + y * multiset_scan_chunks(items).  One set is the launch above.
hipError_t launch_multiset_keys_batch(const uint32_t* pair, uint32_t pair_stride, size_t sets, const gl_t* cols, size_t stride, size_t n, gl_t seed, gl_t* keys,
                                      uint32_t* idx, hipStream_t st);
hipError_t launch_multiset_sort_batch(gl_t* keys, uint32_t* idx, gl_t* keys_alt, uint32_t* idx_alt, size_t items, size_t sets, uint32_t* table, uint32_t* sums,
                                      hipStream_t st);
// Over the sorted items: masks [2][(n + 63) / 64] |= the unmatched rows of each side (zeroed by the caller), counters[0] += the items
// whose key equals their predecessor's while their tuple does not (zeroed by the caller).
hipError_t launch_multiset_classify(const uint32_t* pair, const gl_t* cols, size_t stride, size_t n, const gl_t* keys, const uint32_t* idx,
                                    unsigned long long* masks, unsigned long long* counters, hipStream_t st);
// counters[1 + side] += the bits of masks[side]
hipError_t launch_multiset_count(const unsigned long long* masks, size_t n, unsigned long long* counters, hipStream_t st);

}  // namespace starkhip
