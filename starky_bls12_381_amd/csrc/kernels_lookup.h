// Launchers of kernels_lookup.hip: the placement behind starkhip_lookup_columns (lookup_columns.h has the rule).  They run over the
// (key, idx) items of one lookup as launch_multiset_keys numbers them -- item i = side * n + row, side 0 the input column, side 1 the
// table column -- after launch_multiset_sort.  All launches are asynchronous on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.h"
#include "gl.h"

namespace starkhip {

// sorted positions one workgroup marks, counts and places: the tile of block_scan.h
static const unsigned LOOKUP_TILE = TILE_ITEMS;
inline size_t lookup_tiles(size_t items) { return tile_count(items); }
inline size_t lookup_sum_words(size_t items) { return 3 * lookup_tiles(items); }  // uint32 [3][tiles]: inputs, non-head inputs, unused table items

// out [2][n] = columns col_input and col_table of the row-major trace [n][n_cols]
hipError_t launch_lookup_gather(const gl_t* trace, size_t n_cols, size_t n, uint32_t col_input, uint32_t col_table, gl_t* out, hipStream_t st);
// Over the 2 n sorted items: flags [2 n] = what each position is, sums = the counts of each tile, mask [(n + 63) / 64] |= the input rows
// whose value no table row holds (zeroed by the caller), *missing += their number (zeroed by the caller).
hipError_t launch_lookup_mark(const gl_t* keys, const uint32_t* idx, size_t n, uint8_t* flags, uint32_t* sums, unsigned long long* mask,
                              unsigned long long* missing, hipStream_t st);
// sums [3][tiles] <- their exclusive prefix sums, row by row
hipError_t launch_lookup_scan(uint32_t* sums, size_t n, hipStream_t st);
// The two placements of a lookup that holds, over the marked items and the scanned sums.  Element r of an output column is
// permuted_*[r * stride]; slot: n uint32, every word 0xFFFFFFFF before the first launch.
//   inputs: permuted_input[rank] = key, and permuted_table[rank] = key on a head; slot[non-head rank] = rank otherwise;
//   table:  permuted_table[slot[unused rank]] = key for every unused table item.
hipError_t launch_lookup_place_inputs(const gl_t* keys, const uint8_t* flags, const uint32_t* sums, size_t n, gl_t* permuted_input, gl_t* permuted_table,
                                      size_t stride, uint32_t* slot, hipStream_t st);
hipError_t launch_lookup_place_table(const gl_t* keys, const uint8_t* flags, const uint32_t* sums, size_t n, gl_t* permuted_table, size_t stride,
                                     const uint32_t* slot, hipStream_t st);

}  // namespace starkhip
