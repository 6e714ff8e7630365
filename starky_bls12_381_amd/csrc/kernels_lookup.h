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

// Every launch serves a BATCH of lookups over the same n (grid.y = lookup): lookup y of the batch has its sorted items at keys / idx +
// y * 2 n, and flags + y * 2 n, sums + y * lookup_sum_words(2 n), slot + y * n, mask + y * (n + 63) / 64, missing[y].  A batch of one
// is one lookup with the buffers where they are.
//
// out [batch][4][n]: the first two columns of lookup y = columns desc[3 y + 1] (input) and desc[3 y + 2] (table) of the row-major
// trace [n][n_cols]
hipError_t launch_lookup_gather(const gl_t* trace, size_t n_cols, size_t n, const uint32_t* desc, size_t batch, gl_t* out, hipStream_t st);
// Over the 2 n sorted items of each lookup: flags = what each position is, sums = the counts of each tile, mask |= the input rows
// whose value no table row holds (zeroed by the caller), missing[y] += their number (zeroed by the caller).
hipError_t launch_lookup_mark(const gl_t* keys, const uint32_t* idx, size_t n, size_t batch, uint8_t* flags, uint32_t* sums, unsigned long long* mask,
                              unsigned long long* missing, hipStream_t st);
// sums [batch][3][tiles] <- their exclusive prefix sums, row by row
hipError_t launch_lookup_scan(uint32_t* sums, size_t n, size_t batch, hipStream_t st);
// The two placements, over the marked items and the scanned sums.  Element r of column c of the trace they write is
// out.base[c * col_stride + r * row_stride]; lookup y writes columns out_cols[2 y] (permuted_input) and out_cols[2 y + 1]
// (permuted_table); slot: [batch][n] uint32, every word 0xFFFFFFFF before the launch.
//   inputs: permuted_input[rank] = key, and permuted_table[rank] = key on a head; slot[non-head rank] = rank otherwise;
//   table:  permuted_table[slot[unused rank]] = key for every unused table item.
// gate (device, or null): lookup y is placed only when gate[y] == 0 -- its missing count, so that a lookup that fails leaves its
// columns as they were.  Null places every lookup: the columns of a failed one are then scratch (the prover's own copy of a trace).
struct LookupOut { gl_t* base; size_t col_stride, row_stride; };
hipError_t launch_lookup_place(const gl_t* keys, const uint8_t* flags, const uint32_t* sums, size_t n, size_t batch, const LookupOut& out, const uint32_t* out_cols,
                               const unsigned long long* gate, uint32_t* slot, hipStream_t st);

}  // namespace starkhip
