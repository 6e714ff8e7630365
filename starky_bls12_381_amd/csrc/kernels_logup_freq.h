// Launchers of kernels_logup_freq.hip: the frequencies columns of an AIR's LogUp lookups (logup_frequencies.h has the rule).  Every
// launch serves a BATCH of lookups over the same n rows; the tables of the batch are sorted once each by launch_multiset_sort_batch
// between the keys and the count.  All launches are asynchronous on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.h"
#include "gl.h"

namespace starkhip {

// Element r of column c of the trace the kernels read and write: base[c * col_stride + r * row_stride] -- a column-major trace
// (n, 1), a row-major one (1, n_cols), or the staged columns of a host trace (n, 1) with staged slots for column numbers.
struct LogupFreqTrace { gl_t* base; size_t col_stride, row_stride; };

// keys [slots][n], idx [slots][n]: slot y = column table_cols[y] reduced mod p, and the rows 0 .. n - 1
hipError_t launch_logup_freq_keys(const LogupFreqTrace& t, size_t n, const uint32_t* table_cols, size_t slots, gl_t* keys, uint32_t* idx, hipStream_t st);
// One lane per looked-up cell; cols: n_cols x {column, lookup of the batch, table slot of the batch}.  A cell whose value the sorted
// keys of its slot hold adds 1 to count[lookup][first position of the value]; any other sets bit r of mask[lookup][(n + 63) / 64] and
// adds 1 to missing[lookup] and to missing[lookups + its index in cols].  count, mask and missing are zeroed by the caller.
// combine: equal positions inside a wave are added as one (the result is the same either way).
hipError_t launch_logup_freq_count(const LogupFreqTrace& t, size_t n, const uint32_t* cols, size_t n_cols, size_t lookups, const gl_t* keys, uint32_t* count,
                                   unsigned long long* mask, uint32_t* missing, bool combine, hipStream_t st);
// The same two for lookups over Columns and Filters: desc holds COLUMNs and FILTERs in logup.h's descriptor words, over the trace's
// columns as `t` numbers them; offs [slots]: where slot y's table COLUMN starts; cols: n_cols x {where the value's COLUMN, followed by
// its FILTER, starts, lookup of the batch, table slot of the batch}.  A cell whose filter is 0 is skipped; one whose filter is neither
// 0 nor 1 counts as missing.  n is a power of two (the next row of the last is row 0).
hipError_t launch_logup_freq_keys_general(const LogupFreqTrace& t, size_t n, const uint32_t* desc, const uint32_t* offs, size_t slots, gl_t* keys, uint32_t* idx,
                                          hipStream_t st);
hipError_t launch_logup_freq_count_general(const LogupFreqTrace& t, size_t n, const uint32_t* desc, const uint32_t* cols, size_t n_cols, size_t lookups, const gl_t* keys,
                                           uint32_t* count, unsigned long long* mask, uint32_t* missing, bool combine, hipStream_t st);
// One lane per sorted table position of each lookup; lks: lookups x {table slot, frequencies column}: f[idx[pos]] = count[pos].
// gate (device, or null): lookup y is written only when gate[y] == 0 -- its missing count, so that a lookup that fails leaves its
// column as it was.  Null writes every lookup (the prover's own copy of a trace).
hipError_t launch_logup_freq_write(const LogupFreqTrace& t, size_t n, const uint32_t* lks, size_t lookups, const uint32_t* idx, const uint32_t* count,
                                   const uint32_t* gate, hipStream_t st);

}  // namespace starkhip
