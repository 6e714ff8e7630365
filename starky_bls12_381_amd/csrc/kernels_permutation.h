// Launchers of kernels_permutation.hip.  All launches are asynchronous on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gl.h"

namespace starkhip {

// rows one workgroup scans: the prefix product of a Z is split into spans of this many rows
static const unsigned PERM_SPAN_ROWS = 1024;
inline size_t perm_span_count(size_t n_rows) { return (n_rows + PERM_SPAN_ROWS - 1) / PERM_SPAN_ROWS; }
// words of launch_perm_zs's scratch: the spans' products and their prefixes
inline size_t perm_scratch_words(size_t n_rows, unsigned n_zs) { return 2 * (size_t)n_zs * perm_span_count(n_rows); }

// The Z polynomials of a trace: desc = perm_descriptor(P, by_slot) over `cols` (column c at cols + c * stride, n words each, any word of
// a cell's class), chal [n_zs / 2][2]{beta, gamma}; zs [n_zs][n] (Z[0] = 1, exclusive prefix products of the rows' ratios), closing
// [n_zs] (the product of all n ratios), scratch: perm_scratch_words(n, n_zs).  Four launches, none waits for another's workgroups.
hipError_t launch_perm_zs(const uint32_t* desc, const gl_t* cols, size_t stride, const gl_t* chal, size_t n, unsigned n_zs, gl_t* zs, gl_t* scratch,
                          gl_t* closing, hipStream_t st);
// qvals [2][n << qdb] (the AIR's own fold / Z_H, natural quotient order) <- the fold over the AIR's and the permutation constraints / Z_H;
// desc by trace column, scale_j = alpha_j^(2 n_zs), the number of permutation constraints
hipError_t launch_perm_quotient(const uint32_t* desc, const gl_t* lde, const gl_t* zlde, const gl_t* chal, const gl_t* tab, gl_t* qvals, gl_t alpha0,
                                gl_t alpha1, gl_t scale0, gl_t scale1, unsigned log_n, unsigned rate_bits, unsigned qdb, hipStream_t st);

}  // namespace starkhip
