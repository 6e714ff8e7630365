// Launchers of kernels_logup.hip.  All launches are asynchronous on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gl.h"
#include "kernels_permutation.h"

namespace starkhip {

// words of launch_logup_polys's scratch (the spans' sums and their prefixes: the prefix sum is split like the Zs' prefix product), and
// of its results: the n_zs closing values, then the count of zero denominators
inline size_t logup_scratch_words(size_t n_rows, unsigned n_zs) { return perm_scratch_words(n_rows, n_zs); }
inline size_t logup_result_words(unsigned n_zs) { return (size_t)n_zs + 1; }

// The auxiliary polynomials of a trace (COMPAT.md L2): desc = logup_descriptor(P, by_slot, general) over `cols` (column c at cols + c * stride, n
// words each, any word of a cell's class), zpoly [n_zs] the Zs' polynomial indices (challenge-major), polys [n_polys][n], results
// [logup_result_words(n_zs)], scratch: logup_scratch_words(n, n_zs).  Four launches and one memset, none waits for another's workgroups.
hipError_t launch_logup_polys(const uint32_t* desc, bool general, const uint32_t* zpoly, const gl_t* cols, size_t stride, gl_t chi0, gl_t chi1, size_t n, unsigned n_zs,
                              gl_t* polys, gl_t* scratch, gl_t* results, hipStream_t st);
// The exclusive prefix sums alone: polys[zpoly[z]][r] <- the sum of its words before r, totals[z] <- the sum of all n, for n_zs
// polynomials of increments; scratch: logup_scratch_words(n, n_zs).  The three scan launches of launch_logup_polys.
hipError_t launch_logup_scan(const uint32_t* zpoly, size_t n, unsigned n_zs, gl_t* polys, gl_t* scratch, gl_t* totals, hipStream_t st);
// qvals [2][n << qdb] (the AIR's own fold / Z_H, natural quotient order) <- the fold over the AIR's and the LogUp constraints / Z_H;
// desc by trace column and of the same form (`general`: the kernels over Columns and Filters), alde [nA][N] the auxiliary LDE, scale_j = alpha_j^nL, the number of LogUp constraints
hipError_t launch_logup_quotient(const uint32_t* desc, bool general, const gl_t* lde, const gl_t* alde, gl_t chi0, gl_t chi1, const gl_t* tab, gl_t* qvals, gl_t alpha0,
                                 gl_t alpha1, gl_t scale0, gl_t scale1, unsigned log_n, unsigned rate_bits, unsigned qdb, hipStream_t st);

}  // namespace starkhip
