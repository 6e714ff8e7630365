// Launchers of kernels_ctl.hip: the cross-table lookups of one table of a system (ctl.h).  All launches are asynchronous on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gl.h"
#include "kernels_logup.h"

namespace starkhip {

struct CtlChallenges { gl_t beta0, gamma0, beta1, gamma1; };

// words of launch_ctl_polys's scratch (the scan's, for the 2 E running sums) and of its results: the 2 E sums, then per endpoint the
// count of its zero denominators (both challenges together)
inline size_t ctl_scratch_words(size_t n_rows, unsigned n_endpoints) { return logup_scratch_words(n_rows, 2 * n_endpoints); }
inline size_t ctl_result_words(unsigned n_endpoints) { return 3 * (size_t)n_endpoints; }

// The 4 E polynomials of a trace (COMPAT.md C3): desc = ctl_descriptor(T, true, slot_base) over `cols` (column c at cols + c * stride, n words
// each, any word of a cell's class), zpoly [2 E] the Zs' polynomial indices counted from `polys`, which is where the table's middle matrix
// starts; the CTL polynomials are written from polys + first_poly * n on.  results [ctl_result_words(E)], scratch: ctl_scratch_words(n, E).
// One terms launch, one memset and the three scan launches of kernels_logup.hip; none waits for another's workgroups.
hipError_t launch_ctl_polys(const uint32_t* desc, const uint32_t* zpoly, const gl_t* cols, size_t stride, CtlChallenges ch, size_t n, unsigned n_endpoints,
                            gl_t* polys, unsigned first_poly, gl_t* scratch, gl_t* results, hipStream_t st);
// qvals [2][n << qdb] (the fold over the AIR's own and the LogUp constraints / Z_H, natural quotient order) <- that fold times alpha_j^(8 E)
// plus the fold over the CTL constraints / Z_H.  desc by trace column, clde [4 E][N] the CTL part of the middle matrix's LDE, sums [2 E] on
// the device, half_j = alpha_j^(4 E) (one challenge's share of the fold; every endpoint is walked once for both challenges).
hipError_t launch_ctl_quotient(const uint32_t* desc, const gl_t* lde, const gl_t* clde, CtlChallenges ch, const gl_t* sums, const gl_t* tab, gl_t* qvals, gl_t alpha0,
                               gl_t alpha1, gl_t half0, gl_t half1, unsigned log_n, unsigned rate_bits, unsigned qdb, hipStream_t st);

}  // namespace starkhip
