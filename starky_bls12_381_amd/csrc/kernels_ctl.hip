// Cross-table lookups on gfx950 (starky >= 0.2's CrossTableLookup; COMPAT.md C1 - C8, ctl.h has the conventions):
//
//  * ctl_terms_kernel: one lane per row, every endpoint of the table and both challenge pairs in one walk of the descriptor.  The named
//    columns are read column-major from the copy kept aside -- adjacent lanes, adjacent words --, the next row at (r + 1) & (n - 1), and
//    reduced mod p as every trace reader does.  Per (challenge, endpoint) the lane writes h = filter / c with c = gamma + sum_j beta^j
//    column_j, into the helper polynomial and, as the row's increment, where Z will be.  The inverse costs 127 multiplications (Fermat), so
//    the lane takes ONE per (row, challenge): Montgomery's product over the E denominators, a zero denominator standing in as 1, counted
//    for its endpoint, and inverted as 0.  The running product in front of each endpoint waits in the lane's own word of that endpoint's helper polynomial,
//    so the lane keeps no array; on the way back every endpoint is evaluated again (its descriptor words from cache) with its filter.
//  * the exclusive prefix sums over rows are the three scan launches of kernels_logup.hip (launch_logup_scan): no workgroup waits for
//    another, and a Z's total is the endpoint's sum S.
//  * ctl_quotient_kernel: one lane per point of the quotient's domain, the twin of logup_quotient_general_kernel:
//        q_j <- q_j alpha_j^(8 E) + (the fold over the 8 E CTL constraints with their masks) / Z_H
//    It reads the CTL polynomials' LDE at the point and at the next row's, the named columns of the trace LDE, and the sums.
// Every index is bounded by the row or point count the launch is given; columns and widths come from a validated system
// (air_validate.cpp) through ctl_descriptor.
#include <hip/hip_runtime.h>

#include "ctl.h"
#include "kernels.h"
#include "kernels_ctl.h"

namespace starkhip {

static const unsigned CTL_BLOCK = 256;  // one lane per row or point; the scan launches bring their own workgroup

// one endpoint at `w` on one row: its combined values under both challenge pairs; `w` is left at its filter
template <class Cell>
__device__ __forceinline__ void ctl_endpoint_values(const uint32_t*& w, const Cell& cell, const CtlChallenges& ch, gl_t* c0, gl_t* c1) {
    const uint32_t width = *w++;
    gl_t a0 = ch.gamma0, a1 = ch.gamma1, b0 = 1, b1 = 1;
    for (uint32_t j = 0; j < width; j++) {
        const gl_t v = logup_desc_column(w, cell);
        a0 = gl_add(a0, gl_mul(b0, v));
        a1 = gl_add(a1, gl_mul(b1, v));
        b0 = gl_mul(b0, ch.beta0);
        b1 = gl_mul(b1, ch.beta1);
    }
    *c0 = a0;
    *c1 = a1;
}

// polys[2 (i E + e)][r] <- h, polys[2 (i E + e) + 1][r] <- h (the row's increment of Z), for both challenges and every endpoint
__global__ __launch_bounds__(CTL_BLOCK) void ctl_terms_kernel(const uint32_t* __restrict__ desc, const gl_t* __restrict__ cols, size_t stride, CtlChallenges ch, size_t n,
                                                              gl_t* __restrict__ polys, unsigned long long* __restrict__ zero_count) { STARKHIP_PRIO_ENTRY
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const size_t rn = (r + 1) & (n - 1);
    auto cell = [&](uint32_t col, bool next) { return gl_from_u64(cols[col * stride + (next ? rn : r)]); };
    const uint32_t E = desc[0];
    gl_t* p0 = polys + r;                   // endpoint e: h at p0[2 e n], Z at p0[(2 e + 1) n] under the first pair, p1[...] under the second
    gl_t* p1 = p0 + (size_t)2 * E * n;
    gl_t run0 = 1, run1 = 1;
    for (uint32_t e = 0; e < E; e++) {  // forward: the running product in front of every endpoint
        const uint32_t* w = desc + desc[1 + e];
        gl_t c0, c1;
        ctl_endpoint_values(w, cell, ch, &c0, &c1);
        const uint32_t zeros = (c0 == 0) + (c1 == 0);
        if (zeros) atomicAdd(zero_count + e, (unsigned long long)zeros);  // per endpoint: the caller names the CTL (about n 2^-63 of the rows)
        p0[(size_t)2 * e * n] = run0;
        p1[(size_t)2 * e * n] = run1;
        run0 = gl_mul(run0, c0 == 0 ? 1 : c0);
        run1 = gl_mul(run1, c1 == 0 ? 1 : c1);
    }
    gl_t inv0 = gl_inv(run0), inv1 = gl_inv(run1);  // the one inversion per (row, challenge)
    for (uint32_t e = E; e-- > 0;) {  // back: endpoint after endpoint, with its filter
        const uint32_t* w = desc + desc[1 + e];
        gl_t c0, c1;
        ctl_endpoint_values(w, cell, ch, &c0, &c1);
        const gl_t phi = logup_desc_filter(w, cell);
        const gl_t h0 = c0 == 0 ? 0 : gl_mul(phi, gl_mul(inv0, p0[(size_t)2 * e * n]));
        const gl_t h1 = c1 == 0 ? 0 : gl_mul(phi, gl_mul(inv1, p1[(size_t)2 * e * n]));
        inv0 = gl_mul(inv0, c0 == 0 ? 1 : c0);
        inv1 = gl_mul(inv1, c1 == 0 ? 1 : c1);
        p0[(size_t)2 * e * n] = h0;
        p0[(size_t)(2 * e + 1) * n] = h0;
        p1[(size_t)2 * e * n] = h1;
        p1[(size_t)(2 * e + 1) * n] = h1;
    }
}

// desc: by trace column.  lde [C][N] and clde [4 E][N] coset-major; tab: quotient_tables_kernel's; qvals [2][size] in natural quotient order
__global__ __launch_bounds__(CTL_BLOCK) void ctl_quotient_kernel(const uint32_t* __restrict__ desc, const gl_t* __restrict__ lde, const gl_t* __restrict__ clde,
                                                                 CtlChallenges ch, const gl_t* __restrict__ sums, const gl_t* __restrict__ tab, gl_t* __restrict__ qvals,
                                                                 gl_t alpha0, gl_t alpha1, gl_t half0, gl_t half1, unsigned log_n, unsigned rate_bits, unsigned qdb) { STARKHIP_PRIO_ENTRY
    const size_t n = (size_t)1 << log_n, size = n << qdb, N = n << rate_bits;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= size) return;
    const size_t sp = t >> log_n, k = t & (n - 1), i = (k << qdb) + sp;
    const size_t at0 = ((sp << (rate_bits - qdb)) << log_n) + k, at1 = ((sp << (rate_bits - qdb)) << log_n) + ((k + 1) & (n - 1));  // the point, and the next row's
    auto cell = [&](uint32_t col, bool next) { return lde[(size_t)col * N + (next ? at1 : at0)]; };  // LDE words are canonical
    const gl_t m_tr = tab[t], l_first = tab[size + t], l_last = tab[2 * size + t], zh_inv = tab[3 * size + t];
    const uint32_t E = desc[0];
    // Every endpoint is walked once: its combined values under both challenge pairs and its filter.  The fold is challenge-major, so the
    // lane keeps one pair of accumulators per challenge -- acc[ci][j] folds challenge ci's 4 E constraints under alpha_j -- and joins
    // them at the end: fold = acc[0] alpha^(4 E) + acc[1], with half_j = alpha_j^(4 E).
    gl_t acc[2][2] = {{0, 0}, {0, 0}};
    for (uint32_t e = 0; e < E; e++) {
        const uint32_t* w = desc + desc[1 + e];
        gl_t c[2];
        ctl_endpoint_values(w, cell, ch, &c[0], &c[1]);
        const gl_t phi = logup_desc_filter(w, cell);
#pragma unroll
        for (uint32_t ci = 0; ci < 2; ci++) {
            const gl_t* a = clde + (size_t)2 * (ci * E + e) * N;
            const gl_t h = a[at0], z = a[N + at0], zn = a[N + at1];
            const gl_t k0 = gl_sub(gl_mul(h, c[ci]), phi);                                 // h c - filter
            const gl_t k1 = gl_mul(l_first, z);                                            // Z on the first row
            const gl_t k2 = gl_mul(m_tr, gl_sub(gl_sub(zn, z), h));                        // Z(next) - Z - h off the last row
            const gl_t k3 = gl_mul(l_last, gl_sub(gl_add(z, h), sums[ci * E + e]));        // Z + h - S on the last row
            acc[ci][0] = gl_add(gl_mul(gl_add(gl_mul(gl_add(gl_mul(gl_add(gl_mul(acc[ci][0], alpha0), k0), alpha0), k1), alpha0), k2), alpha0), k3);
            acc[ci][1] = gl_add(gl_mul(gl_add(gl_mul(gl_add(gl_mul(gl_add(gl_mul(acc[ci][1], alpha1), k0), alpha1), k1), alpha1), k2), alpha1), k3);
        }
    }
    const gl_t f0 = gl_add(gl_mul(acc[0][0], half0), acc[1][0]), f1 = gl_add(gl_mul(acc[0][1], half1), acc[1][1]);
    qvals[i] = gl_add(gl_mul(qvals[i], gl_mul(half0, half0)), gl_mul(f0, zh_inv));
    qvals[size + i] = gl_add(gl_mul(qvals[size + i], gl_mul(half1, half1)), gl_mul(f1, zh_inv));
}

hipError_t launch_ctl_polys(const uint32_t* desc, const uint32_t* zpoly, const gl_t* cols, size_t stride, CtlChallenges ch, size_t n, unsigned n_endpoints, gl_t* polys,
                            unsigned first_poly, gl_t* scratch, gl_t* results, hipStream_t st) {
    if (!n_endpoints) return hipSuccess;
    unsigned long long* zero_count = (unsigned long long*)(results + 2 * n_endpoints);  // [E]
    if (hipError_t e = hipMemsetAsync(zero_count, 0, 8 * (size_t)n_endpoints, st); e != hipSuccess) return e;
    hipLaunchKernelGGL(ctl_terms_kernel, dim3(nb(n, CTL_BLOCK)), dim3(CTL_BLOCK), 0, st, desc, cols, stride, ch, n, polys + (size_t)first_poly * n, zero_count);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return launch_logup_scan(zpoly, n, 2 * n_endpoints, polys, scratch, results, st);
}

hipError_t launch_ctl_quotient(const uint32_t* desc, const gl_t* lde, const gl_t* clde, CtlChallenges ch, const gl_t* sums, const gl_t* tab, gl_t* qvals, gl_t alpha0,
                               gl_t alpha1, gl_t half0, gl_t half1, unsigned log_n, unsigned rate_bits, unsigned qdb, hipStream_t st) {
    const size_t size = (size_t)1 << (log_n + qdb);
    hipLaunchKernelGGL(ctl_quotient_kernel, dim3(nb(size, CTL_BLOCK)), dim3(CTL_BLOCK), 0, st, desc, lde, clde, ch, sums, tab, qvals, alpha0, alpha1, half0, half1, log_n,
                       rate_bits, qdb);
    return hipGetLastError();
}

}  // namespace starkhip
