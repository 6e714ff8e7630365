// LogUp lookups on gfx950 (starky >= 0.2's Lookup; COMPAT.md L1 - L7, logup.h has the conventions):
//
//  * logup_terms_kernel: one lane per row, both challenges in one walk of the descriptor.  The named columns are read column-major --
//    adjacent lanes, adjacent words -- and reduced mod p as every trace reader does.  Per (challenge, lookup) the lane writes the helper
//    values h_j = sum over batch j of 1 / (chi + c) and, where Z will be, the row's increment sum_j h_j - f / (chi + t); a zero
//    denominator has inverse 0 and is counted.  The inverse costs 127 multiplications (Fermat), so the lane takes ONE per (row,
//    challenge, lookup): Montgomery's product over the lookup's m + 1 denominators, with a zero denominator standing in as 1.  The
//    running products before each batch wait in the lane's own words of the output (h_j's, and Z's for the table's), so the lane keeps
//    no array; on the way back every batch is read again (from cache) for its product D_j and S_j = sum_c prod_{c' != c} (chi + c'),
//    and h_j = S_j / D_j.  (m + 1 separate inversions gave the same words and a slower kernel: profiles/logup.json.)
//  * the exclusive prefix sum over rows, per Z, n = 2 .. 2^20, as the three launches of the Zs' prefix product (kernels_permutation.hip):
//    the sum of each span of PERM_SPAN_ROWS rows, one workgroup per Z scanning those, which leaves the closing value, and the scan of each span
//    from its prefix.  block_scan under gl_add.  No workgroup waits for another inside a launch; field addition is exact and
//    associative and every sum canonical, so the words do not depend on the split.
//  * logup_quotient_kernel: one lane per point of the quotient's domain, the twin of perm_quotient_kernel:
//        q_j <- q_j alpha_j^nL + (sum of the nL LogUp constraints with their masks and alpha powers) / Z_H
//    It reads the auxiliary LDE at the point and at the next row's point, and the named columns of the trace LDE.
//  * logup_terms_general_kernel / logup_quotient_general_kernel: the same two for lookups over Columns and Filters (logup.h).  A
//    value is constant + sum coefficient * cell over the row and the next one -- row (r + 1) & (n - 1), the neighbouring lane's word of the
//    same column -- and is evaluated from the descriptor each time it is needed: once forward for the running products, once on the
//    way back with its filter, where S_j = sum_c phi_c prod_{c' != c} (chi + v_c').  The one inversion per (row, challenge, lookup), the
//    stand-ins for zero denominators and the three scan launches are the plain kernels'.  A program of plain lookups never runs them
//    (logup_use_general), so its words and its speed are what they were.
// Every index is bounded by the row or point count the launch is given; the columns and polynomial indices come from a validated
// program (air_validate.cpp) through logup_descriptor.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "kernels.h"
#include "kernels_logup.h"
#include "logup.h"

namespace starkhip {

static const unsigned LOGUP_BLOCK = TILE_BLOCK, LOGUP_ITEMS = PERM_SPAN_ROWS / LOGUP_BLOCK;  // block_scan's workgroup
struct ScanGlAdd { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return gl_add(a, b); } };

// polys[(i half + base + j)][r] <- h_j, polys[(i half + base + H)][r] <- the row's increment, for both challenges and every lookup
__global__ __launch_bounds__(LOGUP_BLOCK) void logup_terms_kernel(const uint32_t* __restrict__ desc, const gl_t* __restrict__ cols, size_t stride, gl_t chi0,
                                                                  gl_t chi1, size_t n, gl_t* __restrict__ polys, unsigned long long* __restrict__ zero_count) { STARKHIP_PRIO_ENTRY
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t nl = desc[0], B = desc[1], half = desc[2];
    uint32_t at = LOGUP_DESC_HEAD, zeros = 0;
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t base = desc[at], m = desc[at + 1], H = (m + B - 1) / B;
        const gl_t tv = gl_from_u64(cols[desc[at + 2] * stride + r]), fv = gl_from_u64(cols[desc[at + 3] * stride + r]);
        const uint32_t* cs = desc + at + LOGUP_DESC_LOOKUP;
        at += LOGUP_DESC_LOOKUP + m;
        gl_t* p0 = polys + (size_t)base * n + r;  // polynomial j of the lookup at p0[j n] under chi_0, p1[j n] under chi_1
        gl_t* p1 = p0 + (size_t)half * n;
        const gl_t xt0 = gl_add(chi0, tv), xt1 = gl_add(chi1, tv);
        zeros += (xt0 == 0) + (xt1 == 0);
        // forward: the running product in front of every batch, then in front of the table's denominator
        gl_t run0 = 1, run1 = 1;
        for (uint32_t j = 0; j < H; j++) {
            const uint32_t c1 = (j + 1) * B < m ? (j + 1) * B : m;
            p0[(size_t)j * n] = run0;
            p1[(size_t)j * n] = run1;
            for (uint32_t c = j * B; c < c1; c++) {
                const gl_t v = gl_from_u64(cols[cs[c] * stride + r]), x0 = gl_add(chi0, v), x1 = gl_add(chi1, v);
                zeros += (x0 == 0) + (x1 == 0);
                run0 = gl_mul(run0, x0 == 0 ? 1 : x0);
                run1 = gl_mul(run1, x1 == 0 ? 1 : x1);
            }
        }
        const gl_t nt0 = xt0 == 0 ? 1 : xt0, nt1 = xt1 == 0 ? 1 : xt1;
        gl_t inv0 = gl_inv(gl_mul(run0, nt0)), inv1 = gl_inv(gl_mul(run1, nt1));  // the one inversion per (row, challenge, lookup)
        // back: the table's term, then batch after batch
        gl_t inc0 = gl_neg(gl_mul(fv, xt0 == 0 ? 0 : gl_mul(inv0, run0))), inc1 = gl_neg(gl_mul(fv, xt1 == 0 ? 0 : gl_mul(inv1, run1)));
        inv0 = gl_mul(inv0, nt0);
        inv1 = gl_mul(inv1, nt1);
        for (uint32_t j = H; j-- > 0;) {
            const uint32_t c1 = (j + 1) * B < m ? (j + 1) * B : m;
            gl_t D0 = 1, S0 = 0, D1 = 1, S1 = 0;
            for (uint32_t c = j * B; c < c1; c++) {
                const gl_t v = gl_from_u64(cols[cs[c] * stride + r]), x0 = gl_add(chi0, v), x1 = gl_add(chi1, v);
                S0 = gl_add(gl_mul(S0, x0 == 0 ? 1 : x0), x0 == 0 ? 0 : D0);
                D0 = gl_mul(D0, x0 == 0 ? 1 : x0);
                S1 = gl_add(gl_mul(S1, x1 == 0 ? 1 : x1), x1 == 0 ? 0 : D1);
                D1 = gl_mul(D1, x1 == 0 ? 1 : x1);
            }
            const gl_t h0 = gl_mul(gl_mul(inv0, p0[(size_t)j * n]), S0), h1 = gl_mul(gl_mul(inv1, p1[(size_t)j * n]), S1);
            inv0 = gl_mul(inv0, D0);
            inv1 = gl_mul(inv1, D1);
            p0[(size_t)j * n] = h0;
            p1[(size_t)j * n] = h1;
            inc0 = gl_add(inc0, h0);
            inc1 = gl_add(inc1, h1);
        }
        p0[(size_t)H * n] = inc0;
        p1[(size_t)H * n] = inc1;
    }
    if (zeros) atomicAdd(zero_count, (unsigned long long)zeros);
}

// the same for the general descriptor: values and filters evaluated from their Columns, on the row and the next one
__global__ __launch_bounds__(LOGUP_BLOCK) void logup_terms_general_kernel(const uint32_t* __restrict__ desc, const gl_t* __restrict__ cols, size_t stride, gl_t chi0,
                                                                          gl_t chi1, size_t n, gl_t* __restrict__ polys, unsigned long long* __restrict__ zero_count) { STARKHIP_PRIO_ENTRY
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const size_t rn = (r + 1) & (n - 1);
    auto cell = [&](uint32_t col, bool next) { return gl_from_u64(cols[col * stride + (next ? rn : r)]); };
    const uint32_t nl = desc[0], B = desc[1], half = desc[2];
    uint32_t at = LOGUP_DESC_HEAD, zeros = 0;
    for (uint32_t l = 0; l < nl; l++) {
        const uint32_t base = desc[at], m = desc[at + 1], H = (m + B - 1) / B;
        const uint32_t* starts = desc + at + LOGUP_DESC_LOOKUP_GENERAL;  // where each batch's first value starts
        const uint32_t* w = starts + H;
        at = desc[at + 2];
        const gl_t tv = logup_desc_column(w, cell), fv = logup_desc_column(w, cell);
        gl_t* p0 = polys + (size_t)base * n + r;
        gl_t* p1 = p0 + (size_t)half * n;
        const gl_t xt0 = gl_add(chi0, tv), xt1 = gl_add(chi1, tv);
        zeros += (xt0 == 0) + (xt1 == 0);
        gl_t run0 = 1, run1 = 1;
        for (uint32_t j = 0; j < H; j++) {
            const uint32_t c1 = (j + 1) * B < m ? (j + 1) * B : m;
            p0[(size_t)j * n] = run0;
            p1[(size_t)j * n] = run1;
            for (uint32_t c = j * B; c < c1; c++) {
                const gl_t v = logup_desc_column(w, cell), x0 = gl_add(chi0, v), x1 = gl_add(chi1, v);
                logup_desc_skip_filter(w);
                zeros += (x0 == 0) + (x1 == 0);
                run0 = gl_mul(run0, x0 == 0 ? 1 : x0);
                run1 = gl_mul(run1, x1 == 0 ? 1 : x1);
            }
        }
        const gl_t nt0 = xt0 == 0 ? 1 : xt0, nt1 = xt1 == 0 ? 1 : xt1;
        gl_t inv0 = gl_inv(gl_mul(run0, nt0)), inv1 = gl_inv(gl_mul(run1, nt1));  // the one inversion per (row, challenge, lookup)
        gl_t inc0 = gl_neg(gl_mul(fv, xt0 == 0 ? 0 : gl_mul(inv0, run0))), inc1 = gl_neg(gl_mul(fv, xt1 == 0 ? 0 : gl_mul(inv1, run1)));
        inv0 = gl_mul(inv0, nt0);
        inv1 = gl_mul(inv1, nt1);
        for (uint32_t j = H; j-- > 0;) {
            const uint32_t c1 = (j + 1) * B < m ? (j + 1) * B : m;
            gl_t D0 = 1, S0 = 0, D1 = 1, S1 = 0;
            w = desc + starts[j];
            for (uint32_t c = j * B; c < c1; c++) {
                const gl_t v = logup_desc_column(w, cell), x0 = gl_add(chi0, v), x1 = gl_add(chi1, v);
                const gl_t phi = logup_desc_filter(w, cell);
                S0 = gl_add(gl_mul(S0, x0 == 0 ? 1 : x0), x0 == 0 ? 0 : gl_mul(phi, D0));
                D0 = gl_mul(D0, x0 == 0 ? 1 : x0);
                S1 = gl_add(gl_mul(S1, x1 == 0 ? 1 : x1), x1 == 0 ? 0 : gl_mul(phi, D1));
                D1 = gl_mul(D1, x1 == 0 ? 1 : x1);
            }
            const gl_t h0 = gl_mul(gl_mul(inv0, p0[(size_t)j * n]), S0), h1 = gl_mul(gl_mul(inv1, p1[(size_t)j * n]), S1);
            inv0 = gl_mul(inv0, D0);
            inv1 = gl_mul(inv1, D1);
            p0[(size_t)j * n] = h0;
            p1[(size_t)j * n] = h1;
            inc0 = gl_add(inc0, h0);
            inc1 = gl_add(inc1, h1);
        }
        p0[(size_t)H * n] = inc0;
        p1[(size_t)H * n] = inc1;
    }
    if (zeros) atomicAdd(zero_count, (unsigned long long)zeros);
}

// bs[z][blk] = the sum of the span's increments.  grid (n_blocks, n_zs)
__global__ __launch_bounds__(LOGUP_BLOCK) void logup_block_sums_kernel(const gl_t* __restrict__ polys, const uint32_t* __restrict__ zpoly, size_t n, size_t n_blocks,
                                                                       gl_t* __restrict__ bs) { STARKHIP_PRIO_ENTRY
    __shared__ gl_t lds[TILE_WAVES];
    const gl_t* v = polys + (size_t)zpoly[blockIdx.y] * n;
    const size_t r0 = (size_t)blockIdx.x * PERM_SPAN_ROWS;
    gl_t s = 0;
#pragma unroll
    for (unsigned it = 0; it < LOGUP_ITEMS; it++) {
        const size_t r = r0 + it * LOGUP_BLOCK + threadIdx.x;
        if (r < n) s = gl_add(s, v[r]);
    }
    gl_t total;
    (void)block_scan(s, ScanGlAdd(), (gl_t)0, lds, &total);
    if (threadIdx.x == 0) bs[(size_t)blockIdx.y * n_blocks + blockIdx.x] = total;
}

// pre[z][blk] = the sum of bs[z][0 .. blk), closing[z] = the sum of all of them.  One workgroup per Z, each lane a run of blocks
__global__ __launch_bounds__(LOGUP_BLOCK) void logup_scan_blocks_kernel(const gl_t* __restrict__ bs, size_t n_blocks, gl_t* __restrict__ pre, gl_t* __restrict__ closing) { STARKHIP_PRIO_ENTRY
    __shared__ gl_t lds[TILE_WAVES];
    const gl_t* in = bs + (size_t)blockIdx.x * n_blocks;
    gl_t* out = pre + (size_t)blockIdx.x * n_blocks;
    const size_t per = (n_blocks + LOGUP_BLOCK - 1) / LOGUP_BLOCK, j0 = threadIdx.x * per, j1 = j0 + per < n_blocks ? j0 + per : n_blocks;
    gl_t s = 0;
    for (size_t j = j0; j < j1; j++) s = gl_add(s, in[j]);
    gl_t total;
    gl_t run = block_scan(s, ScanGlAdd(), (gl_t)0, lds, &total);
    for (size_t j = j0; j < j1; j++) {
        const gl_t v = in[j];
        out[j] = run;
        run = gl_add(run, v);
    }
    if (threadIdx.x == 0) closing[blockIdx.x] = total;
}

// Z[r] <- pre[z][blk] plus the sum of the span's increments before r; in place over the increments.  grid (n_blocks, n_zs)
__global__ __launch_bounds__(LOGUP_BLOCK) void logup_apply_kernel(gl_t* __restrict__ polys, const uint32_t* __restrict__ zpoly, size_t n, size_t n_blocks,
                                                                  const gl_t* __restrict__ pre) { STARKHIP_PRIO_ENTRY
    __shared__ gl_t lds[TILE_WAVES];
    gl_t* v = polys + (size_t)zpoly[blockIdx.y] * n;
    const size_t r0 = (size_t)blockIdx.x * PERM_SPAN_ROWS;
    gl_t carry = pre[(size_t)blockIdx.y * n_blocks + blockIdx.x];
#pragma unroll
    for (unsigned it = 0; it < LOGUP_ITEMS; it++) {
        const size_t r = r0 + it * LOGUP_BLOCK + threadIdx.x;
        const gl_t x = r < n ? v[r] : 0;
        gl_t total;
        const gl_t excl = block_scan(x, ScanGlAdd(), (gl_t)0, lds, &total);
        if (r < n) v[r] = gl_add(carry, excl);
        carry = gl_add(carry, total);
    }
}

// desc: by trace column.  lde [C][N] and alde [nA][N] coset-major; tab: quotient_tables_kernel's; qvals [2][size] in natural quotient order
__global__ __launch_bounds__(LOGUP_BLOCK) void logup_quotient_kernel(const uint32_t* __restrict__ desc, const gl_t* __restrict__ lde, const gl_t* __restrict__ alde,
                                                                     gl_t chi0, gl_t chi1, const gl_t* __restrict__ tab, gl_t* __restrict__ qvals, gl_t alpha0,
                                                                     gl_t alpha1, gl_t scale0, gl_t scale1, unsigned log_n, unsigned rate_bits, unsigned qdb) { STARKHIP_PRIO_ENTRY
    const size_t n = (size_t)1 << log_n, size = n << qdb, N = n << rate_bits;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= size) return;
    const size_t sp = t >> log_n, k = t & (n - 1), i = (k << qdb) + sp;
    const size_t at0 = ((sp << (rate_bits - qdb)) << log_n) + k, at1 = ((sp << (rate_bits - qdb)) << log_n) + ((k + 1) & (n - 1));  // the point, and the next row's
    const gl_t l_first = tab[size + t], zh_inv = tab[3 * size + t];
    const uint32_t nl = desc[0], B = desc[1], half = desc[2];
    gl_t acc0 = 0, acc1 = 0;
    for (uint32_t ci = 0; ci < 2; ci++) {
        const gl_t chi = ci ? chi1 : chi0;
        uint32_t at = LOGUP_DESC_HEAD;
        for (uint32_t l = 0; l < nl; l++) {
            const uint32_t base = desc[at], m = desc[at + 1], H = (m + B - 1) / B;
            const gl_t den = gl_add(chi, lde[(size_t)desc[at + 2] * N + at0]), fv = lde[(size_t)desc[at + 3] * N + at0];  // LDE words are canonical
            const uint32_t* cs = desc + at + LOGUP_DESC_LOOKUP;
            at += LOGUP_DESC_LOOKUP + m;
            const gl_t* a = alde + (size_t)(ci * half + base) * N;
            gl_t hsum = 0;
            for (uint32_t j = 0; j < H; j++) {  // h_j prod (chi + c) - sum_c prod_{c' != c} (chi + c')
                const uint32_t c1 = (j + 1) * B < m ? (j + 1) * B : m;
                gl_t prod = 1, sum = 0;
                for (uint32_t c = j * B; c < c1; c++) {
                    const gl_t x = gl_add(chi, lde[(size_t)cs[c] * N + at0]);
                    sum = gl_add(gl_mul(sum, x), prod);
                    prod = gl_mul(prod, x);
                }
                const gl_t h = a[(size_t)j * N + at0], c = gl_sub(gl_mul(h, prod), sum);
                hsum = gl_add(hsum, h);
                acc0 = gl_add(gl_mul(acc0, alpha0), c);
                acc1 = gl_add(gl_mul(acc1, alpha1), c);
            }
            const gl_t z = a[(size_t)H * N + at0], zn = a[(size_t)H * N + at1];
            const gl_t cf = gl_mul(l_first, z);  // Z on the first row
            const gl_t cz = gl_add(gl_mul(gl_sub(gl_sub(zn, z), hsum), den), fv);  // ((Z(next) - Z) - sum_j h_j) (chi + t) + f
            acc0 = gl_add(gl_mul(gl_add(gl_mul(acc0, alpha0), cf), alpha0), cz);
            acc1 = gl_add(gl_mul(gl_add(gl_mul(acc1, alpha1), cf), alpha1), cz);
        }
    }
    qvals[i] = gl_add(gl_mul(qvals[i], scale0), gl_mul(acc0, zh_inv));
    qvals[size + i] = gl_add(gl_mul(qvals[size + i], scale1), gl_mul(acc1, zh_inv));
}

// the same for the general descriptor: the trace LDE is read at the point and at the next row's
__global__ __launch_bounds__(LOGUP_BLOCK) void logup_quotient_general_kernel(const uint32_t* __restrict__ desc, const gl_t* __restrict__ lde, const gl_t* __restrict__ alde,
                                                                             gl_t chi0, gl_t chi1, const gl_t* __restrict__ tab, gl_t* __restrict__ qvals, gl_t alpha0,
                                                                             gl_t alpha1, gl_t scale0, gl_t scale1, unsigned log_n, unsigned rate_bits, unsigned qdb) { STARKHIP_PRIO_ENTRY
    const size_t n = (size_t)1 << log_n, size = n << qdb, N = n << rate_bits;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= size) return;
    const size_t sp = t >> log_n, k = t & (n - 1), i = (k << qdb) + sp;
    const size_t at0 = ((sp << (rate_bits - qdb)) << log_n) + k, at1 = ((sp << (rate_bits - qdb)) << log_n) + ((k + 1) & (n - 1));  // the point, and the next row's
    auto cell = [&](uint32_t col, bool next) { return lde[(size_t)col * N + (next ? at1 : at0)]; };  // LDE words are canonical
    const gl_t l_first = tab[size + t], zh_inv = tab[3 * size + t];
    const uint32_t nl = desc[0], B = desc[1], half = desc[2];
    gl_t acc0 = 0, acc1 = 0;
    for (uint32_t ci = 0; ci < 2; ci++) {
        const gl_t chi = ci ? chi1 : chi0;
        uint32_t at = LOGUP_DESC_HEAD;
        for (uint32_t l = 0; l < nl; l++) {
            const uint32_t base = desc[at], m = desc[at + 1], H = (m + B - 1) / B;
            const uint32_t* w = desc + at + LOGUP_DESC_LOOKUP_GENERAL + H;
            at = desc[at + 2];
            const gl_t den = gl_add(chi, logup_desc_column(w, cell)), fv = logup_desc_column(w, cell);
            const gl_t* a = alde + (size_t)(ci * half + base) * N;
            gl_t hsum = 0;
            for (uint32_t j = 0; j < H; j++) {  // h_j prod (chi + v_c) - sum_c phi_c prod_{c' != c} (chi + v_c')
                const uint32_t c1 = (j + 1) * B < m ? (j + 1) * B : m;
                gl_t prod = 1, sum = 0;
                for (uint32_t c = j * B; c < c1; c++) {
                    const gl_t x = gl_add(chi, logup_desc_column(w, cell));
                    sum = gl_add(gl_mul(sum, x), gl_mul(logup_desc_filter(w, cell), prod));
                    prod = gl_mul(prod, x);
                }
                const gl_t h = a[(size_t)j * N + at0], c = gl_sub(gl_mul(h, prod), sum);
                hsum = gl_add(hsum, h);
                acc0 = gl_add(gl_mul(acc0, alpha0), c);
                acc1 = gl_add(gl_mul(acc1, alpha1), c);
            }
            const gl_t z = a[(size_t)H * N + at0], zn = a[(size_t)H * N + at1];
            const gl_t cf = gl_mul(l_first, z);  // Z on the first row
            const gl_t cz = gl_add(gl_mul(gl_sub(gl_sub(zn, z), hsum), den), fv);  // ((Z(next) - Z) - sum_j h_j) (chi + t) + f
            acc0 = gl_add(gl_mul(gl_add(gl_mul(acc0, alpha0), cf), alpha0), cz);
            acc1 = gl_add(gl_mul(gl_add(gl_mul(acc1, alpha1), cf), alpha1), cz);
        }
    }
    qvals[i] = gl_add(gl_mul(qvals[i], scale0), gl_mul(acc0, zh_inv));
    qvals[size + i] = gl_add(gl_mul(qvals[size + i], scale1), gl_mul(acc1, zh_inv));
}

hipError_t launch_logup_polys(const uint32_t* desc, bool general, const uint32_t* zpoly, const gl_t* cols, size_t stride, gl_t chi0, gl_t chi1, size_t n, unsigned n_zs,
                              gl_t* polys, gl_t* scratch, gl_t* results, hipStream_t st) {
    if (!n_zs) return hipSuccess;
    const size_t blocks = perm_span_count(n);
    gl_t* bs = scratch;
    gl_t* pre = scratch + (size_t)n_zs * blocks;
    unsigned long long* zero_count = (unsigned long long*)(results + n_zs);
    if (hipError_t e = hipMemsetAsync(zero_count, 0, 8, st); e != hipSuccess) return e;
    hipLaunchKernelGGL(general ? logup_terms_general_kernel : logup_terms_kernel, dim3(nb(n, LOGUP_BLOCK)), dim3(LOGUP_BLOCK), 0, st, desc, cols, stride, chi0, chi1, n,
                       polys, zero_count);
    hipLaunchKernelGGL(logup_block_sums_kernel, dim3((unsigned)blocks, n_zs), dim3(LOGUP_BLOCK), 0, st, polys, zpoly, n, blocks, bs);
    hipLaunchKernelGGL(logup_scan_blocks_kernel, dim3(n_zs), dim3(LOGUP_BLOCK), 0, st, bs, blocks, pre, results);
    hipLaunchKernelGGL(logup_apply_kernel, dim3((unsigned)blocks, n_zs), dim3(LOGUP_BLOCK), 0, st, polys, zpoly, n, blocks, pre);
    return hipGetLastError();
}

// the three scan launches alone, over increments somebody else has written (the cross-table lookups' running sums: kernels_ctl.hip)
hipError_t launch_logup_scan(const uint32_t* zpoly, size_t n, unsigned n_zs, gl_t* polys, gl_t* scratch, gl_t* totals, hipStream_t st) {
    if (!n_zs) return hipSuccess;
    const size_t blocks = perm_span_count(n);
    gl_t* bs = scratch;
    gl_t* pre = scratch + (size_t)n_zs * blocks;
    hipLaunchKernelGGL(logup_block_sums_kernel, dim3((unsigned)blocks, n_zs), dim3(LOGUP_BLOCK), 0, st, polys, zpoly, n, blocks, bs);
    hipLaunchKernelGGL(logup_scan_blocks_kernel, dim3(n_zs), dim3(LOGUP_BLOCK), 0, st, bs, blocks, pre, totals);
    hipLaunchKernelGGL(logup_apply_kernel, dim3((unsigned)blocks, n_zs), dim3(LOGUP_BLOCK), 0, st, polys, zpoly, n, blocks, pre);
    return hipGetLastError();
}

hipError_t launch_logup_quotient(const uint32_t* desc, bool general, const gl_t* lde, const gl_t* alde, gl_t chi0, gl_t chi1, const gl_t* tab, gl_t* qvals, gl_t alpha0,
                                 gl_t alpha1, gl_t scale0, gl_t scale1, unsigned log_n, unsigned rate_bits, unsigned qdb, hipStream_t st) {
    const size_t size = (size_t)1 << (log_n + qdb);
    hipLaunchKernelGGL(general ? logup_quotient_general_kernel : logup_quotient_kernel, dim3(nb(size, LOGUP_BLOCK)), dim3(LOGUP_BLOCK), 0, st, desc, lde, alde, chi0, chi1, tab, qvals, alpha0, alpha1, scale0,
                       scale1, log_n, rate_bits, qdb);
    return hipGetLastError();
}

}  // namespace starkhip
