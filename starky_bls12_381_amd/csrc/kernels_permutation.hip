// Permutation arguments on gfx950 (starky's permutation_pairs(); COMPAT.md P1 - P8, permutation.h has the conventions):
//
//  * perm_ratio_kernel: one lane per row.  The pair columns are read column-major -- adjacent lanes, adjacent words -- and reduced
//    mod p as every trace reader does; per Z (batch, challenge) the lane forms prod red_lhs / prod red_rhs with the inverse taken
//    in the lane (Fermat, the inverse of 0 is 0: P8), so nothing travels to the host.
//  * the exclusive prefix product over rows, per Z, n = 2 .. 2^20, as THREE launches on the proof's stream: the product of each
//    workgroup's span of PERM_SPAN rows (perm_block_products_kernel), an exclusive scan of those products in one workgroup per Z,
//    which also leaves the closing product Z[n - 1] ratio(n - 1) (perm_scan_blocks_kernel), and the scan of each span started from its
//    prefix (perm_apply_kernel).  Inside a workgroup: block_scan (block_scan.h) under gl_mul.  No workgroup waits
//    for another inside a launch.  Field multiplication is exact and associative and every product is canonical, so the words do not
//    depend on how the rows are split.
//  * perm_quotient_kernel: one lane per point of the quotient's domain.  The AIR's own fold, already divided by Z_H, is in qvals;
//        q_j <- q_j alpha_j^(2 nZ) + (sum of the 2 nZ permutation constraints with their masks and alpha powers) / Z_H
//    which is the fold over all K + 2 nZ constraints divided by Z_H, because (a alpha^m + b) / Z_H = (a / Z_H) alpha^m + b / Z_H exactly.
//    It reads the Z LDE at the point and at the next row's point, and the pair columns of the trace LDE.  So it works behind both
//    evaluators; an AIR with pairs always runs every constraint on every coset.
// Every index is bounded by the row or point count the launch is given; the columns come from a validated program (air_validate.cpp).
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "kernels.h"
#include "kernels_permutation.h"

namespace starkhip {

static const unsigned PERM_BLOCK = TILE_BLOCK, PERM_ITEMS = PERM_SPAN_ROWS / PERM_BLOCK;  // block_scan's workgroup

// ratio[z][r] for every Z of the program.  cols: the pair columns, column c at cols + c * stride
__global__ __launch_bounds__(PERM_BLOCK) void perm_ratio_kernel(const uint32_t* __restrict__ desc, const gl_t* __restrict__ cols, size_t stride,
                                                                const gl_t* __restrict__ chal, size_t n, gl_t* __restrict__ ratio) { STARKHIP_PRIO_ENTRY
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t nb = desc[0];
    uint32_t at = 1;
    for (uint32_t b = 0; b < nb; b++) {
        const gl_t beta0 = chal[4 * b], gamma0 = chal[4 * b + 1], beta1 = chal[4 * b + 2], gamma1 = chal[4 * b + 3];
        gl_t num0 = 1, den0 = 1, num1 = 1, den1 = 1;
        const uint32_t n_inst = desc[at++];
        for (uint32_t q = 0; q < n_inst; q++) {
            const uint32_t ne = desc[at++];
            gl_t l0 = gamma0, r0 = gamma0, l1 = gamma1, r1 = gamma1, bp0 = 1, bp1 = 1;
            for (uint32_t e = 0; e < ne; e++, at += 2) {
                const gl_t lv = gl_from_u64(cols[desc[at] * stride + r]), rv = gl_from_u64(cols[desc[at + 1] * stride + r]);
                l0 = gl_add(l0, gl_mul(lv, bp0));
                r0 = gl_add(r0, gl_mul(rv, bp0));
                l1 = gl_add(l1, gl_mul(lv, bp1));
                r1 = gl_add(r1, gl_mul(rv, bp1));
                bp0 = gl_mul(bp0, beta0);
                bp1 = gl_mul(bp1, beta1);
            }
            num0 = gl_mul(num0, l0);
            den0 = gl_mul(den0, r0);
            num1 = gl_mul(num1, l1);
            den1 = gl_mul(den1, r1);
        }
        ratio[(size_t)(2 * b) * n + r] = gl_mul(num0, gl_inv(den0));
        ratio[(size_t)(2 * b + 1) * n + r] = gl_mul(num1, gl_inv(den1));
    }
}

// bp[z][blk] = the product of the span's ratios.  grid (n_blocks, nZ)
__global__ __launch_bounds__(PERM_BLOCK) void perm_block_products_kernel(const gl_t* __restrict__ ratio, size_t n, size_t n_blocks, gl_t* __restrict__ bp) { STARKHIP_PRIO_ENTRY
    __shared__ gl_t lds[TILE_WAVES];
    const gl_t* v = ratio + (size_t)blockIdx.y * n;
    const size_t r0 = (size_t)blockIdx.x * PERM_SPAN_ROWS;
    gl_t p = 1;
#pragma unroll
    for (unsigned it = 0; it < PERM_ITEMS; it++) {
        const size_t r = r0 + it * PERM_BLOCK + threadIdx.x;
        if (r < n) p = gl_mul(p, v[r]);
    }
    gl_t total;
    (void)block_scan(p, ScanMul(), (gl_t)1, lds, &total);
    if (threadIdx.x == 0) bp[(size_t)blockIdx.y * n_blocks + blockIdx.x] = total;
}

// pre[z][blk] = the product of bp[z][0 .. blk), closing[z] = the product of all of them.  One workgroup per Z, each lane a run of blocks
__global__ __launch_bounds__(PERM_BLOCK) void perm_scan_blocks_kernel(const gl_t* __restrict__ bp, size_t n_blocks, gl_t* __restrict__ pre, gl_t* __restrict__ closing) { STARKHIP_PRIO_ENTRY
    __shared__ gl_t lds[TILE_WAVES];
    const gl_t* in = bp + (size_t)blockIdx.x * n_blocks;
    gl_t* out = pre + (size_t)blockIdx.x * n_blocks;
    const size_t per = (n_blocks + PERM_BLOCK - 1) / PERM_BLOCK, j0 = threadIdx.x * per, j1 = j0 + per < n_blocks ? j0 + per : n_blocks;
    gl_t p = 1;
    for (size_t j = j0; j < j1; j++) p = gl_mul(p, in[j]);
    gl_t total;
    gl_t run = block_scan(p, ScanMul(), (gl_t)1, lds, &total);
    for (size_t j = j0; j < j1; j++) {
        const gl_t v = in[j];
        out[j] = run;
        run = gl_mul(run, v);
    }
    if (threadIdx.x == 0) closing[blockIdx.x] = total;
}

// zs[z][r] <- pre[z][blk] times the product of the span's ratios before r; in place over the ratios.  grid (n_blocks, nZ)
__global__ __launch_bounds__(PERM_BLOCK) void perm_apply_kernel(gl_t* __restrict__ zs, size_t n, size_t n_blocks, const gl_t* __restrict__ pre) { STARKHIP_PRIO_ENTRY
    __shared__ gl_t lds[TILE_WAVES];
    gl_t* v = zs + (size_t)blockIdx.y * n;
    const size_t r0 = (size_t)blockIdx.x * PERM_SPAN_ROWS;
    gl_t carry = pre[(size_t)blockIdx.y * n_blocks + blockIdx.x];
#pragma unroll
    for (unsigned it = 0; it < PERM_ITEMS; it++) {
        const size_t r = r0 + it * PERM_BLOCK + threadIdx.x;
        const gl_t x = r < n ? v[r] : 1;
        gl_t total;
        const gl_t excl = block_scan(x, ScanMul(), (gl_t)1, lds, &total);
        if (r < n) v[r] = gl_mul(carry, excl);
        carry = gl_mul(carry, total);
    }
}

// desc: by trace column.  lde [C][N] and zlde [nZ][N] coset-major; tab: quotient_tables_kernel's; qvals [2][size] in natural quotient order
__global__ __launch_bounds__(PERM_BLOCK) void perm_quotient_kernel(const uint32_t* __restrict__ desc, const gl_t* __restrict__ lde, const gl_t* __restrict__ zlde,
                                                                   const gl_t* __restrict__ chal, const gl_t* __restrict__ tab, gl_t* __restrict__ qvals,
                                                                   gl_t alpha0, gl_t alpha1, gl_t scale0, gl_t scale1, unsigned log_n, unsigned rate_bits,
                                                                   unsigned qdb) { STARKHIP_PRIO_ENTRY
    const size_t n = (size_t)1 << log_n, size = n << qdb, N = n << rate_bits;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= size) return;
    const size_t sp = t >> log_n, k = t & (n - 1), i = (k << qdb) + sp;
    const size_t at0 = ((sp << (rate_bits - qdb)) << log_n) + k, at1 = ((sp << (rate_bits - qdb)) << log_n) + ((k + 1) & (n - 1));  // the point, and the next row's
    const gl_t l_first = tab[size + t], zh_inv = tab[3 * size + t];
    const uint32_t nb = desc[0];
    gl_t acc0 = 0, acc1 = 0;
    for (uint32_t z = 0; z < 2 * nb; z++) {  // Z_z(local) - 1 on the first row
        const gl_t c = gl_mul(l_first, gl_sub(zlde[(size_t)z * N + at0], 1));
        acc0 = gl_add(gl_mul(acc0, alpha0), c);
        acc1 = gl_add(gl_mul(acc1, alpha1), c);
    }
    uint32_t at = 1;
    for (uint32_t b = 0; b < nb; b++) {
        const gl_t beta0 = chal[4 * b], gamma0 = chal[4 * b + 1], beta1 = chal[4 * b + 2], gamma1 = chal[4 * b + 3];
        gl_t num0 = 1, den0 = 1, num1 = 1, den1 = 1;
        const uint32_t n_inst = desc[at++];
        for (uint32_t q = 0; q < n_inst; q++) {
            const uint32_t ne = desc[at++];
            gl_t l0 = gamma0, r0 = gamma0, l1 = gamma1, r1 = gamma1, bp0 = 1, bp1 = 1;
            for (uint32_t e = 0; e < ne; e++, at += 2) {
                const gl_t lv = lde[(size_t)desc[at] * N + at0], rv = lde[(size_t)desc[at + 1] * N + at0];  // LDE words are canonical
                l0 = gl_add(l0, gl_mul(lv, bp0));
                r0 = gl_add(r0, gl_mul(rv, bp0));
                l1 = gl_add(l1, gl_mul(lv, bp1));
                r1 = gl_add(r1, gl_mul(rv, bp1));
                bp0 = gl_mul(bp0, beta0);
                bp1 = gl_mul(bp1, beta1);
            }
            num0 = gl_mul(num0, l0);
            den0 = gl_mul(den0, r0);
            num1 = gl_mul(num1, l1);
            den1 = gl_mul(den1, r1);
        }
        const gl_t* z0 = zlde + (size_t)(2 * b) * N;
        const gl_t* z1 = z0 + N;
        const gl_t c0 = gl_sub(gl_mul(z0[at1], den0), gl_mul(z0[at0], num0));
        const gl_t c1 = gl_sub(gl_mul(z1[at1], den1), gl_mul(z1[at0], num1));
        acc0 = gl_add(gl_mul(gl_add(gl_mul(acc0, alpha0), c0), alpha0), c1);
        acc1 = gl_add(gl_mul(gl_add(gl_mul(acc1, alpha1), c0), alpha1), c1);
    }
    qvals[i] = gl_add(gl_mul(qvals[i], scale0), gl_mul(acc0, zh_inv));
    qvals[size + i] = gl_add(gl_mul(qvals[size + i], scale1), gl_mul(acc1, zh_inv));
}

hipError_t launch_perm_zs(const uint32_t* desc, const gl_t* cols, size_t stride, const gl_t* chal, size_t n, unsigned n_zs, gl_t* zs, gl_t* scratch,
                          gl_t* closing, hipStream_t st) {
    if (!n_zs) return hipSuccess;
    const size_t blocks = perm_span_count(n);
    gl_t* bp = scratch;
    gl_t* pre = scratch + (size_t)n_zs * blocks;
    hipLaunchKernelGGL(perm_ratio_kernel, dim3(nb(n, PERM_BLOCK)), dim3(PERM_BLOCK), 0, st, desc, cols, stride, chal, n, zs);
    hipLaunchKernelGGL(perm_block_products_kernel, dim3((unsigned)blocks, n_zs), dim3(PERM_BLOCK), 0, st, zs, n, blocks, bp);
    hipLaunchKernelGGL(perm_scan_blocks_kernel, dim3(n_zs), dim3(PERM_BLOCK), 0, st, bp, blocks, pre, closing);
    hipLaunchKernelGGL(perm_apply_kernel, dim3((unsigned)blocks, n_zs), dim3(PERM_BLOCK), 0, st, zs, n, blocks, pre);
    return hipGetLastError();
}

hipError_t launch_perm_quotient(const uint32_t* desc, const gl_t* lde, const gl_t* zlde, const gl_t* chal, const gl_t* tab, gl_t* qvals, gl_t alpha0,
                                gl_t alpha1, gl_t scale0, gl_t scale1, unsigned log_n, unsigned rate_bits, unsigned qdb, hipStream_t st) {
    const size_t size = (size_t)1 << (log_n + qdb);
    hipLaunchKernelGGL(perm_quotient_kernel, dim3(nb(size, PERM_BLOCK)), dim3(PERM_BLOCK), 0, st, desc, lde, zlde, chal, tab, qvals, alpha0, alpha1, scale0,
                       scale1, log_n, rate_bits, qdb);
    return hipGetLastError();
}

}  // namespace starkhip
