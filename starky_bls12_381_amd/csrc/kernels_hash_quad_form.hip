// The quad form's test entry point (starkhip_poseidon_permute_batch_form, form 1; the other forms': kernels_hash.hip).
//
// It is a translation unit of its own because of how the device code is optimised: every non-kernel function is internal to its module,
// and the interprocedural constant propagation that runs BEFORE inlining folds an argument that all call sites agree on into the callee.
// leaf_hash_body passes its one LDS array of triple constants to poseidon_permute_quad_merged at all three call sites; a fourth call site
// with another array in the same module undoes that and leaf_hash_kernel comes out differently scheduled (186 instead of 188 VGPRs).  So
// that the shipped kernel stays byte for byte what it was, this kernel lives here with its own constant-memory image of the SAME
// host-built tables (quad_merged_tables_host, poseidon_tables.cpp) and calls the same poseidon_permute_quad_merged (poseidon_dev.h).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "poseidon_dev.h"

namespace starkhip {

__constant__ QuadMergedTables QUAD_MERGED_FORM;

// Quad form: lane l of a quad holds words l, l + 4, l + 8.  CAP_ONLY specifies words 8 .. 11 (slot 2 of the four lanes).
template <bool CAP_ONLY>
__global__ __launch_bounds__(256) void permute_quad_form_kernel(const gl_t* __restrict__ in, gl_t* __restrict__ out, size_t n) { STARKHIP_PRIO_ENTRY
    __shared__ RcPair rcs[4][96];  // staged as leaf_hash_body (kernels_hash.hip) stages them
    for (unsigned idx = threadIdx.x; idx < 4 * 96; idx += blockDim.x) {
        const unsigned ll = idx / 96, w = idx % 96;
        const gl_t c = w < 90 ? POSEIDON_RC_DEV[12 * (w / 3) + ll + 4 * (w % 3)] : 0;
        rcs[ll][w].lo = c & 0xFFFFFFFFull;
        rcs[ll][w].hi = c >> 32;
    }
    __shared__ RcPair tks[2 * QUAD_MERGED_TRIPLES];
    __shared__ RcPair tk3s[4][3 * QUAD_MERGED_TRIPLES];
    for (unsigned idx = threadIdx.x; idx < 2 * QUAD_MERGED_TRIPLES; idx += blockDim.x) tks[idx] = QUAD_MERGED_FORM.tk[idx];
    for (unsigned idx = threadIdx.x; idx < 4 * 3 * QUAD_MERGED_TRIPLES; idx += blockDim.x)
        tk3s[idx / (3 * QUAD_MERGED_TRIPLES)][idx % (3 * QUAD_MERGED_TRIPLES)] = QUAD_MERGED_FORM.tk3[idx / (3 * QUAD_MERGED_TRIPLES)][idx % (3 * QUAD_MERGED_TRIPLES)];
    __syncthreads();
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const unsigned l = (unsigned)tid & 3u;
    const bool live = (tid >> 2) < n;
    const size_t q = live ? tid >> 2 : n - 1;
    QuadMergedCoef mc;
    {
        const uint32_t* c = QUAD_MERGED_FORM.coef[l];
#pragma unroll
        for (int e = 0; e < 36; e++) mc.n3[e / 12][e % 12] = c[e];
#pragma unroll
        for (int e = 0; e < 3; e++) {
            mc.n1[e] = c[36 + e];
            mc.n2[e] = c[39 + e];
            mc.b2[e] = c[43 + e];
            mc.b3[e] = c[46 + e];
        }
        mc.m00 = c[42];
#pragma unroll
        for (int e = 0; e < 12; e++) mc.cf[e] = c[50 + e];
    }
    const gl_t i0 = in[12 * q + l], i1 = in[12 * q + l + 4], i2 = in[12 * q + l + 8];
    gl_t s0 = i0, s1 = i1, s2 = i2;
    poseidon_permute_quad_merged<CAP_ONLY>(s0, s1, s2, l == 0 ? 8u : 0u, rcs[l], mc, tks, tk3s[l], l == 0, (l & 1u) == 0);
    if (!live) return;
    out[12 * q + l] = CAP_ONLY ? i0 : gl_canon(s0);
    out[12 * q + l + 4] = CAP_ONLY ? i1 : gl_canon(s1);
    out[12 * q + l + 8] = gl_canon(s2);
}

hipError_t launch_permute_quad_form(bool cap_only, const gl_t* in, gl_t* out, size_t n, hipStream_t st) {
    if (n == 0) return hipErrorInvalidValue;
    static bool uploaded[64];  // QUAD_MERGED_FORM's own: kernels_hash.hip's QUAD_MERGED is another symbol of the same type
    if (hipError_t e = upload_table_once(&QUAD_MERGED_FORM, quad_merged_tables_host(), sizeof QUAD_MERGED_FORM, uploaded); e != hipSuccess) return e;
    const unsigned blocks = (unsigned)((4 * n + 255) / 256);
    if (cap_only) hipLaunchKernelGGL(permute_quad_form_kernel<true>, dim3(blocks), dim3(256), 0, st, in, out, n);
    else hipLaunchKernelGGL(permute_quad_form_kernel<false>, dim3(blocks), dim3(256), 0, st, in, out, n);
    return hipGetLastError();
}

}  // namespace starkhip
