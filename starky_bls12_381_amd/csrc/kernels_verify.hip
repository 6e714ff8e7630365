// Device verifier kernels (verifier_device.cpp drives them; the leaf digests are kernels_hash.hip's verify_leaf_digest_kernel,
// which shares the row form's constant tables there).  One chunk of a batch: every proof's region of words (verify_query.h:
// VQProof), its powers of the FRI alpha, and one entry per query round.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "verify_query.h"

namespace starkhip {

// The range check of the query sections the host did not read (the CPU verifier checks every word of a proof < p; a word that is
// not turns the proof into BAD_SHAPE whatever else fails).  grid.y = proof of the chunk.
__global__ __launch_bounds__(256) void verify_range_kernel(const gl_t* __restrict__ words, const VQProof* __restrict__ proofs,
                                                           uint32_t* __restrict__ bad) { STARKHIP_PRIO_ENTRY
    const VQProof& P = proofs[blockIdx.y];
    const gl_t* w = words + P.base + P.off_queries;
    const uint64_t len = P.off_final - P.off_queries;
    bool any = false;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < len; i += (uint64_t)gridDim.x * blockDim.x) any |= w[i] >= GL_P;
    if (any) atomicOr(&bad[blockIdx.y], 1u);
}

// fri_combine_initial's two sums of one query (verifier.cpp: e0, e1), as dot products with the powers of alpha:
//   e1 = sum_c alpha^c trace[c] + sum_z alpha^(C + z) Z[z],   e0 = e1 + sum_q alpha^(C + nZ + q) quotient[q]
// One workgroup per query; the partial sums meet in LDS.
__global__ __launch_bounds__(256) void verify_combine_kernel(const gl_t* __restrict__ words, const VQProof* __restrict__ proofs,
                                                             const uint32_t* __restrict__ query_proof, const gl2_t* __restrict__ apow,
                                                             gl2_t* __restrict__ sums) { STARKHIP_PRIO_ENTRY
    __shared__ gl2_t red[2][256];
    const uint32_t g = blockIdx.x;
    const VQProof& P = proofs[query_proof[g]];
    const gl_t* tleaf = words + P.base + P.off_queries + (uint64_t)(g - P.first_query) * P.query_words;
    const gl_t* zleaf = tleaf + P.C + 4 * (P.log_N - P.cap_h);  // read only when the proof has Zs
    const gl_t* qleaf = tleaf + vq_quot_leaf_off(P);
    const gl2_t* ap = apow + P.apow;
    gl2_t st = gl2_zero(), sq = gl2_zero();
    for (uint32_t c = threadIdx.x; c < P.C; c += blockDim.x) st = gl2_add(st, gl2_mul_base(ap[c], tleaf[c]));
    for (uint32_t z = threadIdx.x; z < P.nZ; z += blockDim.x) st = gl2_add(st, gl2_mul_base(ap[P.C + z], zleaf[z]));
    for (uint32_t q = threadIdx.x; q < P.Q; q += blockDim.x) sq = gl2_add(sq, gl2_mul_base(ap[P.C + P.nZ + q], qleaf[q]));
    red[0][threadIdx.x] = st;
    red[1][threadIdx.x] = sq;
    __syncthreads();
    for (unsigned h = blockDim.x / 2; h > 0; h /= 2) {
        if (threadIdx.x < h) {
            red[0][threadIdx.x] = gl2_add(red[0][threadIdx.x], red[0][threadIdx.x + h]);
            red[1][threadIdx.x] = gl2_add(red[1][threadIdx.x], red[1][threadIdx.x + h]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[2 * (size_t)g] = gl2_add(red[0][0], red[1][0]);
        sums[2 * (size_t)g + 1] = red[0][0];
    }
}

// Every other check of a query round (verify_query.h), one lane per query: Merkle paths, the sum at x, the FRI layers, the final
// polynomial.  A few dozen sequential two-to-one hashes per lane.
__global__ __launch_bounds__(64) void verify_query_kernel(const gl_t* __restrict__ words, const VQProof* __restrict__ proofs,
                                                          const uint32_t* __restrict__ query_proof, const uint64_t* __restrict__ x_index,
                                                          const gl_t* __restrict__ digests, const gl2_t* __restrict__ sums,
                                                          uint32_t* __restrict__ status, size_t n_queries) { STARKHIP_PRIO_ENTRY
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n_queries) return;
    const VQProof& P = proofs[query_proof[i]];
    const uint32_t qi = (uint32_t)i - P.first_query;
    const gl_t* dg = digests + 4 * ((size_t)P.first_digest + (size_t)qi * vq_slots(P));
    status[i] = vq_check_query(P, words + P.base, dg, sums[2 * i], sums[2 * i + 1], x_index[i], qi);
}

hipError_t launch_verify_range(const gl_t* words, const VQProof* proofs, size_t n_proofs, uint32_t* bad, hipStream_t st) {
    if (!n_proofs) return hipSuccess;
    hipLaunchKernelGGL(verify_range_kernel, dim3(64, (unsigned)n_proofs), dim3(256), 0, st, words, proofs, bad);
    return hipGetLastError();
}
hipError_t launch_verify_combine(const gl_t* words, const VQProof* proofs, const uint32_t* query_proof, size_t n_queries, const gl2_t* apow,
                                 gl2_t* sums, hipStream_t st) {
    if (!n_queries) return hipSuccess;
    hipLaunchKernelGGL(verify_combine_kernel, dim3((unsigned)n_queries), dim3(256), 0, st, words, proofs, query_proof, apow, sums);
    return hipGetLastError();
}
hipError_t launch_verify_queries(const gl_t* words, const VQProof* proofs, const uint32_t* query_proof, const uint64_t* x_index, size_t n_queries,
                                 const gl_t* digests, const gl2_t* sums, uint32_t* status, hipStream_t st) {
    if (!n_queries) return hipSuccess;
    hipLaunchKernelGGL(verify_query_kernel, dim3(nb(n_queries, 64)), dim3(64), 0, st, words, proofs, query_proof, x_index, digests, sums, status,
                       n_queries);
    return hipGetLastError();
}

}  // namespace starkhip
