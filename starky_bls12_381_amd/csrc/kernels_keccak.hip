// The Keccak hasher's kernels (keccak.h; COMPAT.md K1 - K8): leaf hashes of a column-major LDE and of row-major leaves, Merkle
// levels, proof-of-work grinding through the challenger's permutation, and the device verifier's leaf digests.  One lane per hash
// everywhere: Keccak-f[1600] is 25 64-bit words of plain 32-bit logic per lane -- no LDS, no table, nothing shared between lanes.
// Digests are four words (keccak_digest_words), in the slots the Poseidon kernels write, so Merkle buffers, the query gathers and the
// proof layout are the same for both hashers.
#include <hip/hip_runtime.h>

#include "keccak.h"
#include "kernels.h"
#include "verify_query.h"

namespace starkhip {

// Leaf digests of a column-major matrix laid out coset-major (kernels_hash.hip has the index rule: the lane that owns physical point
// q = s n + k writes the digest slot bitrev(k R + s)).  The 64 lanes of a wave own 64 adjacent points, so each column load is one
// 512-byte run.  17 columns per permutation; the next block's 17 words are requested before the current permutation, which is all the
// latency hiding a launch of one wave per SIMD has.  Indices and offsets are 64-bit: a FinalExp LDE is 19 GB.
__global__ __launch_bounds__(64) void leaf_hash_keccak_kernel(const gl_t* __restrict__ mat, size_t n_cols, unsigned log_n, unsigned rate_bits,
                                                              gl_t* __restrict__ digests) { STARKHIP_PRIO_ENTRY
    const unsigned log_N = log_n + rate_bits;
    const size_t N = (size_t)1 << log_N;
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q >= N) return;  // trees of fewer than 64 leaves
    const size_t s = q >> log_n, k = q & (((size_t)1 << log_n) - 1);
    const size_t i = (k << rate_bits) + s;
    const size_t j = gl_bitrev((uint32_t)i, log_N);
    const gl_t* col = mat + q;
    gl_t w[4];
    if (n_cols <= 3) {  // K4: copied, zero padded to 25 bytes
        keccak_digest_words(col[0], n_cols > 1 ? col[N] : 0, n_cols > 2 ? col[2 * N] : 0, 0, w);
    } else {
        uint64_t a[25], nx[KECCAK_RATE_WORDS];
#pragma unroll
        for (int e = 0; e < 25; e++) a[e] = 0;
        const size_t n_blocks = n_cols / KECCAK_RATE_WORDS + 1;  // the last one is partial, or only padding
        size_t rem = n_cols < KECCAK_RATE_WORDS ? n_cols : KECCAK_RATE_WORDS;
#pragma unroll
        for (int e = 0; e < KECCAK_RATE_WORDS; e++) nx[e] = (size_t)e < rem ? col[(size_t)e * N] : 0;
        for (size_t b = 0; b < n_blocks; b++) {
#pragma unroll
            for (int e = 0; e < KECCAK_RATE_WORDS; e++) a[e] ^= nx[e];
            if (b + 1 == n_blocks) {  // rem < 17: the 0x01 goes into word `rem`, the 0x80 into the top byte of word 16
#pragma unroll
                for (int e = 0; e < KECCAK_RATE_WORDS; e++) {
                    if ((size_t)e == rem) a[e] ^= 0x01ULL;
                }
                a[16] ^= KECCAK_PAD_LAST;
            } else {
                const size_t off = (b + 1) * KECCAK_RATE_WORDS;
                rem = n_cols - off < KECCAK_RATE_WORDS ? n_cols - off : KECCAK_RATE_WORDS;
#pragma unroll
                for (int e = 0; e < KECCAK_RATE_WORDS; e++) nx[e] = (size_t)e < rem ? col[(off + e) * N] : 0;
            }
            keccak_f1600(a);
        }
        keccak_digest_words(a[0], a[1], a[2], a[3], w);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) digests[4 * j + e] = w[e];
}

// Leaves stored row-major and already in tree order: leaf j = rows[j][0 .. width)
__global__ __launch_bounds__(64) void leaf_hash_rows_keccak_kernel(const gl_t* __restrict__ rows, size_t width, size_t n_leaves,
                                                                   gl_t* __restrict__ digests) { STARKHIP_PRIO_ENTRY
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n_leaves) return;
    gl_t w[4];
    keccak_hash_or_noop(rows + j * width, width, 1, w);
#pragma unroll
    for (int e = 0; e < 4; e++) digests[4 * j + e] = w[e];
}

__global__ __launch_bounds__(64) void merkle_level_keccak_kernel(const gl_t* __restrict__ child, gl_t* __restrict__ parent, size_t n_parent) { STARKHIP_PRIO_ENTRY
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n_parent) return;
    gl_t w[4];
    keccak_two_to_one(child + 8 * j, child + 8 * j + 4, w);
#pragma unroll
    for (int e = 0; e < 4; e++) parent[4 * j + e] = w[e];
}

__global__ __launch_bounds__(64) void keccak_permute_batch_kernel(gl_t* states, size_t n) { STARKHIP_PRIO_ENTRY
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    gl_t s[12];
#pragma unroll
    for (int e = 0; e < 12; e++) s[e] = states[12 * i + e];
    keccak_permute(s);
#pragma unroll
    for (int e = 0; e < 12; e++) states[12 * i + e] = s[e];
}

// pow_grind_kernel (kernels_hash.hip) with K7's permutation: the response is element 7 of the new state, the eighth word that passes
// the filter
__global__ __launch_bounds__(256) void pow_grind_keccak_kernel(const gl_t* __restrict__ base_state, int pos, unsigned pow_bits, uint64_t start,
                                                               uint64_t count, unsigned long long* best) { STARKHIP_PRIO_ENTRY
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint64_t w = start + t;
    gl_t s[12];
#pragma unroll
    for (int e = 0; e < 12; e++) s[e] = e == pos ? w : base_state[e];
    keccak_permute(s);
    if ((s[7] >> (64 - pow_bits)) == 0) atomicMin(best, (unsigned long long)w);
}

// The device verifier's leaf digests of the Keccak proofs of a chunk: one lane per descriptor; the Poseidon ones are
// verify_leaf_digest_kernel's (kernels_hash.hip).  A wave's descriptors are of like length (the host sorts them longest first).
__global__ __launch_bounds__(64) void verify_leaf_digest_keccak_kernel(const gl_t* __restrict__ words, const VQLeaf* __restrict__ leaves,
                                                                       size_t n_leaves, gl_t* __restrict__ digests) { STARKHIP_PRIO_ENTRY
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q >= n_leaves) return;
    const VQLeaf lf = leaves[q];
    if (lf.hasher != STARKHIP_HASHER_KECCAK) return;
    gl_t w[4];
    keccak_hash_or_noop(words + lf.off, lf.len, 1, w);
    gl_t* out = digests + 4 * (size_t)lf.slot;
#pragma unroll
    for (int e = 0; e < 4; e++) out[e] = w[e];
}

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

hipError_t launch_leaf_hash_keccak(const gl_t* mat, size_t n_cols, unsigned log_n, unsigned rate_bits, gl_t* digests, hipStream_t st) {
    const size_t N = (size_t)1 << (log_n + rate_bits);
    hipLaunchKernelGGL(leaf_hash_keccak_kernel, dim3(nblocks(N, 64)), dim3(64), 0, st, mat, n_cols, log_n, rate_bits, digests);
    return hipGetLastError();
}
hipError_t launch_leaf_hash_rows_keccak(const gl_t* rows, size_t width, size_t n_leaves, gl_t* digests, hipStream_t st) {
    hipLaunchKernelGGL(leaf_hash_rows_keccak_kernel, dim3(nblocks(n_leaves, 64)), dim3(64), 0, st, rows, width, n_leaves, digests);
    return hipGetLastError();
}
hipError_t launch_merkle_levels_keccak(gl_t* digests, unsigned log_leaves, unsigned cap_h, hipStream_t st) {
    gl_t* child = digests;
    for (unsigned lv = log_leaves; lv > cap_h; lv--) {
        const size_t n_parent = (size_t)1 << (lv - 1);
        gl_t* parent = child + ((size_t)4 << lv);
        hipLaunchKernelGGL(merkle_level_keccak_kernel, dim3(nblocks(n_parent, 64)), dim3(64), 0, st, child, parent, n_parent);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        child = parent;
    }
    return hipSuccess;
}
hipError_t launch_permute_batch_keccak(gl_t* states, size_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(keccak_permute_batch_kernel, dim3(nblocks(n, 64)), dim3(64), 0, st, states, n);
    return hipGetLastError();
}
hipError_t launch_pow_grind_keccak(const gl_t* base_state, int pos, unsigned pow_bits, uint64_t start, uint64_t count, unsigned long long* best,
                                   hipStream_t st) {
    hipLaunchKernelGGL(pow_grind_keccak_kernel, dim3(nblocks(count, 256)), dim3(256), 0, st, base_state, pos, pow_bits, start, count, best);
    return hipGetLastError();
}
hipError_t launch_verify_leaf_digests_keccak(const gl_t* words, const VQLeaf* leaves, size_t n_leaves, gl_t* digests, hipStream_t st) {
    if (!n_leaves) return hipSuccess;
    hipLaunchKernelGGL(verify_leaf_digest_keccak_kernel, dim3(nblocks(n_leaves, 64)), dim3(64), 0, st, words, leaves, n_leaves, digests);
    return hipGetLastError();
}

}  // namespace starkhip
