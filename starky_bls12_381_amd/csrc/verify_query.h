// The per-query checks of the verifier (plonky2 fri::verifier::fri_verifier_query_round), written once for the device
// verifier's kernel (kernels_verify.hip) and its host replay (verifier_device.cpp, starkhip_verify_batch_replay).  The leaf
// digests and the two sums of fri_combine_initial arrive precomputed (one descriptor per opened leaf, one dot product per query);
// what is left per query is a few dozen two-to-one hashes and the FRI arithmetic, and it reports every check that failed as one
// status word.  The CPU verifier (verifier.cpp) keeps its own loop; both are written from the same equations.
#pragma once
#include <stdint.h>

#include "gl.h"
#include "keccak.h"
#include "poseidon.h"
#if defined(__HIPCC__)
#include "poseidon_dev.h"
#endif

namespace starkhip {

#define VQ_MAX_LAYERS 16

// one bit per kind of check in a query's status word
enum : uint32_t {
    VQ_TRACE_PATH = 1u,   // trace leaf -> trace cap
    VQ_QUOT_PATH = 2u,    // quotient leaf -> quotient cap
    VQ_FRI_COSET = 4u,    // a layer's coset value differs from the previous layer's evaluation (the first: the sum at x)
    VQ_FRI_PATH = 8u,     // a layer's leaf -> that layer's cap
    VQ_FINAL_POLY = 16u,  // the final polynomial at x differs from the last evaluation
    VQ_PERM_PATH = 32u,   // permutation Z leaf -> Z cap (proofs with nZ > 0)
};

// What the queries of one proof need, in the device word buffer.  A proof's region there is
//   [trace cap | (Z cap) | quotient cap | FRI caps | query rounds | final polynomial]
// (the blob's words off_trace_cap .. off_quot_cap + 4 ncap, then off_fri_caps .. off_pow; openings and the rest stay on the host).
// A proof with permutation Zs (nZ > 0) has its Z cap between the other two, the Z leaf and its siblings between the trace's and the
// quotient's in every round, and one more digest per query, the last of the query's slots.
struct VQProof {
    uint64_t base;         // first word of the region
    uint64_t query_words;  // words per query round
    uint64_t off_quot_cap, off_fri_caps, off_queries, off_final;  // within the region (the trace cap is at 0)
    uint64_t apow;         // first element of this proof's powers of the FRI alpha (C + Q of them)
    uint32_t C, Q, L, log_N, cap_h, final_len;
    uint32_t first_query;   // global index of query 0 (statuses, indices, sums)
    uint32_t first_digest;  // global slot of query 0's trace-leaf digest; query q's are first_digest + q vq_slots(P) + {0: trace, 1: quotient, 2 + l: layer l, 2 + L: Z}
    uint32_t arity_bits[VQ_MAX_LAYERS], layer_depth[VQ_MAX_LAYERS];
    uint32_t hasher;        // the proof's hasher id (header word 12): every Merkle path of its queries is checked under it
    uint32_t nZ;            // polynomials of the middle matrix: permutation Zs (header word 13) or LogUp auxiliary polynomials (word 14); 0: no such cap, leaf or digest
    uint64_t off_zs_cap;    // within the region (nZ > 0)
    gl2_t zeta, gzeta, red0, red1, alpha_pow_C;
    gl2_t betas[VQ_MAX_LAYERS];
};

// one opened leaf to hash: `len` words at `off` of the word buffer -> digest slot `slot`, under its proof's hasher
struct VQLeaf {
    uint64_t off;
    uint32_t len, slot;
    uint32_t hasher, pad_;
};

// digest slots per query
GL_HD uint32_t vq_slots(const VQProof& P) { return 2 + P.L + (P.nZ ? 1u : 0u); }
// words of a query round in front of the quotient leaf: the trace leaf and its siblings, then the Z leaf and its siblings
GL_HD uint64_t vq_quot_leaf_off(const VQProof& P) {
    const uint64_t d0 = P.log_N - P.cap_h;
    return P.C + 4 * d0 + (P.nZ ? P.nZ + 4 * d0 : 0);
}

GL_HD void vq_two_to_one(uint32_t hasher, const gl_t* a, const gl_t* b, gl_t* out) {
    if (hasher == STARKHIP_HASHER_KECCAK) {
        keccak_two_to_one(a, b, out);
        return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    poseidon_two_to_one_dev(a, b, out);
#else
    gl_t s[12];
    for (int i = 0; i < 4; i++) {
        s[i] = a[i];
        s[4 + i] = b[i];
        s[8 + i] = 0;
    }
    poseidon_permute_host(s);
    for (int i = 0; i < 4; i++) out[i] = s[i];
#endif
}

// Merkle path from a leaf digest to the cap entry the remaining index selects.  Under the Keccak hasher a sibling whose words are outside
// a digest's ranges (COMPAT.md K6) fails the path: its 25 bytes would not be the words' own.
GL_HD bool vq_path_to_cap(uint32_t hasher, const gl_t* digest, uint64_t index, const gl_t* cap, const gl_t* siblings, uint32_t depth) {
    gl_t cur[4] = {digest[0], digest[1], digest[2], digest[3]};
    bool in_range = true;
    for (uint32_t d = 0; d < depth; d++) {
        gl_t nxt[4];
        if (hasher == STARKHIP_HASHER_KECCAK) in_range = in_range && keccak_digest_in_range(siblings + 4 * d);
        gl_t l[4], r[4];  // one call site: the left and right child by value
        const bool odd = (index & 1) != 0;
        for (int i = 0; i < 4; i++) {
            const gl_t sb = siblings[4 * d + i];
            l[i] = odd ? sb : cur[i];
            r[i] = odd ? cur[i] : sb;
        }
        vq_two_to_one(hasher, l, r, nxt);
        for (int i = 0; i < 4; i++) cur[i] = nxt[i];
        index >>= 1;
    }
    const gl_t* c = cap + 4 * index;
    return in_range && cur[0] == c[0] && cur[1] == c[1] && cur[2] == c[2] && cur[3] == c[3];
}

// plonky2 fri::verifier::compute_evaluation: the arity coset values (stored bit-reversed) interpolated at beta, by Lagrange's
// formula over the coset x g^(-rev(within)) <g>.  No scratch arrays: points and values are formed where they are used.
GL_HD gl2_t vq_fold_eval(gl_t x, uint64_t within, uint32_t arity_bits, const gl_t* evals_in, gl2_t beta) {
    const uint64_t arity = (uint64_t)1 << arity_bits;
    const gl_t g = gl_root_of_unity(arity_bits);
    const uint64_t rev = gl_bitrev((uint32_t)within, arity_bits);
    const gl_t coset_start = gl_mul(x, gl_pow(g, arity - rev));
    gl2_t res = gl2_zero();
    gl_t pi = coset_start;
    for (uint64_t i = 0; i < arity; i++) {
        gl2_t num = gl2_one();
        gl_t den = 1, pj = coset_start;
        for (uint64_t j = 0; j < arity; j++) {
            if (j != i) {
                num = gl2_mul(num, gl2_sub(beta, gl2_from_base(pj)));
                den = gl_mul(den, gl_sub(pi, pj));
            }
            pj = gl_mul(pj, g);
        }
        const uint64_t k = gl_bitrev((uint32_t)i, arity_bits);  // evals[i] of the natural order = evals_in[rev(i)]
        const gl2_t ev = gl2_make(evals_in[2 * k], evals_in[2 * k + 1]);
        res = gl2_add(res, gl2_mul(ev, gl2_mul_base(num, gl_inv(den))));
        pi = gl_mul(pi, g);
    }
    return res;
}

// Every check of query `qi` of proof P.  region: the proof's words; digests: this query's 2 + L leaf digests (4 words each);
// e0, e1: fri_combine_initial's two sums over the opened trace, Z and quotient leaves; x_index: the query's index into the LDE.
// 0 = accepted; otherwise the VQ_* bits of the checks that failed.
GL_HD uint32_t vq_check_query(const VQProof& P, const gl_t* region, const gl_t* digests, gl2_t e0, gl2_t e1, uint64_t x_index, uint32_t qi) {
    uint32_t status = 0;
    const uint32_t d0 = P.log_N - P.cap_h;
    const gl_t* qp = region + P.off_queries + (uint64_t)qi * P.query_words;
    const gl_t* tsib = qp + P.C;
    const gl_t* qsib = qp + vq_quot_leaf_off(P) + P.Q;
    qp = qsib + 4 * d0;
    if (!vq_path_to_cap(P.hasher, digests, x_index, region, tsib, d0)) status |= VQ_TRACE_PATH;
    if (P.nZ && !vq_path_to_cap(P.hasher, digests + 4 * (2 + P.L), x_index, region + P.off_zs_cap, tsib + 4 * d0 + P.nZ, d0)) status |= VQ_PERM_PATH;
    if (!vq_path_to_cap(P.hasher, digests + 4, x_index, region + P.off_quot_cap, qsib, d0)) status |= VQ_QUOT_PATH;
    gl_t subgroup_x = gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(P.log_N), gl_bitrev((uint32_t)x_index, P.log_N)));
    const gl2_t xe = gl2_from_base(subgroup_x);
    gl2_t sum = gl2_mul(gl2_sub(e0, P.red0), gl2_inv(gl2_sub(xe, P.zeta)));
    sum = gl2_add(gl2_mul(sum, P.alpha_pow_C), gl2_mul(gl2_sub(e1, P.red1), gl2_inv(gl2_sub(xe, P.gzeta))));
    gl2_t old_eval = sum;
    for (uint32_t l = 0; l < P.L; l++) {
        const uint32_t ab = P.arity_bits[l];
        const uint64_t arity = (uint64_t)1 << ab;
        const gl_t* evals = qp;
        const gl_t* sib = qp + 2 * arity;
        qp = sib + 4 * (uint64_t)P.layer_depth[l];
        const uint64_t coset_index = x_index >> ab, within = x_index & (arity - 1);
        if (!gl2_eq(gl2_make(evals[2 * within], evals[2 * within + 1]), old_eval)) status |= VQ_FRI_COSET;
        old_eval = vq_fold_eval(subgroup_x, within, ab, evals, P.betas[l]);
        if (!vq_path_to_cap(P.hasher, digests + 4 * (2 + l), coset_index, region + P.off_fri_caps + (uint64_t)l * (4u << P.cap_h), sib, P.layer_depth[l]))
            status |= VQ_FRI_PATH;
        for (uint32_t b = 0; b < ab; b++) subgroup_x = gl_sqr(subgroup_x);
        x_index = coset_index;
    }
    const gl_t* fp = region + P.off_final;
    const gl2_t xf = gl2_from_base(subgroup_x);
    gl2_t acc = gl2_zero();
    for (uint32_t i = P.final_len; i-- > 0;) acc = gl2_add(gl2_mul(acc, xf), gl2_make(fp[2 * i], fp[2 * i + 1]));
    if (!gl2_eq(acc, old_eval)) status |= VQ_FINAL_POLY;
    return status;
}

}  // namespace starkhip
