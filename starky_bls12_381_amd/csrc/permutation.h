// Permutation arguments of a registered AIR (starky's Stark::permutation_pairs(); COMPAT.md P1 - P8): what host and device share.
//   * the descriptor the kernels of kernels_permutation.hip walk -- the batches, their instances (pairs) and the pairs' columns;
//   * the constraints P4 on one frame over any field (the verifier's evaluation at zeta, starkhip_air_eval_frame_full);
//   * the Z polynomials of a trace from plain loops (starkhip_permutation_zs_replay).
// Index conventions: pair p belongs to batch p / B (B = AirProgram::perm_batch_size()); Z index z = batch * 2 + challenge;
// challenges[(set * 2 + challenge) * 2 + {0: beta, 1: gamma}], set-major as the transcript draws them, batch b using set b.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "air_ir.h"

namespace starkhip {

// Descriptor (uint32 words): n_batches, then per batch: n_instances, then per instance: n_entries and n_entries x (lhs, rhs).
// by_slot: lhs / rhs are indices into perm_columns() (the copy of the pair columns prove() keeps aside); otherwise trace columns.
inline std::vector<uint32_t> perm_columns(const AirProgram& P) {  // the distinct columns the pairs name, ascending
    std::vector<uint32_t> cols;
    for (const auto& pr : P.perm_pairs)
        for (uint64_t e : pr) {
            cols.push_back((uint32_t)e);
            cols.push_back((uint32_t)(e >> 32));
        }
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    return cols;
}
inline std::vector<uint32_t> perm_descriptor(const AirProgram& P, bool by_slot) {
    const std::vector<uint32_t> cols = perm_columns(P);
    auto ref = [&](uint32_t col) { return by_slot ? (uint32_t)(std::lower_bound(cols.begin(), cols.end(), col) - cols.begin()) : col; };
    const uint32_t B = P.perm_batch_size(), nb = P.perm_batches();
    std::vector<uint32_t> d = {nb};
    for (uint32_t b = 0; b < nb; b++) {
        const size_t p0 = (size_t)b * B, p1 = std::min<size_t>(p0 + B, P.perm_pairs.size());
        d.push_back((uint32_t)(p1 - p0));
        for (size_t p = p0; p < p1; p++) {
            d.push_back((uint32_t)P.perm_pairs[p].size());
            for (uint64_t e : P.perm_pairs[p]) {
                d.push_back(ref((uint32_t)e));
                d.push_back(ref((uint32_t)(e >> 32)));
            }
        }
    }
    return d;
}

// P4 on one frame: acc_j <- the fold continued over the 2 nZ permutation constraints, acc_j = acc_j alpha_j + mask c for each of them
// in order -- nZ first-row constraints Z_z(local) - 1, then nZ plain ones Z_z(next) prod red_rhs(local) - Z_z(local) prod red_lhs(local),
// red = gamma + sum_t beta^t cell_t.  `acc` holds the fold over the AIR's own constraints on entry (air_eval_folded).
template <class O>
void perm_eval_folded(const AirProgram& p, const typename O::T* local, const typename O::T* zs, const typename O::T* zs_next, const gl_t* challenges,
                      const typename O::T masks[4], const typename O::T* alphas, int n_alpha, typename O::T* acc) {
    typedef typename O::T T;
    const uint32_t B = p.perm_batch_size(), nb = p.perm_batches(), nz = 2 * nb;
    for (uint32_t z = 0; z < nz; z++) {
        const T c = O::mul(masks[KIND_FIRST], O::sub(zs[z], O::one()));
        for (int j = 0; j < n_alpha; j++) acc[j] = O::add(O::mul(acc[j], alphas[j]), c);
    }
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t i = 0; i < 2; i++) {
            const gl_t beta = challenges[(b * 2 + i) * 2], gamma = challenges[(b * 2 + i) * 2 + 1];
            T num = O::one(), den = O::one();
            const size_t p0 = (size_t)b * B, p1 = std::min<size_t>(p0 + B, p.perm_pairs.size());
            for (size_t q = p0; q < p1; q++) {
                T rl = O::from_base(gamma), rr = O::from_base(gamma);
                gl_t bp = 1;
                for (uint64_t e : p.perm_pairs[q]) {
                    rl = O::add(rl, O::mul_base(O::canon(local[(uint32_t)e]), bp));
                    rr = O::add(rr, O::mul_base(O::canon(local[(uint32_t)(e >> 32)]), bp));
                    bp = gl_mul(bp, beta);
                }
                num = O::mul(num, rl);
                den = O::mul(den, rr);
            }
            const uint32_t z = b * 2 + i;
            const T c = O::sub(O::mul(zs_next[z], den), O::mul(zs[z], num));  // a plain constraint: the wrap row counts
            for (int j = 0; j < n_alpha; j++) acc[j] = O::add(O::mul(acc[j], alphas[j]), c);
        }
}

// The Z polynomials of a trace from plain loops.  cell(col, row): any word of the cell's class mod p.  zs [nZ][n], closing [nZ].
template <class Cell>
void perm_zs_host(const AirProgram& p, size_t n, const Cell& cell, const gl_t* challenges, gl_t* zs, gl_t* closing) {
    const uint32_t B = p.perm_batch_size(), nb = p.perm_batches();
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t i = 0; i < 2; i++) {
            const gl_t beta = challenges[(b * 2 + i) * 2], gamma = challenges[(b * 2 + i) * 2 + 1];
            gl_t* Z = zs + (size_t)(b * 2 + i) * n;
            gl_t run = 1;
            const size_t p0 = (size_t)b * B, p1 = std::min<size_t>(p0 + B, p.perm_pairs.size());
            for (size_t r = 0; r < n; r++) {
                Z[r] = run;
                gl_t num = 1, den = 1;
                for (size_t q = p0; q < p1; q++) {
                    gl_t rl = gamma, rr = gamma, bp = 1;
                    for (uint64_t e : p.perm_pairs[q]) {
                        rl = gl_add(rl, gl_mul(gl_from_u64(cell((uint32_t)e, r)), bp));
                        rr = gl_add(rr, gl_mul(gl_from_u64(cell((uint32_t)(e >> 32), r)), bp));
                        bp = gl_mul(bp, beta);
                    }
                    num = gl_mul(num, rl);
                    den = gl_mul(den, rr);
                }
                run = gl_mul(run, gl_mul(num, gl_inv(den)));  // the inverse of 0 is 0 (P8)
            }
            closing[b * 2 + i] = run;
        }
}

}  // namespace starkhip
