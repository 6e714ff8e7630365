// LogUp lookups of a registered AIR (starky >= 0.2's Lookup; COMPAT.md L1 - L7): what host and device share, as permutation.h does for pairs.
//   * the descriptor the kernels of kernels_logup.hip walk -- the lookups and their columns;
//   * the constraints L4 on one frame over any field (the verifier's evaluation at zeta, starkhip_air_eval_frame_logup);
//   * the auxiliary polynomials of a trace from plain loops (starkhip_logup_polys_replay).
// Index conventions: with d the program's degree a lookup's m columns are cut in declaration order into H = ceil(m / (d - 1)) batches.
// Per challenge i (0, 1), then per lookup in declaration order, the polynomials are the H helpers and then Z: nA = 2 sum (H + 1), and
// polynomial (i, lookup, j) has index i * nA / 2 + base(lookup) + j, Z at j = H.  The constraints follow the polynomials: per
// (challenge, lookup) the H helper constraints, Z on the first row, the Z step -- nL = 2 sum (H + 2).  challenges[2] = {chi_0, chi_1}.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "air_ir.h"

namespace starkhip {

// the distinct columns the lookups name (looked-up columns, tables, frequencies), ascending
inline std::vector<uint32_t> logup_columns(const AirProgram& P) {
    std::vector<uint32_t> cols;
    for (const auto& l : P.logups) {
        cols.insert(cols.end(), l.cols.begin(), l.cols.end());
        cols.push_back(l.table);
        cols.push_back(l.freq);
    }
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    return cols;
}

// Descriptor (uint32 words): n_lookups, B = degree - 1, nA / 2, then per lookup: base (its first polynomial within a challenge's half),
// m, table, frequencies, m columns.  by_slot: columns are indices into logup_columns() (the copy prove() keeps aside); otherwise trace columns.
static const uint32_t LOGUP_DESC_HEAD = 3, LOGUP_DESC_LOOKUP = 4;
inline std::vector<uint32_t> logup_descriptor(const AirProgram& P, bool by_slot) {
    const std::vector<uint32_t> cols = logup_columns(P);
    auto ref = [&](uint32_t col) { return by_slot ? (uint32_t)(std::lower_bound(cols.begin(), cols.end(), col) - cols.begin()) : col; };
    std::vector<uint32_t> d = {(uint32_t)P.logups.size(), P.logup_batch_size(), P.logup_polys() / 2};
    uint32_t base = 0;
    for (size_t l = 0; l < P.logups.size(); l++) {
        const auto& lk = P.logups[l];
        d.push_back(base);
        d.push_back((uint32_t)lk.cols.size());
        d.push_back(ref(lk.table));
        d.push_back(ref(lk.freq));
        for (uint32_t c : lk.cols) d.push_back(ref(c));
        base += P.logup_helpers(l) + 1;
    }
    return d;
}

// the Zs' polynomial indices, challenge-major: what the prefix-sum launches scan ([2][n_lookups])
inline std::vector<uint32_t> logup_z_polys(const AirProgram& P) {
    std::vector<uint32_t> z;
    const uint32_t half = P.logup_polys() / 2;
    for (uint32_t i = 0; i < 2; i++) {
        uint32_t at = i * half;
        for (size_t l = 0; l < P.logups.size(); l++) {
            at += P.logup_helpers(l);
            z.push_back(at++);
        }
    }
    return z;
}

// L4 on one frame: acc_j <- the fold continued over the nL LogUp constraints, acc_j = acc_j alpha_j + mask c for each of them in order.
// `acc` holds the fold over the AIR's own constraints on entry (air_eval_folded).  aux / aux_next: the nA polynomials at the point and
// at the next row's.  Every trace operand is local.
template <class O>
void logup_eval_folded(const AirProgram& p, const typename O::T* local, const typename O::T* aux, const typename O::T* aux_next, const gl_t* challenges,
                       const typename O::T masks[4], const typename O::T* alphas, int n_alpha, typename O::T* acc) {
    typedef typename O::T T;
    const uint32_t B = p.logup_batch_size(), half = p.logup_polys() / 2;
    auto fold = [&](const T& c) {
        for (int j = 0; j < n_alpha; j++) acc[j] = O::add(O::mul(acc[j], alphas[j]), c);
    };
    for (uint32_t i = 0; i < 2; i++) {
        const T chi = O::from_base(challenges[i]);
        uint32_t at = i * half;
        for (size_t l = 0; l < p.logups.size(); l++) {
            const auto& lk = p.logups[l];
            const uint32_t H = p.logup_helpers(l);
            T hsum = O::zero();
            for (uint32_t j = 0; j < H; j++) {  // h_j prod (chi + c) - sum_c prod_{c' != c} (chi + c')
                const size_t c0 = (size_t)j * B, c1 = std::min<size_t>(c0 + B, lk.cols.size());
                T prod = O::one(), sum = O::zero();
                for (size_t c = c0; c < c1; c++) {
                    const T x = O::add(chi, O::canon(local[lk.cols[c]]));
                    sum = O::add(O::mul(sum, x), prod);
                    prod = O::mul(prod, x);
                }
                fold(O::sub(O::mul(aux[at + j], prod), sum));
                hsum = O::add(hsum, aux[at + j]);
            }
            const T z = aux[at + H], zn = aux_next[at + H];
            fold(O::mul(masks[KIND_FIRST], z));  // Z(first row) = 0
            const T den = O::add(chi, O::canon(local[lk.table]));
            // (Z(next) - Z(local)) (chi + t) - (sum_j h_j) (chi + t) + f: a plain constraint, the wrap row counts
            fold(O::add(O::sub(O::mul(O::sub(zn, z), den), O::mul(hsum, den)), O::canon(local[lk.freq])));
            at += H + 1;
        }
    }
}

// The auxiliary polynomials of a trace from plain loops.  cell(col, row): any word of the cell's class mod p.  polys [nA][n], closing
// [2][n_lookups] (challenge-major: Z(n - 1) plus the last row's increment), *zero_denominators: how many chi + cell were 0 (their inverse is taken as 0).
template <class Cell>
void logup_polys_host(const AirProgram& p, size_t n, const Cell& cell, const gl_t* challenges, gl_t* polys, gl_t* closing, uint64_t* zero_denominators) {
    const uint32_t B = p.logup_batch_size(), half = p.logup_polys() / 2;
    uint64_t zeros = 0;
    auto inv0 = [&](gl_t x) {
        if (x == 0) zeros++;
        return gl_inv(x);  // the inverse of 0 is 0
    };
    for (uint32_t i = 0; i < 2; i++) {
        const gl_t chi = challenges[i];
        uint32_t at = i * half;
        for (size_t l = 0; l < p.logups.size(); l++) {
            const auto& lk = p.logups[l];
            const uint32_t H = p.logup_helpers(l);
            gl_t* Z = polys + (size_t)(at + H) * n;
            gl_t run = 0;
            for (size_t r = 0; r < n; r++) {
                Z[r] = run;
                for (uint32_t j = 0; j < H; j++) {
                    const size_t c0 = (size_t)j * B, c1 = std::min<size_t>(c0 + B, lk.cols.size());
                    gl_t h = 0;
                    for (size_t c = c0; c < c1; c++) h = gl_add(h, inv0(gl_add(chi, gl_from_u64(cell(lk.cols[c], r)))));
                    polys[(size_t)(at + j) * n + r] = h;
                    run = gl_add(run, h);
                }
                run = gl_sub(run, gl_mul(gl_from_u64(cell(lk.freq, r)), inv0(gl_add(chi, gl_from_u64(cell(lk.table, r))))));
            }
            closing[i * p.logups.size() + l] = run;
            at += H + 1;
        }
    }
    *zero_denominators = zeros;
}

}  // namespace starkhip
