// LogUp lookups of a registered AIR (starky >= 0.2's Lookup; COMPAT.md L1 - L7): what host and device share, as permutation.h does for pairs.
//   * the descriptor the kernels of kernels_logup.hip walk -- the lookups and their columns;
//   * the constraints L4 on one frame over any field (the verifier's evaluation at zeta, starkhip_air_eval_frame_logup);
//   * the auxiliary polynomials of a trace from plain loops (starkhip_logup_polys_replay).
// Index conventions: with d the program's degree a lookup's m columns are cut in declaration order into H = ceil(m / (d - 1)) batches.
// Per challenge i (0, 1), then per lookup in declaration order, the polynomials are the H helpers and then Z: nA = 2 sum (H + 1), and
// polynomial (i, lookup, j) has index i * nA / 2 + base(lookup) + j, Z at j = H.  The constraints follow the polynomials: per
// (challenge, lookup) the H helper constraints, Z on the first row, the Z step -- nL = 2 sum (H + 2).  challenges[2] = {chi_0, chi_1}.
// A lookup's m looked-up values v_c, its table t and its frequencies f are Columns (constant + sum coefficient * cell over the local and
// the next row, the last row's next being row 0) and every v_c has a Filter phi_c (sum A B + sum C over Columns; 1 when empty):
//   h_j = sum over batch j of phi_c / (chi + v_c),  Z(r + 1) = Z(r) + sum_j h_j - f / (chi + t)
// A lookup is PLAIN when every v_c, t and f is one local cell with coefficient 1 and constant 0 and every filter is empty; a program of
// plain lookups keeps the descriptor, the kernels and so the words it always had.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "air_ir.h"

namespace starkhip {

// the distinct trace columns any Column or Filter of any lookup reads, ascending: what prove() keeps aside before the LDE overwrites the trace
inline std::vector<uint32_t> logup_columns(const AirProgram& P) {
    std::vector<uint32_t> cols;
    for (const auto& l : P.logups) l.each_column([&](uint32_t c) { cols.push_back(c); });
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    return cols;
}

// Whether the general kernels run: some lookup is not plain, or STARKHIP_LOGUP_GENERAL=1 forces them onto a plain program (for A/B
// runs and one test: the words must be the plain kernels').  Read whenever a descriptor is built.
inline bool logup_use_general(const AirProgram& P) {
    const char* e = getenv("STARKHIP_LOGUP_GENERAL");
    return P.logup_general() || (e && *e == '1');
}

// Descriptor (uint32 words): n_lookups, B = degree - 1, nA / 2, then per lookup
//   plain:   base (its first polynomial within a challenge's half), m, table, frequencies, m columns
//   general: base, m, the word after the lookup, H words -- where each batch's first value starts --, COLUMN table, COLUMN frequencies,
//            m x { COLUMN value, FILTER }
//            COLUMN := n_local | n_next << 16, constant (low, high), then per term: column, coefficient (low, high); local terms first
//            FILTER := n_products | n_sums << 16, then 2 n_products + n_sums COLUMNs
// by_slot: columns are indices into logup_columns() (the copy prove() keeps aside); otherwise trace columns.
static const uint32_t LOGUP_DESC_HEAD = 3, LOGUP_DESC_LOOKUP = 4, LOGUP_DESC_LOOKUP_GENERAL = 3;
// one COLUMN, one FILTER of the general form appended to `d`; ref(trace column): the column as the kernel numbers it
template <class Ref>
void logup_desc_push_column(std::vector<uint32_t>& d, const AirProgram::Column& c, const Ref& ref) {
    d.push_back(c.n_local | ((uint32_t)(c.terms.size() - c.n_local) << 16));
    d.push_back((uint32_t)c.constant);
    d.push_back((uint32_t)(c.constant >> 32));
    for (const auto& t : c.terms) {
        d.push_back(ref(t.col));
        d.push_back((uint32_t)t.coef);
        d.push_back((uint32_t)(t.coef >> 32));
    }
}
template <class Ref>
void logup_desc_push_filter(std::vector<uint32_t>& d, const AirProgram::Filter& f, const Ref& ref) {
    d.push_back(f.n_products | ((uint32_t)(f.cols.size() - 2 * f.n_products) << 16));
    for (const auto& fc : f.cols) logup_desc_push_column(d, fc, ref);
}
inline std::vector<uint32_t> logup_descriptor(const AirProgram& P, bool by_slot, bool general) {
    const std::vector<uint32_t> cols = logup_columns(P);
    auto ref = [&](uint32_t col) { return by_slot ? (uint32_t)(std::lower_bound(cols.begin(), cols.end(), col) - cols.begin()) : col; };
    std::vector<uint32_t> d = {(uint32_t)P.logups.size(), P.logup_batch_size(), P.logup_polys() / 2};
    auto column = [&](const AirProgram::Column& c) { logup_desc_push_column(d, c, ref); };
    auto filter = [&](const AirProgram::Filter& f) { logup_desc_push_filter(d, f, ref); };
    uint32_t base = 0;
    for (size_t l = 0; l < P.logups.size(); l++) {
        const auto& lk = P.logups[l];
        const uint32_t H = P.logup_helpers(l), B = P.logup_batch_size();
        d.push_back(base);
        d.push_back((uint32_t)lk.cols.size());
        if (!general) {
            d.push_back(ref(lk.table.col()));
            d.push_back(ref(lk.freq.col()));
            for (const auto& v : lk.cols) d.push_back(ref(v.col()));
        } else {
            const size_t at = d.size();
            d.resize(at + 1 + H);
            column(lk.table);
            column(lk.freq);
            for (size_t c = 0; c < lk.cols.size(); c++) {
                if (c % B == 0) d[at + 1 + c / B] = (uint32_t)d.size();
                column(lk.cols[c]);
                filter(lk.filters[c]);
            }
            d[at] = (uint32_t)d.size();
        }
        base += H + 1;
    }
    return d;
}

// The general descriptor's walkers, shared by the kernels: `w` moves past what is read.  cell(ref, next): the canonical value of column
// `ref` on the local (0) or the next (1) row.
template <class Cell>
GL_HD gl_t logup_desc_column(const uint32_t*& w, const Cell& cell) {
    const uint32_t nl = w[0] & 0xFFFFu, nt = nl + (w[0] >> 16);
    gl_t v = (gl_t)w[1] | ((gl_t)w[2] << 32);
    w += 3;
    for (uint32_t k = 0; k < nt; k++, w += 3) v = gl_add(v, gl_mul((gl_t)w[1] | ((gl_t)w[2] << 32), cell(w[0], k >= nl)));
    return v;
}
template <class Cell>
GL_HD gl_t logup_desc_filter(const uint32_t*& w, const Cell& cell) {
    const uint32_t np = w[0] & 0xFFFFu, ns = w[0] >> 16;
    w++;
    if (!(np | ns)) return 1;
    gl_t v = 0;
    for (uint32_t k = 0; k < np; k++) {
        const gl_t a = logup_desc_column(w, cell);
        v = gl_add(v, gl_mul(a, logup_desc_column(w, cell)));
    }
    for (uint32_t k = 0; k < ns; k++) v = gl_add(v, logup_desc_column(w, cell));
    return v;
}
GL_HD void logup_desc_skip_column(const uint32_t*& w) { w += 3 + 3 * ((w[0] & 0xFFFFu) + (w[0] >> 16)); }
GL_HD void logup_desc_skip_filter(const uint32_t*& w) {
    const uint32_t k = 2 * (w[0] & 0xFFFFu) + (w[0] >> 16);
    w++;
    for (uint32_t i = 0; i < k; i++) logup_desc_skip_column(w);
}

inline std::vector<uint32_t> logup_descriptor(const AirProgram& P, bool by_slot) { return logup_descriptor(P, by_slot, logup_use_general(P)); }

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

// A Column and a Filter on one frame over any field: O::canon on every cell read
template <class O>
typename O::T logup_column_value(const AirProgram::Column& c, const typename O::T* local, const typename O::T* next) {
    typename O::T v = O::from_base(c.constant);
    for (size_t k = 0; k < c.terms.size(); k++)
        v = O::add(v, O::mul(O::from_base(c.terms[k].coef), O::canon((k < c.n_local ? local : next)[c.terms[k].col])));
    return v;
}
template <class O>
typename O::T logup_filter_value(const AirProgram::Filter& f, const typename O::T* local, const typename O::T* next) {
    if (f.empty()) return O::one();
    typename O::T v = O::zero();
    for (size_t k = 0; k < f.cols.size(); k++)
        if (k < 2 * (size_t)f.n_products) {
            v = O::add(v, O::mul(logup_column_value<O>(f.cols[k], local, next), logup_column_value<O>(f.cols[k + 1], local, next)));
            k++;
        } else {
            v = O::add(v, logup_column_value<O>(f.cols[k], local, next));
        }
    return v;
}

// L4 on one frame: acc_j <- the fold continued over the nL LogUp constraints, acc_j = acc_j alpha_j + mask c for each of them in order.
// `acc` holds the fold over the AIR's own constraints on entry (air_eval_folded).  aux / aux_next: the nA polynomials at the point and
// at the next row's.  Every Column and Filter is evaluated on the frame (local, next).  The one place the verifiers and
// starkhip_air_eval_frame_logup go through.
template <class O>
void logup_eval_folded(const AirProgram& p, const typename O::T* local, const typename O::T* next, const typename O::T* aux, const typename O::T* aux_next,
                       const gl_t* challenges, const typename O::T masks[4], const typename O::T* alphas, int n_alpha, typename O::T* acc) {
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
            for (uint32_t j = 0; j < H; j++) {  // h_j prod (chi + v_c) - sum_c phi_c prod_{c' != c} (chi + v_c')
                const size_t c0 = (size_t)j * B, c1 = std::min<size_t>(c0 + B, lk.cols.size());
                T prod = O::one(), sum = O::zero();
                for (size_t c = c0; c < c1; c++) {
                    const T x = O::add(chi, logup_column_value<O>(lk.cols[c], local, next));
                    sum = O::add(O::mul(sum, x), O::mul(logup_filter_value<O>(lk.filters[c], local, next), prod));
                    prod = O::mul(prod, x);
                }
                fold(O::sub(O::mul(aux[at + j], prod), sum));
                hsum = O::add(hsum, aux[at + j]);
            }
            const T z = aux[at + H], zn = aux_next[at + H];
            fold(O::mul(masks[KIND_FIRST], z));  // Z(first row) = 0
            const T den = O::add(chi, logup_column_value<O>(lk.table, local, next));
            // (Z(next) - Z(local)) (chi + t) - (sum_j h_j) (chi + t) + f: a plain constraint, the wrap row counts
            fold(O::add(O::sub(O::mul(O::sub(zn, z), den), O::mul(hsum, den)), logup_column_value<O>(lk.freq, local, next)));
            at += H + 1;
        }
    }
}

// A Column and a Filter on row r of a trace of n rows (a power of two; the next row of the last is row 0).  cell(col, row): any word of
// the cell's class mod p
template <class Cell>
gl_t logup_column_at(const AirProgram::Column& c, const Cell& cell, size_t r, size_t n) {
    gl_t v = c.constant;
    for (size_t k = 0; k < c.terms.size(); k++) v = gl_add(v, gl_mul(c.terms[k].coef, gl_from_u64(cell(c.terms[k].col, k < c.n_local ? r : (r + 1) & (n - 1)))));
    return v;
}
template <class Cell>
gl_t logup_filter_at(const AirProgram::Filter& f, const Cell& cell, size_t r, size_t n) {
    if (f.empty()) return 1;
    gl_t v = 0;
    for (size_t k = 0; k < f.cols.size(); k++)
        if (k < 2 * (size_t)f.n_products) {
            v = gl_add(v, gl_mul(logup_column_at(f.cols[k], cell, r, n), logup_column_at(f.cols[k + 1], cell, r, n)));
            k++;
        } else {
            v = gl_add(v, logup_column_at(f.cols[k], cell, r, n));
        }
    return v;
}

// The auxiliary polynomials of a trace from plain loops.  cell(col, row): any word of the cell's class mod p.  polys [nA][n], closing
// [2][n_lookups] (challenge-major: Z(n - 1) plus the last row's increment), *zero_denominators: how many chi + v_c and chi + t were 0
// (their inverse is taken as 0), filtered-off cells included.
template <class Cell>
void logup_polys_host(const AirProgram& p, size_t n, const Cell& cell, const gl_t* challenges, gl_t* polys, gl_t* closing, uint64_t* zero_denominators) {
    const uint32_t B = p.logup_batch_size(), half = p.logup_polys() / 2;
    uint64_t zeros = 0;
    auto inv0 = [&](gl_t x) {
        if (x == 0) zeros++;
        return gl_inv(x);  // the inverse of 0 is 0
    };
    auto column = [&](const AirProgram::Column& c, size_t r) { return logup_column_at(c, cell, r, n); };
    auto filter = [&](const AirProgram::Filter& f, size_t r) { return logup_filter_at(f, cell, r, n); };
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
                    for (size_t c = c0; c < c1; c++) h = gl_add(h, gl_mul(filter(lk.filters[c], r), inv0(gl_add(chi, column(lk.cols[c], r)))));
                    polys[(size_t)(at + j) * n + r] = h;
                    run = gl_add(run, h);
                }
                run = gl_sub(run, gl_mul(column(lk.freq, r), inv0(gl_add(chi, column(lk.table, r)))));
            }
            closing[i * p.logups.size() + l] = run;
            at += H + 1;
        }
    }
    *zero_denominators = zeros;
}

}  // namespace starkhip
