// Cross-table lookups of a system of registered AIRs (starky >= 0.2's CrossTableLookup; COMPAT.md 2d, C1 - C8): what host and device share,
// as logup.h does for the lookups inside one trace.
//   * the system -- its tables and its CTLs -- and one table's endpoints in system order;
//   * the descriptor the kernels of kernels_ctl.hip walk;
//   * the four constraints C4 on one frame over any field (ctl_eval_folded: every verifier path and starkhip_system_eval_frame_ctl);
//   * the polynomials and sums of a trace from plain loops (starkhip_ctl_polys_replay).
// An endpoint is (table, w Columns, one Filter); under the challenge pair (beta_i, gamma_i) row r has
//   c(r) = gamma + sum_j beta^j columns[j](r),   h(r) = filter(r) / c(r),   Z(0) = 0, Z(r + 1) = Z(r) + h(r),   S = Z(n - 1) + h(n - 1)
// System order of a table's endpoints: CTL after CTL, inside a CTL the looked endpoint first and then the looking ones as declared.
// Polynomial (challenge i, endpoint e of E) has index 2 (i E + e) for h and 2 (i E + e) + 1 for Z, behind the table's LogUp polynomials;
// nC = 4 E.  sums[i E + e].  challenges[4] = {beta_0, gamma_0, beta_1, gamma_1}.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/starkhip.h"
#include "air_ir.h"
#include "logup.h"

namespace starkhip {

static const uint64_t SYSTEM_MAGIC = 0x31304C5443535953ULL;  // "SYSCTL01": a system blob (starkhip_system_register)
static const uint32_t SYSTEM_MAX_TABLES = STARKHIP_SYSTEM_MAX_TABLES, SYSTEM_MAX_CTLS = STARKHIP_SYSTEM_MAX_CTLS, SYSTEM_MAX_LOOKING = STARKHIP_SYSTEM_MAX_LOOKING,
                      CTL_MAX_WIDTH = STARKHIP_CTL_MAX_WIDTH;  // include/starkhip.h

struct CtlEndpoint {
    uint32_t table = 0;
    std::vector<AirProgram::Column> cols;
    AirProgram::Filter filter;
    uint32_t ctl = 0;     // the CTL it belongs to
    bool looked = false;  // ... and its side
    template <class F> void each_column(const F& f) const {
        for (const auto& c : cols) c.each_column(f);
        for (const auto& c : filter.cols) c.each_column(f);
    }
};
struct Ctl {
    uint32_t width = 0;
    CtlEndpoint looked;
    std::vector<CtlEndpoint> looking;
};
// one table's endpoints in system order: what its prover, its verifier and the kernels take
struct CtlTable {
    std::vector<CtlEndpoint> eps;
    size_t polys() const { return 4 * eps.size(); }        // nC
    size_t constraints() const { return 8 * eps.size(); }  // four per (challenge, endpoint)
};
struct SystemProgram {
    std::vector<int> airs;  // the tables
    std::vector<Ctl> ctls;
    CtlTable table(uint32_t t) const {
        CtlTable T;
        for (const Ctl& k : ctls) {
            if (k.looked.table == t) T.eps.push_back(k.looked);
            for (const CtlEndpoint& e : k.looking)
                if (e.table == t) T.eps.push_back(e);
        }
        return T;
    }
};

// the distinct trace columns the endpoints read, ascending: what the prover keeps aside behind the LogUp columns
inline std::vector<uint32_t> ctl_columns(const CtlTable& T) {
    std::vector<uint32_t> cols;
    for (const auto& e : T.eps) e.each_column([&](uint32_t c) { cols.push_back(c); });
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    return cols;
}

// Descriptor (uint32 words): E, then E words -- where each endpoint starts --, then per endpoint: w, w COLUMNs, FILTER (logup.h's forms).
// by_slot: columns are slot_base + the index into ctl_columns(); otherwise trace columns.
inline std::vector<uint32_t> ctl_descriptor(const CtlTable& T, bool by_slot, uint32_t slot_base = 0) {
    const std::vector<uint32_t> cols = ctl_columns(T);
    auto ref = [&](uint32_t col) { return by_slot ? slot_base + (uint32_t)(std::lower_bound(cols.begin(), cols.end(), col) - cols.begin()) : col; };
    const size_t E = T.eps.size();
    std::vector<uint32_t> d(1 + E);
    d[0] = (uint32_t)E;
    for (size_t e = 0; e < E; e++) {
        d[1 + e] = (uint32_t)d.size();
        d.push_back((uint32_t)T.eps[e].cols.size());
        for (const auto& c : T.eps[e].cols) logup_desc_push_column(d, c, ref);
        logup_desc_push_filter(d, T.eps[e].filter, ref);
    }
    return d;
}
// the Zs' polynomial indices within the middle matrix, challenge-major: what the prefix-sum launches scan ([2][E]); first: the LogUp polynomials in front
inline std::vector<uint32_t> ctl_z_polys(const CtlTable& T, uint32_t first) {
    std::vector<uint32_t> z;
    for (uint32_t k = 0; k < 2 * T.eps.size(); k++) z.push_back(first + 2 * k + 1);
    return z;
}

// C4 on one frame: acc_j <- the fold continued over the 8 E CTL constraints, per (challenge, endpoint) in this order
//   plain h c - filter;  first-row Z;  transition Z(next) - Z - h;  last-row Z + h - S.
// `acc` holds the fold over the AIR's own and the LogUp constraints on entry.  aux / aux_next: the 4 E CTL polynomials at the point and at
// the next row's; sums: the 2 E sums of the proof.  The one place the verifiers and starkhip_system_eval_frame_ctl go through.
template <class O>
void ctl_eval_folded(const CtlTable& T, const typename O::T* local, const typename O::T* next, const typename O::T* aux, const typename O::T* aux_next,
                     const gl_t* challenges, const gl_t* sums, const typename O::T masks[4], const typename O::T* alphas, int n_alpha, typename O::T* acc) {
    typedef typename O::T V;
    const size_t E = T.eps.size();
    auto fold = [&](const V& c) {
        for (int j = 0; j < n_alpha; j++) acc[j] = O::add(O::mul(acc[j], alphas[j]), c);
    };
    for (size_t i = 0; i < 2; i++) {
        const V beta = O::from_base(challenges[2 * i]);
        for (size_t e = 0; e < E; e++) {
            const CtlEndpoint& ep = T.eps[e];
            V c = O::from_base(challenges[2 * i + 1]), bp = O::one();
            for (const auto& col : ep.cols) {
                c = O::add(c, O::mul(bp, logup_column_value<O>(col, local, next)));
                bp = O::mul(bp, beta);
            }
            const V h = aux[2 * (i * E + e)], z = aux[2 * (i * E + e) + 1], zn = aux_next[2 * (i * E + e) + 1];
            fold(O::sub(O::mul(h, c), logup_filter_value<O>(ep.filter, local, next)));
            fold(O::mul(masks[KIND_FIRST], z));
            fold(O::mul(masks[KIND_TRANSITION], O::sub(O::sub(zn, z), h)));
            fold(O::mul(masks[KIND_LAST], O::sub(O::add(z, h), O::from_base(sums[i * E + e]))));
        }
    }
}

// The polynomials of a trace from plain loops.  cell(col, row): any word of the cell's class mod p.  polys [4 E][n], sums [2 E],
// *zero_denominators: how many c(r) were 0 (their inverse is taken as 0), filtered-off rows included.
template <class Cell>
void ctl_polys_host(const CtlTable& T, size_t n, const Cell& cell, const gl_t* challenges, gl_t* polys, gl_t* sums, uint64_t* zero_denominators) {
    const size_t E = T.eps.size();
    uint64_t zeros = 0;
    for (size_t i = 0; i < 2; i++) {
        const gl_t beta = challenges[2 * i], gamma = challenges[2 * i + 1];
        for (size_t e = 0; e < E; e++) {
            const CtlEndpoint& ep = T.eps[e];
            gl_t* H = polys + 2 * (i * E + e) * n;
            gl_t* Z = H + n;
            gl_t run = 0;
            for (size_t r = 0; r < n; r++) {
                gl_t c = gamma, bp = 1;
                for (const auto& col : ep.cols) {
                    c = gl_add(c, gl_mul(bp, logup_column_at(col, cell, r, n)));
                    bp = gl_mul(bp, beta);
                }
                if (c == 0) zeros++;
                H[r] = gl_mul(logup_filter_at(ep.filter, cell, r, n), gl_inv(c));  // the inverse of 0 is 0
                Z[r] = run;
                run = gl_add(run, H[r]);
            }
            sums[i * E + e] = run;
        }
    }
    *zero_denominators = zeros;
}

// Whether every CTL's sums balance: sums_of[t] the 2 E_t sums of table t.  -1, or the first CTL that does not.
inline int ctl_first_unbalanced(const SystemProgram& S, const std::vector<std::vector<gl_t>>& sums_of) {
    std::vector<size_t> at(S.airs.size(), 0), E(S.airs.size());
    for (size_t t = 0; t < S.airs.size(); t++) E[t] = sums_of[t].size() / 2;
    for (size_t k = 0; k < S.ctls.size(); k++) {
        gl_t diff[2] = {0, 0};
        auto take = [&](const CtlEndpoint& e, bool looked) {
            for (size_t i = 0; i < 2; i++) {
                const gl_t s = sums_of[e.table][i * E[e.table] + at[e.table]];
                diff[i] = looked ? gl_sub(diff[i], s) : gl_add(diff[i], s);
            }
            at[e.table]++;
        };
        take(S.ctls[k].looked, true);
        for (const CtlEndpoint& e : S.ctls[k].looking) take(e, false);
        if (diff[0] != 0 || diff[1] != 0) return (int)k;
    }
    return -1;
}

}  // namespace starkhip
