// Proof blob layout helpers (layout documented in include/starkhip.h; field order of
// starky's StarkProofWithPublicInputs).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/starkhip.h"
#include "air_ir.h"
#include "gl.h"

namespace starkhip {

struct FriGeometry {
    unsigned log_n, rate_bits, cap_h, log_N;
    std::vector<unsigned> arities;  // reduction_arity_bits
    size_t final_poly_len;
    // The one config rule of every prove, pool and verify entry point (starkhip_fri_geometry exposes it): plonky2
    // FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits), App. A.8,
    //     while db > final_poly_bits && db + rate_bits - arity_bits >= cap_height { push arity_bits; assert!(db >= arity_bits); db -= arity_bits }
    // with the comparison taken over the integers, refused where plonky2's assert fires; then the limits the proof header can carry
    // (ProofLayout::read_header) and the ones the project supports: 2 challenges, rate_bits <= 8, cap_height <= 16 and <= log_n +
    // rate_bits, 1 <= arity_bits <= 8, at most 16 FRI layers, proof_of_work_bits <= 64, log_n <= 32.  False = BAD_SHAPE.
    static bool make(const starkhip_config_t& cfg, unsigned log_n, FriGeometry* g) {
        g->log_n = log_n;
        g->rate_bits = cfg.rate_bits;
        g->cap_h = cfg.cap_height;
        g->log_N = log_n + cfg.rate_bits;
        g->arities.clear();
        g->final_poly_len = 0;
        if (cfg.num_challenges != 2 || cfg.rate_bits > 8 || cfg.cap_height > 16 || cfg.arity_bits < 1 || cfg.arity_bits > 8 ||
            cfg.proof_of_work_bits > 64 || log_n > 32 || g->log_N < g->cap_h)
            return false;
        unsigned db = log_n;
        while (db > cfg.final_poly_bits && db + cfg.rate_bits >= cfg.cap_height + cfg.arity_bits) {
            if (db < cfg.arity_bits || g->arities.size() == 16) return false;
            g->arities.push_back(cfg.arity_bits);
            db -= cfg.arity_bits;
        }
        // every layer keeps db + rate_bits >= cap_height, so the arities never exceed log_N - cap_height
        g->final_poly_len = (size_t)1 << db;
        return true;
    }
};

// the quotient degree factor of an AIR of constraint degree `degree`: degree - 1, at least 1 (a proof has 2 x factor quotient polynomials)
inline unsigned quotient_factor(unsigned degree) { return degree > 1 ? degree - 1 : 1; }
// log2 of it, rounded up; a config needs rate_bits >= it
inline unsigned quotient_degree_bits(unsigned degree) {
    const unsigned factor = quotient_factor(degree);
    unsigned qdb = 0;
    while ((1u << qdb) < factor) qdb++;
    return qdb;
}

// One matrix of polynomials a proof commits -- in proof order the trace, the middle matrix (the permutation Zs of an AIR with pairs, or the auxiliary polynomials of one with LogUp lookups), the quotient -- and where its words are.  A proof
// treats them alike (a cap in the transcript, openings, a run of powers of the FRI alpha, a leaf and a path per query round), so the prover and both verifiers walk ProofLayout::mat.
struct MatrixLayout {
    size_t cols, off_cap;           // polynomials (a leaf's words), and its cap [2^cap_h][4]
    size_t n_open[2], off_open[2];  // how many are opened at zeta (all) and at g zeta (all, or none: the quotient), 2 words each, and where
    size_t q_leaf, q_sib;           // inside a query round: its leaf, its log N - cap_h siblings of 4 words
};

struct ProofLayout {
    size_t C, Q, log_n, rate_bits, cap_h, L, n_queries, final_len, n_pis, arity_bits, n_challenges;
    size_t hasher = 0;  // header word 12: STARKHIP_HASHER_POSEIDON (0, what the word has always been) or STARKHIP_HASHER_KECCAK
    size_t nZ = 0;      // header word 13: permutation Z polynomials (0, what the word has always been, for an AIR without pairs)
    size_t nA = 0;      // header word 14: LogUp auxiliary polynomials (0, what the word has always been, for an AIR without LogUp lookups); never beside nZ
    size_t nC = 0;      // header word 15: cross-table-lookup polynomials, 4 per endpoint of the table, behind the nA LogUp ones in the middle matrix (0, what the
                        // word has always been, for a proof that is no table of a system with endpoints); never beside nZ
    size_t ncap;     // 2^cap_h
    size_t log_N;
    MatrixLayout mat[3];  // the committed matrices, n_mats of them: trace, the middle matrix if nZ + nA > 0, quotient (the last)
    size_t middle() const { return nZ + nA + nC; }  // the middle matrix's polynomials: the Zs, or LogUp || CTL
    size_t n_mats = 0;
    size_t batch_cols[2];  // polynomials opened at zeta (all) and at g zeta: the lengths of the two FRI batches
    // offsets (in words) of what follows the matrices' caps and openings
    size_t off_fri_caps, off_queries, query_words, off_final, off_pow, off_pis, off_sums, total;  // (off_sums: the nC / 2 CTL sums, the last section)
    std::vector<size_t> layer_depth;  // siblings per FRI layer

    // the layout of a proof of AIR program `P` with 2^log_n rows under `cfg` (`geo`: FriGeometry::make(cfg, log_n))
    static ProofLayout make(const AirProgram& P, const starkhip_config_t& cfg, const FriGeometry& geo, unsigned log_n, unsigned hasher = 0, size_t n_ctl_polys = 0) {
        ProofLayout pl;
        pl.hasher = hasher;
        pl.C = P.n_cols; pl.Q = (size_t)quotient_factor(P.degree) * 2; pl.log_n = log_n; pl.rate_bits = cfg.rate_bits; pl.cap_h = cfg.cap_height;
        pl.L = geo.arities.size(); pl.n_queries = cfg.num_query_rounds; pl.final_len = geo.final_poly_len; pl.n_pis = P.n_pis;
        pl.arity_bits = cfg.arity_bits; pl.n_challenges = 2;
        pl.nZ = P.perm_zs();
        pl.nA = P.logup_polys();
        pl.nC = n_ctl_polys;
        pl.compute();
        return pl;
    }
    const MatrixLayout& quotient() const { return mat[n_mats - 1]; }
    void compute() {
        ncap = (size_t)1 << cap_h;
        log_N = log_n + rate_bits;
        const size_t d0 = log_N - cap_h;
        n_mats = middle() ? 3 : 2;
        mat[0].cols = C; mat[1].cols = middle(); mat[n_mats - 1].cols = Q;
        size_t o = 16 + n_mats * 4 * ncap, q = 0;  // the caps back to back, then the openings matrix by matrix
        batch_cols[0] = batch_cols[1] = 0;
        for (size_t k = 0; k < n_mats; k++) {
            MatrixLayout& m = mat[k];
            m.off_cap = 16 + k * 4 * ncap;
            for (size_t b = 0; b < 2; b++) {
                m.n_open[b] = b == 0 || k + 1 < n_mats ? m.cols : 0;  // at g zeta: all but the quotient
                m.off_open[b] = o; o += 2 * m.n_open[b];
                batch_cols[b] += m.n_open[b];
            }
            m.q_leaf = q; q += m.cols;
            m.q_sib = q; q += 4 * d0;
        }
        off_fri_caps = o; o += L * 4 * ncap;
        off_queries = o;
        layer_depth.clear();
        size_t lg = log_N;
        for (size_t l = 0; l < L; l++) {
            lg -= arity_bits;
            size_t d = lg - cap_h;
            layer_depth.push_back(d);
            q += 2 * ((size_t)1 << arity_bits) + 4 * d;
        }
        query_words = q;
        o += n_queries * query_words;
        off_final = o; o += 2 * final_len;
        off_pow = o; o += 1;
        off_pis = o; o += n_pis;
        off_sums = o; o += nC / 2;
        total = o;
    }
    void write_header(uint64_t* h) const {
        h[0] = STARKHIP_PROOF_MAGIC; h[1] = C; h[2] = Q; h[3] = log_n; h[4] = rate_bits; h[5] = cap_h; h[6] = L;
        h[7] = n_queries; h[8] = final_len; h[9] = n_pis; h[10] = arity_bits; h[11] = n_challenges;
        h[12] = hasher;
        h[13] = nZ;
        h[14] = nA;
        h[15] = nC;
    }
    bool read_header(const uint64_t* h, size_t words) {
        if (words < 16 || h[0] != STARKHIP_PROOF_MAGIC) return false;
        C = h[1]; Q = h[2]; log_n = h[3]; rate_bits = h[4]; cap_h = h[5]; L = h[6]; n_queries = h[7]; final_len = h[8];
        n_pis = h[9]; arity_bits = h[10]; n_challenges = h[11]; hasher = h[12]; nZ = h[13]; nA = h[14]; nC = h[15];
        if (hasher > STARKHIP_HASHER_KECCAK || nZ > 128 || nA > STARKHIP_AIR_MAX_LOGUP_POLYS || (nZ && nA)) return false;
        if ((nC & 3) || nC > STARKHIP_AIR_MAX_LOGUP_POLYS || nA + nC > STARKHIP_AIR_MAX_LOGUP_POLYS || (nZ && nC)) return false;
        if (log_n > 32 || rate_bits > 8 || cap_h > 16 || L > 16 || arity_bits > 8 || log_n + rate_bits < cap_h) return false;
        if (L * arity_bits + cap_h > log_n + rate_bits) return false;
        compute();
        return total == words;
    }
};

}  // namespace starkhip
