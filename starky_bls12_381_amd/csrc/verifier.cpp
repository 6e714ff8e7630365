// CPU verifier: the counterpart of starky::verifier::verify_stark_proof, which the reference calls
// right after every prove (/root/reference/src/aggregate_proof.rs:67,113,146,177).  Written from the
// verifier's equations, i.e. an independent code path from the prover: it
// re-derives every Fiat-Shamir challenge, checks the quotient identity at zeta with an extension-field
// evaluation of the AIR, and runs the FRI query checks.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "air_eval.h"
#include "airs.h"
#include "ctl.h"
#include "logup.h"
#include "permutation.h"
#include "poseidon.h"
#include "proof.h"
#include "verifier.h"

namespace starkhip {

// under the proof's hasher; a Keccak sibling whose words are outside a digest's ranges (COMPAT.md K6) fails the path
static bool merkle_verify_to_cap(size_t hasher, const gl_t* leaf, size_t leaf_len, size_t index, const gl_t* cap, const gl_t* siblings, size_t depth) {
    const bool keccak = hasher == STARKHIP_HASHER_KECCAK;
    gl_t cur[4];
    if (keccak) keccak_hash_or_noop(leaf, leaf_len, 1, cur);
    else poseidon_hash_or_noop(leaf, leaf_len, 1, cur);
    for (size_t d = 0; d < depth; d++) {
        gl_t nxt[4];
        const gl_t* sib = siblings + 4 * d;
        if (keccak) {
            if (!keccak_digest_in_range(sib)) return false;
            if (index & 1) keccak_two_to_one(sib, cur, nxt);
            else keccak_two_to_one(cur, sib, nxt);
        } else if (index & 1) poseidon_two_to_one(sib, cur, nxt);
        else poseidon_two_to_one(cur, sib, nxt);
        memcpy(cur, nxt, sizeof cur);
        index >>= 1;
    }
    return memcmp(cur, cap + 4 * index, sizeof cur) == 0;
}

static gl2_t eval_poly_ext(const gl2_t* coeffs, size_t n, gl2_t x) {
    gl2_t acc = gl2_zero();
    for (size_t i = n; i-- > 0;) acc = gl2_add(gl2_mul(acc, x), coeffs[i]);
    return acc;
}

// plonky2 fri::verifier::compute_evaluation: interpolate the arity coset values and evaluate at beta.
static gl2_t fri_fold_eval(gl_t x, size_t x_index_within_coset, unsigned arity_bits, const gl2_t* evals_in, gl2_t beta) {
    size_t arity = (size_t)1 << arity_bits;
    gl_t g = gl_root_of_unity(arity_bits);
    std::vector<gl2_t> evals(arity);
    for (size_t i = 0; i < arity; i++) evals[gl_bitrev((uint32_t)i, arity_bits)] = evals_in[i];
    size_t rev = gl_bitrev((uint32_t)x_index_within_coset, arity_bits);
    gl_t coset_start = gl_mul(x, gl_pow(g, arity - rev));
    std::vector<gl_t> pts(arity);
    gl_t y = 1;
    for (size_t i = 0; i < arity; i++) {
        pts[i] = gl_mul(coset_start, y);
        y = gl_mul(y, g);
    }
    // Lagrange interpolation at beta
    gl2_t res = gl2_zero();
    for (size_t i = 0; i < arity; i++) {
        gl2_t num = gl2_one();
        gl_t den = 1;
        for (size_t j = 0; j < arity; j++) {
            if (j == i) continue;
            num = gl2_mul(num, gl2_sub(beta, gl2_from_base(pts[j])));
            den = gl_mul(den, gl_sub(pts[i], pts[j]));
        }
        res = gl2_add(res, gl2_mul(evals[i], gl2_mul_base(num, gl_inv(den))));
    }
    return res;
}

int verify_prelude(const AirInfo& air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words, bool check_query_words,
                   VerifyPrelude* out, const CtlVerify* ctl) {
    ProofLayout& pl = out->pl;
    if (!pl.read_header(proof, words)) return STARKHIP_ERR_BAD_SHAPE;
    const AirProgram& P = air.prog;
    FriGeometry& geo = out->geo;
    if (!FriGeometry::make(cfg, (unsigned)pl.log_n, &geo) || quotient_degree_bits(P.degree) > cfg.rate_bits) return STARKHIP_ERR_BAD_SHAPE;
    const unsigned factor = quotient_factor(P.degree);
    if (pl.C != P.n_cols || pl.n_pis != P.n_pis || pl.rate_bits != cfg.rate_bits || pl.cap_h != cfg.cap_height ||
        pl.n_queries != cfg.num_query_rounds || pl.n_challenges != cfg.num_challenges || pl.Q != (size_t)factor * cfg.num_challenges ||
        pl.arity_bits != cfg.arity_bits || pl.nZ != P.perm_zs() || pl.nA != P.logup_polys() ||
        pl.nC != (ctl ? ctl->table->polys() : 0))  // (a table proof of a system on its own: its header names CTL polynomials, nobody here knows its endpoints)
        return STARKHIP_ERR_BAD_SHAPE;
    const size_t skip_lo = check_query_words ? words : pl.off_queries, skip_hi = check_query_words ? words : pl.off_final;
    for (size_t i = 16; i < skip_lo; i++)
        if (proof[i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    for (size_t i = skip_hi; i < words; i++)
        if (proof[i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    if (geo.arities.size() != pl.L || geo.final_poly_len != pl.final_len) return STARKHIP_ERR_BAD_SHAPE;
    if (pl.hasher == STARKHIP_HASHER_KECCAK) {  // K6: a cap entry outside a digest's ranges is not the encoding of any 25 bytes
        for (size_t k = 0; k < pl.n_mats; k++)
            for (size_t i = 0; i < pl.ncap; i++)
                if (!keccak_digest_in_range(proof + pl.mat[k].off_cap + 4 * i)) return STARKHIP_ERR_VERIFY;
        for (size_t i = 0; i < pl.L * pl.ncap; i++)
            if (!keccak_digest_in_range(proof + pl.off_fri_caps + 4 * i)) return STARKHIP_ERR_VERIFY;
    }

    const size_t n = (size_t)1 << pl.log_n, N = (size_t)1 << pl.log_N, ncap = pl.ncap, nZ = pl.nZ, last = pl.n_mats - 1;
    // the openings of matrix k at zeta (batch 0) or at g zeta (batch 1), pl.mat[k].n_open[batch] of them
    auto opened = [&](size_t k, int batch) { return (const gl2_t*)(proof + pl.mat[k].off_open[batch]); };
    const gl2_t *op_local = opened(0, 0), *op_next = opened(0, 1), *op_q = opened(last, 0);
    const gl2_t* final_poly = (const gl2_t*)(proof + pl.off_final);
    const gl_t* pis = proof + pl.off_pis;

    // ---- challenges, in transcript order (App. A.5)
    Challenger ch((int)pl.hasher);  // the hasher the header names: the sponge's permutation, and proof of work through it
    if (ctl) {  // C2: the table's transcript is a copy of the system's, which has observed every table's trace cap
        if (ctl->initial->hasher != (int)pl.hasher) return STARKHIP_ERR_VERIFY;
        ch = *ctl->initial;
    } else {
        ch.observe_many(proof + pl.mat[0].off_cap, 4 * ncap);
    }
    // permutation challenges (COMPAT.md P1): B sets of 2 x (beta, gamma) after the trace cap, then the Z cap (P3), then the alphas
    std::vector<gl_t> perm_chal(nZ ? (size_t)P.perm_batch_size() * 4 : 0);
    for (gl_t& x : perm_chal) x = ch.get();
    // LogUp challenges (COMPAT.md L1): chi_0, chi_1 in the same place, then the auxiliary cap (L3)
    gl_t logup_chal[2] = {0, 0};
    if (pl.nA)
        for (gl_t& x : logup_chal) x = ch.get();
    for (size_t k = 1; k < last; k++) ch.observe_many(proof + pl.mat[k].off_cap, 4 * ncap);
    ch.observe_many(proof + pl.off_sums, pl.nC / 2);  // C2: the table's sums, behind the cap of LogUp || CTL
    std::vector<gl2_t> alphas(cfg.num_challenges);
    for (auto& a : alphas) a = gl2_from_base(ch.get());
    ch.observe_many(proof + pl.mat[last].off_cap, 4 * ncap);
    gl2_t zeta = ch.get_ext();
    for (int batch = 0; batch < 2; batch++)  // P5: local || zs || quotient, then next || zs_next
        for (size_t k = 0; k < pl.n_mats; k++)
            for (size_t i = 0; i < pl.mat[k].n_open[batch]; i++) ch.observe_ext(opened(k, batch)[i]);
    gl2_t fri_alpha = ch.get_ext();
    std::vector<gl2_t>& betas = out->betas;
    betas.resize(pl.L);
    for (size_t l = 0; l < pl.L; l++) {
        ch.observe_many(proof + pl.off_fri_caps + l * 4 * ncap, 4 * ncap);
        betas[l] = ch.get_ext();
    }
    for (size_t k = 0; k < pl.final_len; k++) ch.observe_ext(final_poly[k]);
    ch.observe(proof[pl.off_pow]);
    gl_t pow_response = ch.get();
    if (cfg.proof_of_work_bits > 0 && (pow_response >> (64 - cfg.proof_of_work_bits)) != 0) return STARKHIP_ERR_VERIFY;
    std::vector<size_t>& indices = out->indices;
    indices.resize(pl.n_queries);
    for (auto& x : indices) x = (size_t)(ch.get() % N);

    // ---- quotient identity at zeta
    gl_t g = gl_root_of_unity((unsigned)pl.log_n);
    gl2_t zeta_n = gl2_pow(zeta, n);
    gl2_t z_h = gl2_sub(zeta_n, gl2_one());
    gl2_t masks[4];
    masks[KIND_PLAIN] = gl2_one();
    masks[KIND_TRANSITION] = gl2_sub(zeta, gl2_from_base(gl_inv(g)));
    masks[KIND_FIRST] = gl2_mul(z_h, gl2_inv(gl2_mul_base(gl2_sub(zeta, gl2_one()), (gl_t)n)));
    masks[KIND_LAST] = gl2_mul(z_h, gl2_inv(gl2_mul_base(gl2_sub(gl2_mul_base(zeta, g), gl2_one()), (gl_t)n)));
    std::vector<gl2_t> acc(cfg.num_challenges);
    air_eval_folded<ExtOps>(P, op_local, op_next, pis, masks, alphas.data(), (int)cfg.num_challenges, acc.data());
    if (nZ) perm_eval_folded<ExtOps>(P, op_local, opened(1, 0), opened(1, 1), perm_chal.data(), masks, alphas.data(), (int)cfg.num_challenges, acc.data());  // P4
    if (pl.nA) logup_eval_folded<ExtOps>(P, op_local, op_next, opened(1, 0), opened(1, 1), logup_chal, masks, alphas.data(), (int)cfg.num_challenges, acc.data());  // L4
    if (pl.nC)  // C4, with the sums taken from the proof
        ctl_eval_folded<ExtOps>(*ctl->table, op_local, op_next, opened(1, 0) + pl.nA, opened(1, 1) + pl.nA, ctl->challenges, proof + pl.off_sums, masks, alphas.data(),
                                (int)cfg.num_challenges, acc.data());
    for (unsigned i = 0; i < cfg.num_challenges; i++) {
        gl2_t s = gl2_zero();
        for (unsigned k = factor; k-- > 0;) s = gl2_add(gl2_mul(s, zeta_n), op_q[i * factor + k]);
        if (!gl2_eq(acc[i], gl2_mul(z_h, s))) return STARKHIP_ERR_VERIFY;
    }

    // ---- what the FRI queries take from here
    out->zeta = zeta;
    out->gzeta = gl2_mul_base(zeta, g);
    out->fri_alpha = fri_alpha;
    // precomputed reduced openings per batch: sum_j alpha^j open_j
    out->red[0] = out->red[1] = gl2_zero();
    for (int batch = 0; batch < 2; batch++)
        for (size_t k = pl.n_mats; k-- > 0;)
            for (size_t i = pl.mat[k].n_open[batch]; i-- > 0;) out->red[batch] = gl2_add(gl2_mul(out->red[batch], fri_alpha), opened(k, batch)[i]);
    out->alpha_pow_C = gl2_pow(fri_alpha, pl.batch_cols[1]);  // alpha^{|batch 1|}
    return STARKHIP_OK;
}

int verify_proof(const AirInfo& air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words) { return verify_proof(air, cfg, proof, words, nullptr); }

int verify_proof(const AirInfo& air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words, const CtlVerify* ctl) {
    VerifyPrelude pre;
    if (int rc = verify_prelude(air, cfg, proof, words, true, &pre, ctl); rc != STARKHIP_OK) return rc;
    const ProofLayout& pl = pre.pl;
    const FriGeometry& geo = pre.geo;
    const size_t ncap = pl.ncap;
    const gl2_t fri_alpha = pre.fri_alpha, zeta = pre.zeta, gzeta = pre.gzeta, red0 = pre.red[0], red1 = pre.red[1], alpha_pow_C = pre.alpha_pow_C;
    const std::vector<gl2_t>& betas = pre.betas;
    const std::vector<size_t>& indices = pre.indices;
    const gl2_t* final_poly = (const gl2_t*)(proof + pl.off_final);

    // The 84 query rounds are independent and dominated by re-hashing a trace leaf each (FinalExp: 9191 permutations per
    // leaf, 0.8 M in all -- about a second on one core), so they are checked by a few host threads.
    const size_t d0 = pl.log_N - pl.cap_h;
    auto check_query = [&](size_t qi) -> bool {
        const uint64_t* qp = proof + pl.off_queries + qi * pl.query_words;
        size_t x_index = indices[qi];
        gl_t subgroup_x = gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity((unsigned)pl.log_N), gl_bitrev((uint32_t)x_index, (unsigned)pl.log_N)));
        // every matrix's leaf (P6: trace, zs, quotient) against its cap, and into fri_combine_initial's sums: batch 0, and batch 1 if it is opened at g zeta
        gl2_t e0 = gl2_zero(), e1 = gl2_zero();
        for (size_t k = pl.n_mats; k-- > 0;) {
            const MatrixLayout& m = pl.mat[k];
            if (!merkle_verify_to_cap(pl.hasher, qp + m.q_leaf, m.cols, x_index, proof + m.off_cap, qp + m.q_sib, d0)) return false;
            for (size_t i = m.n_open[0]; i-- > 0;) e0 = gl2_add(gl2_mul(e0, fri_alpha), gl2_from_base(qp[m.q_leaf + i]));
            for (size_t i = m.n_open[1]; i-- > 0;) e1 = gl2_add(gl2_mul(e1, fri_alpha), gl2_from_base(qp[m.q_leaf + i]));
        }
        qp += pl.quotient().q_sib + 4 * d0;
        gl2_t xe = gl2_from_base(subgroup_x);
        gl2_t sum = gl2_mul(gl2_sub(e0, red0), gl2_inv(gl2_sub(xe, zeta)));
        sum = gl2_add(gl2_mul(sum, alpha_pow_C), gl2_mul(gl2_sub(e1, red1), gl2_inv(gl2_sub(xe, gzeta))));
        gl2_t old_eval = sum;
        for (size_t l = 0; l < pl.L; l++) {
            unsigned ab = geo.arities[l];
            size_t arity = (size_t)1 << ab;
            const gl2_t* evals = (const gl2_t*)qp; qp += 2 * arity;
            const gl_t* sib = qp; qp += 4 * pl.layer_depth[l];
            size_t coset_index = x_index >> ab, within = x_index & (arity - 1);
            if (!gl2_eq(evals[within], old_eval)) return false;
            old_eval = fri_fold_eval(subgroup_x, within, ab, evals, betas[l]);
            if (!merkle_verify_to_cap(pl.hasher, (const gl_t*)evals, 2 * arity, coset_index, proof + pl.off_fri_caps + l * 4 * ncap, sib, pl.layer_depth[l]))
                return false;
            for (unsigned b = 0; b < ab; b++) subgroup_x = gl_sqr(subgroup_x);
            x_index = coset_index;
        }
        if (!gl2_eq(eval_poly_ext(final_poly, pl.final_len, gl2_from_base(subgroup_x)), old_eval)) return false;
        return true;
    };
    const size_t n_threads = std::min<size_t>(std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency())), pl.n_queries);
    std::atomic<bool> ok(true);
    std::atomic<size_t> next(0);
    auto worker = [&]() {
        for (size_t qi; ok.load(std::memory_order_relaxed) && (qi = next.fetch_add(1)) < pl.n_queries;)
            if (!check_query(qi)) ok.store(false);
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_threads; t++) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    if (!ok.load()) return STARKHIP_ERR_VERIFY;
    return STARKHIP_OK;
}

}  // namespace starkhip
