// Kernel-level entry points: single kernels, or a transform as prove() dispatches it, on data of the caller's.  NOT on the proving
// path -- only the tests and the micro-benchmarks call them (starkhip_lde_batch, starkhip_ntt_long, starkhip_lde_bench,
// starkhip_expand_log, starkhip_merkle_cap, starkhip_permute_batch(_form), starkhip_field_ops, starkhip_host_alloc / _free).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "ctl.h"
#include "ctx.h"
#include "kernels_ctl.h"
#include "kernels_logup.h"
#include "kernels_permutation.h"
#include "logup.h"
#include "permutation.h"

namespace starkhip {

// kernel-level test entry: the Z polynomials of `air` on the caller's trace as prove() computes them -- the pair columns gathered into
// the copy prove() keeps aside, then launch_perm_zs.  The caller has checked the trace argument, the rows and the challenges.
int permutation_zs(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* challenges, uint64_t* zs_out, uint64_t* closing_out) {
    const AirProgram& P = air.prog;
    const size_t n = in.n_rows, C = in.n_cols, nZ = P.perm_zs(), B = P.perm_batch_size();
    HIPCHK(hipSetDevice(c->device));
    const std::vector<uint32_t> cols = perm_columns(P), desc = perm_descriptor(P, true);
    Ctx::PermBufs& pb = c->perm;
    HIPCHK(c->values.ensure(C * n * 8));
    HIPCHK(c->lde.ensure(C * n * 8));  // upload_dense stages host rows there
    HIPCHK(pb.cols.ensure(cols.size() * n * 8));
    HIPCHK(pb.desc.ensure(desc.size() * 4));
    HIPCHK(pb.chal.ensure(B * 4 * 8));
    HIPCHK(pb.zvals.ensure(nZ * n * 8));
    HIPCHK(pb.scan.ensure((perm_scratch_words(n, (unsigned)nZ) + nZ) * 8));
    const gl_t* d_values = nullptr;
    if (int rc = upload_dense(c, in, c->values.as<gl_t>(), &d_values)) return rc;
    for (size_t k = 0; k < cols.size(); k++)
        HIPCHK(hipMemcpyAsync(pb.cols.as<gl_t>() + k * n, d_values + (size_t)cols[k] * n, n * 8, hipMemcpyDeviceToDevice, c->st));
    HIPCHK(hipMemcpyAsync(pb.desc.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(pb.chal.p, challenges, B * 4 * 8, hipMemcpyHostToDevice, c->st));
    gl_t* const d_closing = pb.scan.as<gl_t>() + perm_scratch_words(n, (unsigned)nZ);
    HIPCHK(launch_perm_zs(pb.desc.as<uint32_t>(), pb.cols.as<gl_t>(), n, pb.chal.as<gl_t>(), n, (unsigned)nZ, pb.zvals.as<gl_t>(), pb.scan.as<gl_t>(), d_closing, c->st));
    HIPCHK(hipMemcpyAsync(zs_out, pb.zvals.p, nZ * n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(closing_out, d_closing, nZ * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

// kernel-level test entry: the auxiliary polynomials of `air` on the caller's trace as prove() computes them -- the named columns gathered
// into the copy prove() keeps aside (the slots of the pairs' buffers: Ctx::PermBufs), then launch_logup_polys.  The caller has checked
// the trace argument, the rows and the challenges.
int logup_polys(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* challenges, uint64_t* polys_out, uint64_t* closing_out, uint64_t* zero_denominators_out) {
    const AirProgram& P = air.prog;
    const size_t n = in.n_rows, C = in.n_cols, nA = P.logup_polys();
    const unsigned nzs = 2 * (unsigned)P.logups.size();
    HIPCHK(hipSetDevice(c->device));
    const std::vector<uint32_t> cols = logup_columns(P);
    const bool general = logup_use_general(P);
    std::vector<uint32_t> desc = logup_descriptor(P, true, general);
    const size_t desc_words = desc.size();
    const std::vector<uint32_t> zp = logup_z_polys(P);
    desc.insert(desc.end(), zp.begin(), zp.end());
    Ctx::PermBufs& pb = c->perm;
    HIPCHK(c->values.ensure(C * n * 8));
    HIPCHK(c->lde.ensure(C * n * 8));  // upload_dense stages host rows there
    HIPCHK(pb.cols.ensure(cols.size() * n * 8));
    HIPCHK(pb.desc.ensure(desc.size() * 4));
    HIPCHK(pb.zvals.ensure(nA * n * 8));
    HIPCHK(pb.scan.ensure((logup_scratch_words(n, nzs) + logup_result_words(nzs)) * 8));
    const gl_t* d_values = nullptr;
    if (int rc = upload_dense(c, in, c->values.as<gl_t>(), &d_values)) return rc;
    for (size_t k = 0; k < cols.size(); k++)
        HIPCHK(hipMemcpyAsync(pb.cols.as<gl_t>() + k * n, d_values + (size_t)cols[k] * n, n * 8, hipMemcpyDeviceToDevice, c->st));
    HIPCHK(hipMemcpyAsync(pb.desc.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, c->st));
    gl_t* const d_results = pb.scan.as<gl_t>() + logup_scratch_words(n, nzs);
    HIPCHK(launch_logup_polys(pb.desc.as<uint32_t>(), general, pb.desc.as<uint32_t>() + desc_words, pb.cols.as<gl_t>(), n, challenges[0], challenges[1], n, nzs,
                              pb.zvals.as<gl_t>(), pb.scan.as<gl_t>(), d_results, c->st));
    std::vector<gl_t> results(logup_result_words(nzs));
    HIPCHK(hipMemcpyAsync(polys_out, pb.zvals.p, nA * n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(results.data(), d_results, results.size() * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    std::copy(results.begin(), results.begin() + nzs, closing_out);
    *zero_denominators_out = results[nzs];
    return STARKHIP_OK;
}

// kernel-level test entry: the CTL polynomials of one table of a system on the caller's trace as the system prover computes them -- the
// named columns gathered into the copy kept aside, then launch_ctl_polys (no LogUp polynomials in front).  The caller has checked the
// trace argument, the rows and the challenges.
int ctl_polys(Ctx* c, const CtlTable& T, const TraceInput& in, const uint64_t* challenges, uint64_t* polys_out, uint64_t* sums_out, uint64_t* zero_denominators_out) {
    const size_t n = in.n_rows, C = in.n_cols;
    const unsigned E = (unsigned)T.eps.size();
    HIPCHK(hipSetDevice(c->device));
    const std::vector<uint32_t> cols = ctl_columns(T);
    std::vector<uint32_t> desc = ctl_descriptor(T, true);
    const size_t desc_words = desc.size();
    const std::vector<uint32_t> zp = ctl_z_polys(T, 0);
    desc.insert(desc.end(), zp.begin(), zp.end());
    Ctx::PermBufs& pb = c->perm;
    HIPCHK(c->values.ensure(C * n * 8));
    HIPCHK(c->lde.ensure(C * n * 8));  // upload_dense stages host rows there
    HIPCHK(pb.cols.ensure(cols.size() * n * 8));
    HIPCHK(pb.desc.ensure(desc.size() * 4));
    HIPCHK(pb.zvals.ensure(T.polys() * n * 8));
    HIPCHK(pb.scan.ensure((ctl_scratch_words(n, E) + ctl_result_words(E)) * 8));
    const gl_t* d_values = nullptr;
    if (int rc = upload_dense(c, in, c->values.as<gl_t>(), &d_values)) return rc;
    for (size_t k = 0; k < cols.size(); k++)
        HIPCHK(hipMemcpyAsync(pb.cols.as<gl_t>() + k * n, d_values + (size_t)cols[k] * n, n * 8, hipMemcpyDeviceToDevice, c->st));
    HIPCHK(hipMemcpyAsync(pb.desc.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, c->st));
    gl_t* const d_results = pb.scan.as<gl_t>() + ctl_scratch_words(n, E);
    HIPCHK(launch_ctl_polys(pb.desc.as<uint32_t>(), pb.desc.as<uint32_t>() + desc_words, pb.cols.as<gl_t>(), n, CtlChallenges{challenges[0], challenges[1], challenges[2], challenges[3]},
                            n, E, pb.zvals.as<gl_t>(), 0, pb.scan.as<gl_t>(), d_results, c->st));
    std::vector<gl_t> results(ctl_result_words(E));
    HIPCHK(hipMemcpyAsync(polys_out, pb.zvals.p, T.polys() * n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(results.data(), d_results, results.size() * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    std::copy(results.begin(), results.begin() + 2 * E, sums_out);
    *zero_denominators_out = 0;
    for (unsigned e = 0; e < E; e++) *zero_denominators_out += results[2 * E + e];  // (counted per endpoint)
    return STARKHIP_OK;
}

int lde_batch(Ctx* c, const uint64_t* values, size_t n_cols, unsigned log_n, unsigned rate_bits, uint64_t* coeffs_out, uint64_t* lde_out) {
    if (log_n < 1 || log_n > STARKHIP_MAX_LOG_ROWS || rate_bits > 8) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_tables(c, log_n, rate_bits, 0))) return rc;
    const size_t n = (size_t)1 << log_n, N = n << rate_bits;
    HIPCHK(c->values.ensure(n_cols * n * 8));
    HIPCHK(c->lde.ensure(n_cols * N * 8));
    HIPCHK(hipMemcpyAsync(c->values.p, values, n_cols * n * 8, hipMemcpyHostToDevice, c->st));
    // the LDE comes from the kernel prove() uses for this shape: for 8192 rows the wave-resident one, which keeps no coefficients --
    // those, when asked for, come from the other kernel afterwards (in place of the values, which the first run leaves untouched)
    const bool wave = lde_wave_supported(log_n) && c->opt_lde_impl == 0;
    // as in prove(): the kernels count the columns e_c for the leaf hash's saved prefix state (kernels.h: LeafPrefix), from zero for
    // each run over the columns -- what starkhip_leaf_hash_lane_group's prefix_mask then reads.  Whatever n_cols: with fewer than n + 8
    // columns it is the leaf kernels that must not skip.
    const bool prefix = leaf_prefix_wanted(c, n + 8, log_n, rate_bits);
    if (prefix && (rc = ensure_leaf_prefix(c, log_n, rate_bits))) return rc;
    unsigned* const unit_count = prefix ? leaf_prefix_counter(c) : nullptr;
    std::vector<gl_t> tmp;
    if (wave) {
        HIPCHK(leaf_prefix_reset(c));
        HIPCHK(run_lde(c, c->values.as<gl_t>(), nullptr, c->lde.as<gl_t>(), n_cols, log_n, rate_bits, 0, 0, unit_count));
        if (lde_out) {
            tmp.resize(n_cols * N);
            HIPCHK(hipMemcpyAsync(tmp.data(), c->lde.p, n_cols * N * 8, hipMemcpyDeviceToHost, c->st));
            HIPCHK(stream_wait(c));
        }
    }
    if (!wave || coeffs_out) {
        HIPCHK(leaf_prefix_reset(c));
        HIPCHK(run_lde(c, c->values.as<gl_t>(), c->values.as<gl_t>(), c->lde.as<gl_t>(), n_cols, log_n, rate_bits, 0, 0, unit_count));
    }
    if (coeffs_out) HIPCHK(hipMemcpyAsync(coeffs_out, c->values.p, n_cols * n * 8, hipMemcpyDeviceToHost, c->st));  // in place
    HIPCHK(stream_wait(c));
    if (lde_out) {
        // device layout is coset-major; hand back NATURAL point order i = k * R + s
        if (!wave) {
            tmp.resize(n_cols * N);
            HIPCHK(hipMemcpy(tmp.data(), c->lde.p, n_cols * N * 8, hipMemcpyDeviceToHost));
        }
        const size_t R = (size_t)1 << rate_bits;
        for (size_t col = 0; col < n_cols; col++)
            for (size_t s = 0; s < R; s++)
                for (size_t k = 0; k < n; k++) lde_out[col * N + k * R + s] = tmp[col * N + s * n + k];
    }
    return STARKHIP_OK;
}

// kernel-level test entry: n_vecs vectors of 2^log_len words (2^16 .. 2^26) through the multi-workgroup transform as prove() runs it on
// the quotient's values and the FRI layers -- in place, forward or inverse (with 2^-log_len)
int ntt_long(Ctx* c, uint64_t* data, size_t n_vecs, unsigned log_len, int inverse) {
    if (!long_vector(log_len) || !n_vecs || !data) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = ensure_tables(c, 1, 0, 0)) return rc;  // (the long tables are cached with a shape's)
    const size_t words = n_vecs << log_len;
    HIPCHK(c->values.ensure(words * 8));
    HIPCHK(c->lde.ensure(words * 8));
    HIPCHK(hipMemcpyAsync(c->values.p, data, words * 8, hipMemcpyHostToDevice, c->st));
    if (int rc = run_ntt(c, c->values.as<gl_t>(), c->lde.as<gl_t>(), n_vecs, (size_t)1 << log_len, log_len, inverse != 0, nullptr, nullptr)) return rc;
    HIPCHK(hipMemcpyAsync(data, c->values.p, words * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

// micro-benchmark entry: the trace LDE of `n_cols` synthetic columns (powers of a generator: no constant or unit column, so every
// column is transformed unless const_per_64 says otherwise), `reps` launches timed with HIP events on the context's stream; average milliseconds per launch
int lde_bench(Ctx* c, size_t n_cols, unsigned log_n, unsigned rate_bits, unsigned reps, unsigned const_per_64, const uint64_t* device_values, float* ms_out, float* each_ms) {
    if (log_n < 1 || log_n > STARKHIP_MAX_LOG_ROWS || rate_bits > 8 || !n_cols) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_tables(c, log_n, rate_bits, 0))) return rc;
    const size_t n = (size_t)1 << log_n, N = n << rate_bits;
    const bool long_cols = lde_long_supported(log_n);
    HIPCHK(c->values.ensure(n_cols * n * 8 * (long_cols ? 2 : 1)));  // long columns: + the coefficients the transform keeps, beside the input
    HIPCHK(c->lde.ensure(n_cols * N * 8));
    const gl_t* in = device_values ? (const gl_t*)device_values : c->values.as<gl_t>();  // the caller's own column-major matrix, or the synthetic one
    gl_t* const cf = long_cols ? c->values.as<gl_t>() + n_cols * n : nullptr;
    if (device_values) const_per_64 = 0;
    else HIPCHK(launch_fill_powers(c->values.as<gl_t>(), 3, GL_GENERATOR, n_cols * n, c->st));
    // `const_per_64` of every 64 columns constant (a FinalExp trace: 11 of 64 take a closed form), in runs of up to 12 as its Fp12 blocks are
    // (+ 256: unit vectors instead -- one 1 per column, at a different row each -- the other closed form: FinalExp's 8192 row selectors)
    const bool unit = (const_per_64 & 256u) != 0, prewarm = (const_per_64 & 1024u) != 0, touch = (const_per_64 & 2048u) != 0;  // + 1024 / + 2048 (with reps == 0): see below
    const_per_64 &= 255u;
    for (size_t c0 = 0; const_per_64 && c0 < n_cols; c0 += 64) {
        const size_t cnt = std::min<size_t>(const_per_64, n_cols - c0);
        HIPCHK(hipMemsetAsync(c->values.as<gl_t>() + c0 * n, unit ? 0 : 1, cnt * n * 8, c->st));
        for (size_t k = 0; unit && k < cnt; k++) HIPCHK(hipMemsetAsync(c->values.as<gl_t>() + (c0 + k) * n + ((c0 + k) * 37) % n, 1, 1, c->st));
    }
    const bool cold = reps == 0;  // reps == 0: ONE launch with no warm-up launch in front of it
    if (cold) reps = 1;
    reps = std::min(reps, 16u);
    std::vector<hipEvent_t> ev(reps + 1, nullptr);
    hipError_t err = hipSuccess;
    for (hipEvent_t& e : ev)
        if (err == hipSuccess) err = hipEventCreate(&e);
    if (err == hipSuccess && cold && touch) err = hipMemsetAsync(c->lde.p, 0, n_cols * N * 8, c->st);  // every page of the output written once just before
    if (err == hipSuccess && cold && prewarm)  // a few milliseconds of the same arithmetic on a small footprint, then the launch that is timed
        for (int k = 0; k < 4 && err == hipSuccess; k++) err = run_lde(c, in, cf, c->lde.as<gl_t>(), std::min<size_t>(n_cols, 4096), log_n, rate_bits, 0);
    if (err == hipSuccess) err = cold ? hipStreamSynchronize(c->st) : run_lde(c, in, cf, c->lde.as<gl_t>(), n_cols, log_n, rate_bits, 0);  // warm-up
    if (err == hipSuccess) err = hipEventRecord(ev[0], c->st);
    for (unsigned r = 0; r < reps && err == hipSuccess; r++) {
        err = run_lde(c, in, cf, c->lde.as<gl_t>(), n_cols, log_n, rate_bits, 0);
        if (err == hipSuccess) err = hipEventRecord(ev[r + 1], c->st);
    }
    if (err == hipSuccess) err = hipEventSynchronize(ev[reps]);
    float ms = 0;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev[0], ev[reps]);
    for (unsigned r = 0; r < reps && err == hipSuccess && each_ms; r++) err = hipEventElapsedTime(&each_ms[r], ev[r], ev[r + 1]);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    HIPCHK(err);
    *ms_out = ms / reps;
    return STARKHIP_OK;
}

// kernel-level test entry: a recorded trace through expand_trace_kernel + zero_cells_kernel, handed back column-major [C][rows]
int expand_log(Ctx* c, const TraceLog* log, uint64_t* out_colmajor) {
    HIPCHK(hipSetDevice(c->device));
    const size_t nw = log->total_words(), nr = log->total_records(), nz = log->total_late_zeros();
    std::vector<uint32_t> h(nw + nr + nz);
    for (const LogPiece& pc : recording_pieces(*log)) std::copy(pc.src, pc.src + pc.words, h.begin() + pc.at);
    const size_t cells = log->rows * log->cols;
    HIPCHK(c->values.ensure(cells * 8));
    HIPCHK(c->staging.ensure(std::max<size_t>(h.size(), 1) * 4));
    uint32_t* d = c->staging.as<uint32_t>();
    if (!h.empty()) HIPCHK(hipMemcpyAsync(d, h.data(), h.size() * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemsetAsync(c->values.p, 0, cells * 8, c->st));
    if (nr) HIPCHK(launch_expand_trace(d, d + nw, nr, c->values.as<gl_t>(), log->rows, c->st));
    if (nz) HIPCHK(launch_zero_cells(d + nw + nr, nz / 2, c->values.as<gl_t>(), log->rows, c->st));
    HIPCHK(hipMemcpyAsync(out_colmajor, c->values.p, cells * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

int merkle_cap(Ctx* c, const uint64_t* lde_natural, size_t n_cols, unsigned log_N, unsigned cap_h, uint64_t* cap_out) {
    if (log_N < cap_h) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    const size_t N = (size_t)1 << log_N;
    // treat the input as rate_bits = 0 (coset-major == natural)
    HIPCHK(c->lde.ensure(n_cols * N * 8));
    HIPCHK(c->digests.ensure(digest_words(N) * 8));
    HIPCHK(hipMemcpyAsync(c->lde.p, lde_natural, n_cols * N * 8, hipMemcpyHostToDevice, c->st));
    int form;
    HIPCHK(launch_leaf_hash_lone(c, c->lde.as<gl_t>(), n_cols, log_N, 0, c->digests.as<gl_t>(), c->st, &form));
    HIPCHK(launch_merkle_levels(c->digests.as<gl_t>(), log_N, cap_h, c->st));
    HIPCHK(hipMemcpyAsync(cap_out, c->digests.as<gl_t>() + 4 * level_off(N, log_N - cap_h), ((size_t)4 << cap_h) * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

int permute_batch(Ctx* c, uint64_t* states, size_t n) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->staging.ensure(n * 12 * 8));
    HIPCHK(hipMemcpyAsync(c->staging.p, states, n * 96, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_permute_batch(c->staging.as<gl_t>(), n, c->st));
    HIPCHK(hipMemcpyAsync(states, c->staging.p, n * 96, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

// the Keccak hasher's challenger permutation (keccak.h: K7) on whole states
int keccak_permute_batch(Ctx* c, uint64_t* states, size_t n) {
    if (n == 0) return STARKHIP_OK;
    if (!states) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->staging.ensure(n * 96));
    HIPCHK(hipMemcpyAsync(c->staging.p, states, n * 96, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_permute_batch_keccak(c->staging.as<gl_t>(), n, c->st));
    HIPCHK(hipMemcpyAsync(states, c->staging.p, n * 96, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

// merkle_cap under either hasher, with the leaf digests: hasher 0 takes the leaf-hash form a lone proof would, hasher 1 the Keccak kernel
int merkle_tree_hasher(Ctx* c, int hasher, const uint64_t* lde_natural, size_t n_cols, unsigned log_N, unsigned cap_h, uint64_t* digests_out, uint64_t* cap_out) {
    if (hasher < STARKHIP_HASHER_POSEIDON || hasher > STARKHIP_HASHER_KECCAK || !lde_natural || !cap_out || !n_cols || log_N < cap_h || log_N > 28)
        return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    const size_t N = (size_t)1 << log_N;
    HIPCHK(c->lde.ensure(n_cols * N * 8));  // rate_bits = 0: coset-major == natural
    HIPCHK(c->digests.ensure(digest_words(N) * 8));
    HIPCHK(hipMemcpyAsync(c->lde.p, lde_natural, n_cols * N * 8, hipMemcpyHostToDevice, c->st));
    int form;
    if (hasher == STARKHIP_HASHER_KECCAK) HIPCHK(launch_leaf_hash_keccak(c->lde.as<gl_t>(), n_cols, log_N, 0, c->digests.as<gl_t>(), c->st));
    else HIPCHK(launch_leaf_hash_lone(c, c->lde.as<gl_t>(), n_cols, log_N, 0, c->digests.as<gl_t>(), c->st, &form));
    HIPCHK(launch_merkle_levels_by(hasher, c->digests.as<gl_t>(), log_N, cap_h, c->st));
    if (digests_out) HIPCHK(hipMemcpyAsync(digests_out, c->digests.p, 4 * N * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(cap_out, c->digests.as<gl_t>() + 4 * level_off(N, log_N - cap_h), ((size_t)4 << cap_h) * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

int hash_rows_hasher(Ctx* c, int hasher, const uint64_t* rows, size_t width, size_t n_leaves, uint64_t* digests_out) {
    if (hasher < STARKHIP_HASHER_POSEIDON || hasher > STARKHIP_HASHER_KECCAK || !rows || !digests_out || !width || !n_leaves || width > ((size_t)1 << 24) ||
        n_leaves > ((size_t)1 << 28))
        return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->staging.ensure((width + 4) * n_leaves * 8));
    gl_t* d_rows = c->staging.as<gl_t>();
    gl_t* d_dig = d_rows + width * n_leaves;
    HIPCHK(hipMemcpyAsync(d_rows, rows, width * n_leaves * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_leaf_hash_rows_by(hasher, d_rows, width, n_leaves, d_dig, c->st));
    HIPCHK(hipMemcpyAsync(digests_out, d_dig, 4 * n_leaves * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

// the permutation of one leaf-hash form on whole states (kernels_hash.hip: the test entry points); a bad form or variant launches nothing
int permute_batch_form(Ctx* c, int form, int variant, uint64_t* states, size_t n) {
    if (variant < 0 || (unsigned)variant >= permute_form_variants(form)) return STARKHIP_ERR_BAD_SHAPE;
    if (n == 0) return STARKHIP_OK;
    if (!states) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->staging.ensure(2 * n * 96));
    gl_t* in = c->staging.as<gl_t>();
    HIPCHK(hipMemcpyAsync(in, states, n * 96, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_permute_batch_form(form, variant, in, in + 12 * n, n, c->st));
    HIPCHK(hipMemcpyAsync(states, in + 12 * n, n * 96, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

// the lane-form leaf hash on 1 .. 4 matrices of one shape: the pool's grouped launch (one grid) or the per-commitment launches -- those
// also in the pair form.  prefix_mask bit s: segment s is given the context's saved prefix state for this shape and the counter as the
// last starkhip_lde_batch of this shape left it (kernels.h: LeafPrefix); the other segments get null pointers.
int leaf_hash_lane_group(Ctx* c, const uint64_t* mats, size_t n_segments, size_t n_cols, unsigned log_n, unsigned rate_bits, int grouped, int form,
                         unsigned prefix_mask, uint64_t* digests_out) {
    if (!mats || !digests_out || n_segments == 0 || n_segments > 4 || n_cols == 0 || log_n + rate_bits > 20 || n_cols > ((size_t)1 << 20)) return STARKHIP_ERR_BAD_SHAPE;
    if ((form != FORM_LANE && form != FORM_PAIR) || (grouped && form != FORM_LANE) || (prefix_mask >> n_segments) != 0) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    LeafPrefix pf;
    // (whatever n_cols, as in lde_batch; with "leaf_hash_prefix" = 0, or for a shape without the table, every segment gets null pointers)
    if (prefix_mask && leaf_prefix_wanted(c, ((size_t)1 << log_n) + 8, log_n, rate_bits)) {
        if (int rc = ensure_tables(c, log_n, rate_bits, 0)) return rc;
        if (int rc = ensure_leaf_prefix(c, log_n, rate_bits)) return rc;
        pf = leaf_prefix(c);
    }
    const size_t N = (size_t)1 << (log_n + rate_bits), mat_words = n_cols * N, dig_words = 4 * N;
    HIPCHK(c->staging.ensure(n_segments * (mat_words + dig_words) * 8));
    gl_t* d_mats = c->staging.as<gl_t>();
    gl_t* d_dig = d_mats + n_segments * mat_words;
    HIPCHK(hipMemcpyAsync(d_mats, mats, n_segments * mat_words * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemsetAsync(d_dig, 0xEE, n_segments * dig_words * 8, c->st));  // a digest that is not written does not come back as a field element
    LeafHashBatch B = {};
    for (size_t s = 0; s < n_segments; s++) {
        B.mat[s] = d_mats + s * mat_words;
        B.digests[s] = d_dig + s * dig_words;
        if (prefix_mask >> s & 1u) {
            B.prefix_count[s] = pf.count;
            B.prefix_cap[s] = pf.cap;
        }
    }
    if (grouped) {
        HIPCHK(launch_leaf_hash_lane_group(B, (unsigned)n_segments, n_cols, log_n, rate_bits, c->st));
    } else {
        for (size_t s = 0; s < n_segments; s++) HIPCHK(launch_leaf_hash_form((LeafHashForm)form, B.mat[s], n_cols, log_n, rate_bits, B.digests[s], c->st, LeafPrefix{B.prefix_count[s], B.prefix_cap[s]}));
    }
    HIPCHK(hipMemcpyAsync(digests_out, d_dig, n_segments * dig_words * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

int leaf_prefix_table(Ctx* c, unsigned log_n, unsigned rate_bits, uint64_t* cap_out) {
    if (!cap_out || log_n > STARKHIP_MAX_LOG_ROWS || rate_bits > 8 || !leaf_prefix_wanted(c, ((size_t)1 << log_n) + 8, log_n, rate_bits)) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = ensure_tables(c, log_n, rate_bits, 0)) return rc;
    if (int rc = ensure_leaf_prefix(c, log_n, rate_bits)) return rc;
    HIPCHK(hipMemcpyAsync(cap_out, c->tab->leaf_prefix.p, leaf_prefix_words(log_n, rate_bits) * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

int field_ops(Ctx* c, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->staging.ensure(3 * n * 8));
    gl_t* d = c->staging.as<gl_t>();
    HIPCHK(hipMemcpyAsync(d, a, n * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(d + n, b, n * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_field_ops(op, d, d + n, d + 2 * n, n, c->st));
    HIPCHK(hipMemcpyAsync(out, d + 2 * n, n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

int host_alloc(Ctx* c, size_t bytes, void** out) {
    if (bytes == 0) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return STARKHIP_ERR_OOM;
    }
    HIPCHK(e);
    *out = p;
    return STARKHIP_OK;
}

void host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

}  // namespace starkhip
