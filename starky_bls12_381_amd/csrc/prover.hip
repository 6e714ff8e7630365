// Host driver of the GPU prover: the MI355X-native replacement of starky::prover::prove as called at
// /root/reference/src/aggregate_proof.rs:59-65 (and :105, :138, :169).  prove() follows the transcript of SURVEY.md App. A.5 as a list
// of phases (the methods of ProveCall), sized and laid out by one ProofShape and one table of work buffers that ctx_reserve() shares;
// every heavy step is one of the kernels in kernels_*.hip, the host only runs the Fiat-Shamir challenger, two length-n synthetic
// divisions and the proof assembly.  What a proof commits is a list of matrices in proof order (ProveCall::mats beside ProofLayout::mat): the trace, the Zs of an
// AIR with permutation pairs (COMPAT.md P1 - P8; made and committed at the start of the quotient phase, ProveCall::permutation) or the auxiliary polynomials of one with LogUp lookups (L1 - L7; ProveCall::logup, in the same place and the same buffers), the quotient.  Below prove(): the pool's reservation.  The context and its caches are ctx.h / ctx.hip, the trace
// checkers' host halves check_trace.hip and permutation_check.hip, the kernel-level entry points of the tests kernel_entries.hip.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>

#include "airs.h"
#include "blob_arena.h"
#include "check_report.h"
#include "ctl.h"
#include "ctx.h"
#include "kernels.h"
#include "kernels_ctl.h"
#include "kernels_logup.h"
#include "kernels_permutation.h"
#include "lde_ranges.h"
#include "logup.h"
#include "logup_frequencies.h"
#include "permutation.h"
#include "trace_log.h"
#include "poseidon.h"
#include "proof.h"
#include "quotient_ops.h"
#include "quotient_plan.h"
#include "prover.h"
#include "scheduler.h"

#ifdef STARKHIP_ROCTX  // make ROCTX=1: phase ranges for rocprofv3 --marker-trace; the default build has no profiler-SDK dependency
#include <rocprofiler-sdk-roctx/roctx.h>
#endif

namespace starkhip {

// One open rocTX range at a time on the calling thread; closed on every way out of prove().  Without STARKHIP_ROCTX: nothing.
struct PhaseRanges {
#ifdef STARKHIP_ROCTX
    bool open = false;
    void next(const char* name) {
        if (open) roctxRangePop();
        roctxRangePushA(name);
        open = true;
    }
    ~PhaseRanges() {
        if (open) roctxRangePop();
    }
#else
    void next(const char*) {}
#endif
};

// The LDE of a trace whose columns are parked in the buffer the LDE goes to, as its last C n words (in_place).  lde_ranges.h has the
// launch plan and why it is safe: launches over 3/4, 3/16, 3/64 of the columns for R = 4, each overwriting only columns an earlier
// launch has transformed, and the last lde_tail_columns(C) columns -- 1/64 of them, 75 MB for FinalExp -- from a copy (`tail`).  Carried
// to the end the series would be log_R(C) launches, the last of them a few columns wide and each as long as one column takes; four
// launches cost 0.07 ms of 17.5 against one (same box, alternating builds).
// unit_count (or null): the word in which the launches count the columns e_c, each launch from the absolute index of its first column
// (kernels.h: LeafPrefix); every column is transformed by exactly one launch.
static hipError_t run_lde_trace(Ctx* c, const gl_t* values, gl_t* lde, gl_t* tail, size_t C, unsigned log_n, unsigned rate, bool in_place, unsigned* unit_count) {
    if (!in_place) return run_lde(c, values, nullptr, lde, C, log_n, rate, 0, 0, unit_count);
    const size_t n = (size_t)1 << log_n, R = (size_t)1 << rate;
    for (const LdeLaunch& l : lde_launch_plan(C, rate)) {
        const gl_t* in = values + l.a * n;
        if (l.from_copy) {
            if (hipError_t e = hipMemcpyAsync(tail, in, (l.b - l.a) * n * 8, hipMemcpyDeviceToDevice, c->st); e != hipSuccess) return e;
            in = tail;
        }
        if (hipError_t e = run_lde(c, in, nullptr, lde + l.a * R * n, l.b - l.a, log_n, rate, 0, (unsigned)l.a, unit_count); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// (F(X) - F(z)) / (X - z), padded with one zero coefficient back to length n (plonky2 divide_by_linear + push(0))
static void divide_by_linear(const gl2_t* F, size_t n, gl2_t z, gl2_t* q) {
    gl2_t carry = gl2_zero();
    q[n - 1] = gl2_zero();
    for (size_t k = n; k-- > 1;) {
        carry = gl2_add(F[k], gl2_mul(carry, z));
        q[k - 1] = carry;
    }
}

namespace {
struct HostWatch {  // accumulates wall time of the host-side stretches of prove()
    double ms = 0;
    std::chrono::steady_clock::time_point t0;
    void start() { t0 = std::chrono::steady_clock::now(); }
    void stop() { ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// The dimensions of one proof, derived in one place: prove() and ctx_reserve() size and lay out everything from these.
struct ProofShape {
    unsigned log_n, r, cap_h, log_N, qdb, factor;  // log2 of rows, blow-up, cap size, LDE points; the quotient's degree bits and factor
    size_t n, N, C, Q, size, ncap, L;              // rows, LDE points, trace and quotient columns, quotient points (n << qdb), cap nodes, FRI layers
    size_t nZ, perm_cols, perm_desc_words;         // permutation pairs: Z polynomials, the columns the pairs name, words of one descriptor (0 without pairs)
    size_t nA, nLZ;                                // LogUp lookups: auxiliary polynomials and, of them, the Zs (2 per lookup); perm_cols and perm_desc_words are then theirs
    size_t nC, nE, ctl_cols, ctl_desc_words;       // a table of a system: its CTL polynomials (4 per endpoint), its endpoints, the columns they name, words of one CTL descriptor
    size_t mid;                                    // the middle matrix's polynomials: nZ, or nA + nC (LogUp || CTL), 0 without any
    bool logup_general;                            // LogUp lookups over Columns and Filters (or the general kernels forced): the form of the descriptors
    FriGeometry geo;
    ProofLayout pl;
    // STARKHIP_ERR_BAD_SHAPE for what prove() refuses: rows that are no power of two in 2 .. 2^max_log_rows(air), a config that the one
    // config rule (FriGeometry::make) refuses or whose blow-up is below the AIR's quotient degree
    static int make(const AirInfo& air, const starkhip_config_t& cfg, size_t n_rows, ProofShape* s, const CtlTable* ctl = nullptr) {
        const AirProgram& P = air.prog;
        unsigned log_n = 0;
        if (!log2_rows(n_rows, &log_n) || cfg.num_challenges != 2 || log_n > max_log_rows(air)) return STARKHIP_ERR_BAD_SHAPE;
        if (!FriGeometry::make(cfg, log_n, &s->geo) || quotient_degree_bits(P.degree) > cfg.rate_bits) return STARKHIP_ERR_BAD_SHAPE;
        s->log_n = log_n; s->r = cfg.rate_bits; s->cap_h = cfg.cap_height; s->log_N = log_n + s->r;
        s->qdb = quotient_degree_bits(P.degree); s->factor = quotient_factor(P.degree);
        s->n = n_rows; s->N = s->n << s->r; s->C = P.n_cols; s->Q = (size_t)s->factor * 2; s->size = s->n << s->qdb;
        s->ncap = (size_t)1 << s->cap_h; s->L = s->geo.arities.size();
        s->nZ = P.perm_zs(); s->perm_cols = s->nZ ? perm_columns(P).size() : 0; s->perm_desc_words = s->nZ ? perm_descriptor(P, false).size() : 0;
        s->nA = P.logup_polys(); s->nLZ = 2 * P.logups.size(); s->logup_general = false;
        if (s->nA) { s->perm_cols = logup_columns(P).size(); s->logup_general = logup_use_general(P); s->perm_desc_words = logup_descriptor(P, false, s->logup_general).size(); }
        s->nE = ctl ? ctl->eps.size() : 0; s->nC = 4 * s->nE; s->ctl_cols = s->nE ? ctl_columns(*ctl).size() : 0; s->ctl_desc_words = s->nE ? ctl_descriptor(*ctl, false).size() : 0;
        if (s->nC && (s->nZ || s->nA + s->nC > STARKHIP_AIR_MAX_LOGUP_POLYS || P.degree < 2)) return STARKHIP_ERR_BAD_SHAPE;  // (a registered system never has such a table)
        s->mid = s->nZ + s->nA + s->nC;
        s->pl = ProofLayout::make(P, cfg, s->geo, log_n, 0, s->nC);
        return STARKHIP_OK;
    }
};

// fri_combine_kernel sums the columns of a matrix in chunks of this many, one partial sum per chunk (comb_partial)
static const size_t COMB_PPC = 256;
static size_t comb_chunks(size_t C) { return (C + COMB_PPC - 1) / COMB_PPC; }

// THE size of every work buffer of a proof of shape `s` whose quotient is evaluated in `n_chunks` chunks -- by class (`plan` non-null and
// by_class) in plan->n_work rows of one coset each, recombined from 2 plan->n_vecs vectors of n words (and as many of scratch).  prove() and ctx_reserve()
// both allocate from this list, so a context that a pool has warmed never grows a buffer inside a proof (see ctx_reserve).  What the
// two do not share is theirs to say: `values_bytes` (a whole trace, the tail of run_lde_trace, or nothing) and `park_bytes`, what
// the upload stages at the start of the LDE buffer.
struct BufWant { DevBuf* b; size_t bytes; };
// fill_lookups: the proof fills `n_lookups` lookups first (lookup_fill_in_prove), in batches whose buffers are listed here too.
// fill_freq: the program whose LogUp frequencies the proof fills first (logup_fill_in_prove), or null: likewise.
static std::vector<BufWant> work_buffers(Ctx* c, const ProofShape& s, unsigned n_chunks, const Ctx::PlanDev* plan, size_t values_bytes, size_t park_bytes,
                                         size_t fill_lookups, const AirProgram* fill_freq) {
    const size_t n = s.n, N = s.N, C = s.C, Q = s.Q, size = s.size, nq = s.pl.n_queries;
    const bool by_class = plan && plan->by_class;
    const size_t partial_words = by_class ? std::max<size_t>((size_t)plan->n_work * plan->n_classes * 2 * n, 2 * size) : (size_t)n_chunks * 2 * size;
    std::vector<BufWant> w = {
        {&c->values, values_bytes}, {&c->lde, std::max(C * N * 8, park_bytes)}, {&c->digests, digest_words(N) * 8},
        {&c->pis, std::max<size_t>(1, s.pl.n_pis) * 8}, {&c->apow, 2 * (AIR_MAX_GROUP + 1) * 8}, {&c->chunk_scale, 2 * (size_t)n_chunks * 8},
        {&c->partial, partial_words * 8}, {&c->qclass, by_class ? (size_t)plan->n_vecs * 2 * 2 * n * 8 : 0}, {&c->qvals, 2 * size * 8}, {&c->qcoef, Q * n * 8}, {&c->qlde, Q * N * 8},
        {&c->qdigests, digest_words(N) * 8},
        {&c->zpow, 2 * n * 16},  // powers of zeta (the quotient polynomials' openings), then the coset-0 weights of zeta
        {&c->gzpow, n * 16},     // the weights of g zeta
        {&c->open_local, C * 16}, {&c->open_next, C * 16}, {&c->open_q, Q * 16}, {&c->ext_apow, s.pl.batch_cols[0] * 16},
        {&c->comb_partial, (comb_chunks(C) + comb_chunks(s.mid)) * n * 16},  // (the middle matrix's sum: one more chunk for the Zs, up to four for LogUp)
        {&c->comb_out, 2 * n * 16}, {&c->fri_coef, 2 * N * 8}, {&c->fri_vals, 2 * N * 8},
        {&c->scale_tab, N * 8}, {&c->pow_state, 12 * 8}, {&c->pow_best, 8}, {&c->qidx, nq * 4},
        {&c->gather_t, nq * s.pl.query_words * 8},  // every query round's leaves and Merkle paths, in proof layout
        // the leaf hash's saved state past an identity prefix and its counter, kept with the shape's tables (ctx.h); 0 where this proof cannot use it
        {&c->tab->leaf_prefix, leaf_prefix_bytes(c, C, s.log_n, s.r)}};
    if (const size_t nZ = s.mid) {  // an AIR with permutation pairs or with LogUp lookups: the middle matrix (Ctx::PermBufs)
        Ctx::PermBufs& pb = c->perm;
        // (a table of a system: the CTL columns behind the LogUp ones, the two CTL descriptors and the Zs' indices behind LogUp's, the scan's
        // scratch shared -- the CTL polynomials are done before logup() starts --, and in `chal` the CTL sums and the count of zero denominators)
        const size_t scan_words = s.nA + s.nC ? std::max(logup_scratch_words(n, (unsigned)s.nLZ) + logup_result_words((unsigned)s.nLZ), ctl_scratch_words(n, (unsigned)s.nE))
                                              : perm_scratch_words(n, (unsigned)nZ) + nZ;
        for (const BufWant& b : {BufWant{&pb.cols, (s.perm_cols + s.ctl_cols) * n * 8}, BufWant{&pb.desc, (2 * s.perm_desc_words + s.nLZ + 2 * s.ctl_desc_words + 2 * s.nE) * 4},
                                 BufWant{&pb.chal, std::max(4 * (size_t)s.factor, ctl_result_words((unsigned)s.nE)) * 8},
                                 BufWant{&pb.zvals, nZ * n * 8}, BufWant{&pb.zcoef, lde_long_supported(s.log_n) ? nZ * n * 8 : 0}, BufWant{&pb.zlde, nZ * N * 8},
                                 BufWant{&pb.zdigests, digest_words(N) * 8}, BufWant{&pb.scan, scan_words * 8},
                                 BufWant{&pb.open_z, nZ * 16}, BufWant{&pb.open_zn, nZ * 16}})
            w.push_back(b);
    }
    if (fill_lookups)  // "fill_lookups" on an AIR registered with its lookups (Ctx::LookupBufs and the sorted items of a batch)
        for (const LookupWant& b : lookup_work_buffers(c, n, fill_lookups, false)) w.push_back({b.b, b.bytes});
    if (fill_freq)  // "fill_frequencies" on a fillable AIR with LogUp lookups (Ctx::LogupFreqBufs and the sorted tables of a batch)
        for (const LookupWant& b : logup_freq_work_buffers(c, *fill_freq, n, false)) w.push_back({b.b, b.bytes});
    size_t len = N;
    for (size_t l = 0; l < s.L; l++) {  // a FRI layer's leaves and digests stay on the device for the query phase
        w.push_back({&c->fri_rows[l], len * 2 * 8});
        len >>= s.geo.arities[l];
        w.push_back({&c->fri_digests[l], digest_words(len) * 8});
    }
    return w;
}

// `values` of a proof: the columns the last LDE launch of a parked trace reads (run_lde_trace), a whole trace, or -- a short trace read
// from the caller's own columns -- nothing.  A long trace always has a whole trace of words there: its coefficients (run_lde).
static size_t values_bytes_for(const ProofShape& s, bool trace_in_lde, bool callers_columns) {
    if (lde_long_supported(s.log_n)) return s.C * s.n * 8;
    return trace_in_lde ? lde_tail_columns(s.C) * s.n * 8 : callers_columns ? 0 : s.C * s.n * 8;
}

// The long transform's tables for every length a proof of shape `s` transforms: the trace and quotient columns (n), the quotient's
// values (n << qdb), the combined polynomial (n) and the FRI layers
static int ensure_long_tables(Ctx* c, const ProofShape& s) {
    std::vector<unsigned> logs = {s.log_n, s.log_n + s.qdb};
    unsigned log_len = s.log_N;
    for (size_t l = 0; l < s.L; l++) {
        logs.push_back(log_len);
        log_len -= s.geo.arities[l];
    }
    for (unsigned lg : logs)
        if (lg == s.log_n ? lde_long_supported(lg) : long_vector(lg))
            if (int rc = ensure_long_tw(c, lg, nullptr)) return rc;
    return 0;
}

// What one prove() call carries from phase to phase, and the phases: named like the entries of starkhip_last_timings and the rocTX
// ranges, run by prove() in that order.  Each enqueues its work on the context's stream; where the host needs a result it requests a
// read-back that the NEXT phase's first stream_wait completes -- prove() records the phase boundary in between -- so the host vectors
// those land in live here.  A vector that one phase alone fills and reads is local to it, in front of the stream_wait that lets it go.
struct ProveCall {
    Ctx* c;
    const AirInfo& air;
    const starkhip_config_t& cfg;
    const ProofShape& s;
    hipStream_t st;
    const TraceInput& in;  // prove()'s arguments
    const uint64_t* pis_host;
    uint64_t pow_witness;
    bool tiled;          // the quotient's evaluator: the tiled plan, or the op-stream interpreter
    unsigned n_chunks;   // ... and the chunks its constraints are cut into
    bool trace_in_lde;   // the trace waits for the LDE inside the LDE buffer, as its last C n words (run_lde_trace)
    bool fill;           // "fill_lookups" and an AIR registered with its lookups: upload() fills their permuted columns in the prover's own copy
    bool fill_freq;      // "fill_frequencies" and a fillable AIR with LogUp lookups: upload() fills their frequencies columns likewise
    bool prefix;         // the LDE counts the columns e_c and the trace commitment may start from the saved state past them (kernels.h: LeafPrefix)
    gl_t* d_trace;       // where the upload puts the trace, column-major
    const gl_t* d_values = nullptr;  // where it is: d_trace, or the caller's own device memory
    Challenger ch;
    HostWatch fs, host_other;  // Fiat-Shamir hashing / other host arithmetic of this proof
    // The committed matrix that s.pl.mat[k] lays out (trace, Zs of an AIR with pairs or auxiliary polynomials of one with LogUp lookups, quotient): the context's own buffers (ctx.h),
    // only pointed at, and the host vectors its cap's and its openings' read-backs land in.  (Without Zs the third record is unused.)
    struct Committed {
        DevBuf *lde, *digests;  // its LDE, column-major, and the Merkle tree over its bit-reversed rows
        DevBuf* d_open[2];      // where the openings at zeta / at g zeta are computed
        DevBuf* coef;           // null: opened from coset 0 of the LDE (trace, Zs); else from these coefficients (quotient)
        std::vector<gl_t> cap;
        std::vector<gl2_t> open[2];
    } mats[3] = {{&c->lde, &c->digests, {&c->open_local, &c->open_next}},
                 s.mid ? Committed{&c->perm.zlde, &c->perm.zdigests, {&c->perm.open_z, &c->perm.open_zn}} : Committed{&c->qlde, &c->qdigests, {&c->open_q}, &c->qcoef},
                 {&c->qlde, &c->qdigests, {&c->open_q}, &c->qcoef}};
    std::vector<gl_t> quot_tail, fri_caps;
    std::vector<gl2_t> final_poly;
    // an AIR with permutation pairs: the challenges (B sets of 2 x {beta, gamma}), the two descriptors back to back (by copy slot, by trace column;
    // for LogUp lookups theirs, followed by the Zs' polynomial indices)
    std::vector<gl_t> perm_chal;
    std::vector<uint32_t> perm_desc;
    int permutation();
    gl_t logup_chal[2] = {0, 0};  // an AIR with LogUp lookups: chi_0, chi_1
    int logup();
    // A table of a system (COMPAT.md 2d): its endpoints (null: a proof on its own), the challenger after the system transcript, which the
    // table's transcript starts from instead of observing its own trace cap (C2), the CTL challenges, the table's sums (challenge-major)
    // and how many denominators were zero.  ctl_polys() runs between the two halves of the proof; aux_commit() commits LogUp || CTL.
    const CtlTable* ctl = nullptr;
    const Challenger* ch_initial = nullptr;
    CtlChallenges ctl_chal = {0, 0, 0, 0};
    std::vector<gl_t> ctl_sums;
    std::vector<uint64_t> ctl_zero_denominators;  // per endpoint, both challenges together
    size_t ctl_desc_at() const { return 2 * s.perm_desc_words + s.nLZ; }  // where the CTL descriptors start in perm.desc: by slot, the Zs' indices, by trace column
    int ctl_polys(const gl_t chal[4]);
    int aux_commit();
    gl_t alphas[2] = {0, 0};
    gl2_t zeta = gl2_zero();
    uint64_t* out = nullptr;  // the proof blob, from queries() on -- or the check blob of a trace that upload() refused
    size_t check_words = 0;   // ... and that blob's length
    int upload(), ifft_lde(), trace_merkle(), quotient(), quotient_commit(), openings(), fri_combine(), fri_commit(), pow(), queries();
    int upload_recording(const TraceLog* log), upload_column_table(const uint64_t* const* cols), leaf_hash_on_host();
    int run_quotient_tiles(unsigned debug_mode, gl_t* qvals_out, bool timed), run_quotient_ops(), compare_quotient_evaluators();
    int run_quotient_classes(), commit_cap(Committed& m), commit_narrow(Committed& m, size_t cols);
};

// The end of a commitment, above leaf digests the caller has enqueued: the Merkle levels under the context's hasher, and the cap's
// read-back requested -- the caller's (or the next phase's) stream_wait completes it
int ProveCall::commit_cap(Committed& m) {
    HIPCHK(launch_merkle_levels_by((int)c->opt_hasher, m.digests->as<gl_t>(), s.log_N, s.cap_h, st));
    m.cap.resize(4 * s.ncap);
    HIPCHK(read_back(c, m.cap.data(), m.digests->as<gl_t>() + 4 * level_off(s.N, s.log_N - s.cap_h), 4 * s.ncap * 8, st));
    return 0;
}
// A matrix of a few columns (the Zs, the quotient) from its LDE: the leaves under Keccak or in the quad form, then the above
int ProveCall::commit_narrow(Committed& m, size_t cols) {
    if (c->opt_hasher == STARKHIP_HASHER_KECCAK) HIPCHK(launch_leaf_hash_keccak(m.lde->as<gl_t>(), cols, s.log_n, s.r, m.digests->as<gl_t>(), st));
    else HIPCHK(launch_leaf_hash_form(FORM_QUAD, m.lde->as<gl_t>(), cols, s.log_n, s.r, m.digests->as<gl_t>(), st));
    return commit_cap(m);
}

// ---- phase 0: trace into column-major device memory (trace_rows_to_poly_values), by layout
// compact trace: upload the generator's write log and expand it here
int ProveCall::upload_recording(const TraceLog* log) {
    const size_t n = s.n, C = s.C;
    const size_t nw = log->total_words(), nr = log->total_records(), nz = log->total_late_zeros();
    if (log->rows != n || log->cols != C) return STARKHIP_ERR_BAD_SHAPE;
    uint32_t* d_words = c->lde.as<uint32_t>();  // the recording's words wait at the start of the (still unused) LDE buffer
    uint32_t* d_offsets = d_words + nw;
    uint32_t* d_zeros = d_offsets + nr;
    HIPCHK(hipMemsetAsync(d_trace, 0, C * n * 8, st));
    // The parts (recording_pieces) are gathered into ONE page-locked staging buffer of the context and go up as ONE copy: a FinalExp
    // recording has 53 parts x 3 arrays, and on a GPU that other proofs keep busy every one of 160 dependent stream operations waits
    // its turn (measured: 0.9 - 1.6 s of "upload" for a proof whose copies queued behind other proofs' commitments, against 6 ms alone).
    const size_t total = nw + nr + nz;
    HIPCHK(ensure_host_staging(c, total * 4, total * 4 + total));  // + 25 %: the next recording of this AIR is about as long
    uint32_t* h = (uint32_t*)c->host_staging;
    const std::vector<LogPiece> pieces = recording_pieces(*log);
    // 150 MB for FinalExp: gathered on a few threads (10 ms on one), pieces dealt round-robin
    const unsigned n_thr = total * 4 > ((size_t)32 << 20) ? 4 : 1;
    run_on_helpers(n_thr, [&](unsigned w) {
        for (size_t i = w; i < pieces.size(); i += n_thr) memcpy(h + pieces[i].at, pieces[i].src, pieces[i].words * 4);
    });
    if (total) HIPCHK(hipMemcpyAsync(d_words, h, total * 4, hipMemcpyHostToDevice, st));
    if (nr) HIPCHK(launch_expand_trace(d_words, d_offsets, nr, d_trace, n, st));
    if (nz) HIPCHK(launch_zero_cells(d_zeros, nz / 2, d_trace, n, st));
    d_values = d_trace;
    return 0;
}

// The literal argument of starky's prove(): `Vec<PolynomialValues<F>>`, one heap allocation per column
// (/root/reference/src/aggregate_proof.rs:168-175) -- `cols` is a table of C column pointers.  C separate pageable copies of 64 KB would
// each be staged by the runtime (73 527 of them for FinalExp); instead host threads gather runs of columns into the two halves of
// the context's page-locked staging and every half goes up as one copy, the gather of the next half under the copy of this one.
// Column-major device memory is just the columns back to back.
int ProveCall::upload_column_table(const uint64_t* const* cols) {
    const size_t n = s.n, C = s.C, col_bytes = n * 8;
    HIPCHK(ensure_host_staging(c, std::max<size_t>(2 * col_bytes, (size_t)32 << 20), std::max<size_t>(2 * col_bytes, (size_t)128 << 20)));
    for (auto& e : c->col_ev)
        if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventBlockingSync));
    const size_t half_bytes = c->host_staging_cap / 2, per_half = std::max<size_t>(1, half_bytes / col_bytes);
    bool used[2] = {false, false};
    unsigned h = 0;
    for (size_t c0 = 0; c0 < C; c0 += per_half, h ^= 1) {
        const size_t cnt = std::min(per_half, C - c0);
        char* dst = (char*)c->host_staging + (size_t)h * half_bytes;
        if (used[h]) HIPCHK(event_wait_sleeping(c->col_ev[h]));  // the copy that last read this half has run
        const unsigned n_thr = cnt * col_bytes > ((size_t)8 << 20) ? 4 : 1;
        run_on_helpers(n_thr, [&](unsigned w) {
            for (size_t i = w; i < cnt; i += n_thr) memcpy(dst + i * col_bytes, cols[c0 + i], col_bytes);
        });
        HIPCHK(hipMemcpyAsync(d_trace + c0 * n, dst, cnt * col_bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(c->col_ev[h], st));
        used[h] = true;
    }
    d_values = d_trace;
    return 0;
}

int ProveCall::upload() {
    int rc;
    switch (in.form) {
        case TraceForm::Recording: rc = upload_recording(in.log); break;
        case TraceForm::ColumnTable: rc = upload_column_table(in.columns); break;
        default: rc = upload_dense(c, in, d_trace, &d_values);
    }
    // "fill_lookups": the permuted columns of the AIR's lookups, written into the prover's own copy before anything reads them -- the
    // check below and the copy of the pair columns, from which the Zs are built.  Column-major device memory of the caller's, which
    // is otherwise read where it lies, is copied first: the caller's buffer is only read.  A lookup that fails ends the proof here
    // with STARKHIP_ERR_TRACE and the lookup blob in `out`.
    if (rc == 0 && (fill || fill_freq)) {
        if (in.callers_columns()) {
            HIPCHK(hipMemcpyAsync(d_trace, in.words, s.C * s.n * 8, hipMemcpyDeviceToDevice, st));
            d_values = d_trace;
        }
        if (fill) rc = lookup_fill_in_prove(c, air, d_trace, s.n, &out, &check_words);
        // "fill_frequencies": the frequencies columns of the AIR's LogUp lookups, at the same place and under the same terms; a
        // lookup that fails hands back the LogUp blob
        if (rc == 0 && fill_freq) rc = logup_fill_in_prove(c, air, d_trace, s.n, &out, &check_words);
    }
    // "check_trace": every constraint on every row of the trace where the upload has just put it, before anything of the LDE is
    // enqueued; a violating trace ends the proof here with STARKHIP_ERR_TRACE and its check blob in `out`
    if (rc == 0 && c->opt_check_trace) rc = check_trace_in_prove(c, air, d_values, s.n, pis_host, &out, &check_words);
    if (rc == 0 && s.mid) {  // the columns the permutation pairs (or the LogUp lookups) name, aside: the LDE overwrites a parked trace and keeps no coefficients of it
        const std::vector<uint32_t> cols = s.nA ? logup_columns(air.prog) : s.nZ ? perm_columns(air.prog) : std::vector<uint32_t>();
        for (size_t k = 0; k < cols.size(); k++)
            HIPCHK(hipMemcpyAsync(c->perm.cols.as<gl_t>() + k * s.n, d_values + (size_t)cols[k] * s.n, s.n * 8, hipMemcpyDeviceToDevice, st));
        if (s.nC) {  // ... and the columns the table's CTL endpoints name, behind them
            const std::vector<uint32_t> more = ctl_columns(*ctl);
            for (size_t k = 0; k < more.size(); k++)
                HIPCHK(hipMemcpyAsync(c->perm.cols.as<gl_t>() + (cols.size() + k) * s.n, d_values + (size_t)more[k] * s.n, s.n * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    return rc;
}

// ---- phase 1: IFFT + LDE (PolynomialBatch::from_values, App. A.3)
int ProveCall::ifft_lde() {
    HIPCHK(hipEventRecord(c->kev[4], st));
    if (lde_long_supported(s.log_n)) HIPCHK(run_lde(c, d_values, c->values.as<gl_t>(), c->lde.as<gl_t>(), s.C, s.log_n, s.r, 0));  // coefficients into `values`
    else {
        HIPCHK(leaf_prefix_reset(c));  // whatever an earlier proof of this shape counted
        HIPCHK(run_lde_trace(c, d_values, c->lde.as<gl_t>(), c->values.as<gl_t>(), s.C, s.log_n, s.r, trace_in_lde, prefix ? leaf_prefix_counter(c) : nullptr));
    }
    HIPCHK(hipEventRecord(c->kev[5], st));
    return 0;
}

// A commitment of a few leaves is a latency chain on the GPU whatever the form: FP12Mul (16 rows at blow-up 2) has 32 leaves of
// 7 536 sequential permutations -- 42 ms in the row form at 5.6 us per permutation on eight waves of a chip that holds 4 096.
// The host permutation the challenger uses runs at 0.8 us, and 32 independent leaves spread over the process's CPUs: the LDE
// (15 MB) comes down, host threads hash the leaves, the digests go back up and the tree is built on the device as usual.
// Same function, same bytes (tests/test_gpu_airs.py: FP12Mul against the oracle).
int ProveCall::leaf_hash_on_host() {
    const size_t n = s.n, N = s.N, C = s.C;
    const unsigned r = s.r, log_N = s.log_N;
    if (c->hs && !HashService::is_big(s.log_n, r)) {  // a pooled proof was announced to the scheduler's window: it is not coming
        c->hs->abandon_small();
        c->hash_requested = true;
    }
    c->hash_timing.form = SENT_HOST;
    c->hash_timing.group = 1;
    c->host_lde.resize(C * N);
    HIPCHK(hipMemcpyAsync(c->host_lde.data(), c->lde.p, C * N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(c));
    std::vector<gl_t> leaf_digests(4 * N);
    const gl_t* lde_h = c->host_lde.data();
    const unsigned n_thr = (unsigned)std::min<size_t>(N, std::max(1u, cpu_budget()));
    run_on_helpers(n_thr, [&](unsigned w) {
        for (size_t j = w; j < N; j += n_thr) {
            size_t i = 0;  // leaf j holds the LDE row of natural point index bitrev(j) = k * R + s, stored coset-major at [s][k]
            for (unsigned b = 0; b < log_N; b++) i |= ((j >> b) & 1) << (log_N - 1 - b);
            const size_t s_ = i & (((size_t)1 << r) - 1), k_ = i >> r;
            gl_t state[12] = {0};
            const gl_t* col = lde_h + s_ * n + k_;
            for (size_t off = 0; off < C; off += 8) {
                const size_t cnt = std::min<size_t>(8, C - off);
                for (size_t e = 0; e < cnt; e++) state[e] = col[(off + e) * N];
                poseidon_permute_host(state);
            }
            for (int e = 0; e < 4; e++) leaf_digests[4 * j + e] = state[e];
        }
    });
    HIPCHK(hipMemcpyAsync(c->digests.p, leaf_digests.data(), 4 * N * 8, hipMemcpyHostToDevice, st));
    HIPCHK(stream_wait(c));  // leaf_digests goes out of scope
    return 0;
}

// ---- phase 2: Merkle tree over bit-reversed LDE rows
int ProveCall::trace_merkle() {
    const LeafPrefix pf = prefix ? leaf_prefix(c) : LeafPrefix();
    HIPCHK(hipEventRecord(c->kev[0], st));
    if (c->opt_hasher == STARKHIP_HASHER_KECCAK) {
        // The Keccak leaf hash is the context's own launch on its own stream, pooled or not: the pool's merged and lane-group launches are
        // Poseidon forms (its jobs of this hasher are not announced to the scheduler either: pool.cpp), and "leaf_hash_form" and
        // "host_commit_leaves" pick among Poseidon forms
        c->hash_timing.form = SENT_KECCAK;
        c->hash_timing.group = 1;
        HIPCHK(launch_leaf_hash_keccak(c->lde.as<gl_t>(), s.C, s.log_n, s.r, c->digests.as<gl_t>(), st));
    } else if (s.N <= (size_t)c->opt_host_commit_leaves && s.C >= 64 && c->opt_leaf_hash_form == FORM_AUTO) {
        if (int rc = leaf_hash_on_host()) return rc;
    } else if (c->hs) {  // pooled: the scheduler decides when this commitment runs and which others share its launch
        c->hash_requested = true;
        HIPCHK(c->hs->hash(c->lde.as<gl_t>(), s.C, s.log_n, s.r, c->digests.as<gl_t>(), st, c->hash_ready, c->hash_done, !HashService::is_big(s.log_n, s.r), c->urgent,
                           &c->hash_timing, pf));
    } else {
        c->hash_timing.group = 1;
        HIPCHK(launch_leaf_hash_lone(c, c->lde.as<gl_t>(), s.C, s.log_n, s.r, c->digests.as<gl_t>(), st, &c->hash_timing.form, pf));
    }
    HIPCHK(hipEventRecord(c->kev[1], st));
    return commit_cap(mats[0]);
}

// The tiled evaluator (quotient_plan.h) with the context's current plan: per-proof weights of the plan's records, one pass over the
// LDE in LDS-staged column tiles, the chunks' partial sums combined into `qvals_out` ([2][size] words).  `timed`: the pass is the proof's
// quotient evaluation and is bracketed by kev[2] / kev[3].
int ProveCall::run_quotient_tiles(unsigned debug_mode, gl_t* qvals_out, bool timed) {
    const Ctx::PlanDev& D = *c->plan;
    HIPCHK(launch_quotient_weights(D.q_recs.as<QTRec>(), D.q_contrib_off.as<uint32_t>(), D.q_contribs.as<QTContrib>(), D.recs, D.q_apow.as<gl_t>(),
                                   air.prog.n_constraints, D.q_consts.as<gl_t>(), c->pis.as<gl_t>(), alphas[0], alphas[1], st));
    if (timed) HIPCHK(hipEventRecord(c->kev[2], st));
    HIPCHK(launch_quotient_tiles(D.q_recs.as<QTRec>(), D.q_streams.as<QTStream>(), D.q_chunk_tile_off.as<uint32_t>(), D.q_tile_list.as<uint32_t>(), D.chunks,
                                 c->lde.as<gl_t>(), c->tab->qtab.as<gl_t>(), c->partial.as<gl_t>(), s.log_n, s.r, s.qdb, (unsigned)s.C, debug_mode, st));
    if (timed) HIPCHK(hipEventRecord(c->kev[3], st));
    HIPCHK(launch_quotient_tiles_combine(c->partial.as<gl_t>(), D.chunks, c->tab->qtab.as<gl_t>(), s.log_n, s.qdb, qvals_out, st));
    return 0;
}

// The tiled evaluator by class ("quotient_cosets" = 0, QTClassPlan): every class's chunks on the cosets the class needs, then from the
// classes' sums to the quotient's COEFFICIENTS in qvals ([2][size] words, chunk after chunk) -- what the inverse transform of all
// `size` values gives (kernels_quotient.hip has the algebra).  kev[2] / kev[3] bracket the pass over the LDE as in run_quotient_tiles.
int ProveCall::run_quotient_classes() {
    const Ctx::PlanDev& D = *c->plan;
    HIPCHK(launch_quotient_weights(D.q_recs.as<QTRec>(), D.q_contrib_off.as<uint32_t>(), D.q_contribs.as<QTContrib>(), D.recs, D.q_apow.as<gl_t>(),
                                   air.prog.n_constraints, D.q_consts.as<gl_t>(), c->pis.as<gl_t>(), alphas[0], alphas[1], st));
    HIPCHK(hipEventRecord(c->kev[2], st));
    HIPCHK(launch_quotient_tiles(D.q_recs.as<QTRec>(), D.q_streams.as<QTStream>(), D.q_chunk_tile_off.as<uint32_t>(), D.q_tile_list.as<uint32_t>(), D.chunks,
                                 c->lde.as<gl_t>(), c->tab->qtab.as<gl_t>(), c->partial.as<gl_t>(), s.log_n, s.r, s.qdb, (unsigned)s.C, 0, st,
                                 D.q_work.as<uint32_t>(), D.n_work, D.n_classes));
    HIPCHK(hipEventRecord(c->kev[3], st));
    gl_t* const vecs = c->qclass.as<gl_t>();
    HIPCHK(launch_quotient_class_sums(c->partial.as<gl_t>(), D.q_sum_off.as<uint32_t>(), D.q_vec_slot.as<uint32_t>(), D.n_vecs, D.n_classes + 1,
                                      c->tab->qtab.as<gl_t>(), s.log_n, s.qdb, vecs, st));
    if (int rc = run_ntt(c, vecs, vecs + (size_t)2 * D.n_vecs * s.n, 2 * D.n_vecs, s.n, s.log_n, true, nullptr, nullptr)) return rc;
    HIPCHK(launch_quotient_class_solve(vecs, D.q_vec_of.as<uint32_t>(), D.n_classes, c->tab->qsolve.as<gl_t>(), s.log_n, s.qdb, c->qvals.as<gl_t>(), st));
    return 0;
}

// The op-stream interpreter (quotient_ops.h; "quotient_impl" = 1, kept as the cross-check) into qvals
int ProveCall::run_quotient_ops() {
    std::vector<gl_t> apow(2 * (AIR_MAX_GROUP + 1)), cscale(2 * n_chunks);
    for (int j = 0; j < 2; j++) {
        apow[j * (AIR_MAX_GROUP + 1)] = 1;
        for (unsigned m = 1; m <= AIR_MAX_GROUP; m++) apow[j * (AIR_MAX_GROUP + 1) + m] = gl_mul(apow[j * (AIR_MAX_GROUP + 1) + m - 1], alphas[j]);
        for (unsigned k = 0; k < n_chunks; k++) cscale[k * 2 + j] = gl_pow(alphas[j], c->prog.chunk_k_after[k]);
    }
    HIPCHK(hipMemcpyAsync(c->apow.p, apow.data(), apow.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->chunk_scale.p, cscale.data(), cscale.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->kev[2], st));
    HIPCHK(launch_quotient_eval(c->prog.ops.as<QOp>(), c->prog.loads.as<uint32_t>(), c->prog.slots, c->prog.chunk_off.as<uint32_t>(), n_chunks,
                                c->pis.as<gl_t>(), c->lde.as<gl_t>(), c->tab->qtab.as<gl_t>(), c->apow.as<gl_t>(), alphas[0], alphas[1],
                                c->partial.as<gl_t>(), s.log_n, s.r, s.qdb, st));
    HIPCHK(hipEventRecord(c->kev[3], st));
    HIPCHK(launch_quotient_combine(c->partial.as<gl_t>(), c->chunk_scale.as<gl_t>(), n_chunks, c->tab->qtab.as<gl_t>(), s.log_n, s.qdb,
                                   c->qvals.as<gl_t>(), st));
    HIPCHK(stream_wait(c));  // apow / cscale go out of scope
    return 0;
}

// development aid ("quotient_debug" = 9 with the interpreter): the tiled evaluator's values against the interpreter's on this very proof (stderr)
int ProveCall::compare_quotient_evaluators() {
    const size_t n = s.n, size = s.size, qdb = s.qdb;
    if (int rc = ensure_plan(c, air, size)) return rc;
    std::vector<gl_t> ref(2 * size), got(2 * size);
    HIPCHK(read_back(c, ref.data(), c->qvals.p, 2 * size * 8, st));
    HIPCHK(c->partial.ensure((size_t)std::max(n_chunks, c->plan->chunks) * 2 * size * 8));
    if (int rc = run_quotient_tiles(0, c->comb_partial.as<gl_t>(), false)) return rc;
    HIPCHK(read_back(c, got.data(), c->comb_partial.p, 2 * size * 8, st));
    HIPCHK(stream_wait(c));
    size_t bad = 0, last_blk = (size_t)-1;
    for (size_t i = 0; i < 2 * size; i++)
        if (ref[i] != got[i]) {
            const size_t ii = i % size, k = ii >> qdb, spp = ii & (((size_t)1 << qdb) - 1), tt = spp * n + k, blk = tt / 64;
            if (blk != last_blk && bad < 4096) fprintf(stderr, "quotient mismatch alpha %zu point-block %zu (sp %zu, k %zu..)\n", i / size, blk, spp, k & ~(size_t)63);
            last_blk = blk;
            bad++;
        }
    fprintf(stderr, "quotient compare: %zu of %zu values differ\n", bad, 2 * size);
    return 0;
}

// ---- phase 3, for an AIR with permutation pairs (COMPAT.md P1 - P3; timed with the quotient): the challenges, the Z polynomials from
// the copy of the pair columns, their closing products -- a Z that does not close ends the proof here with QUOTIENT_NOT_DIVISIBLE,
// before anything of the Zs is committed (upstream would go on to a quotient that does not divide, or to a proof nobody accepts) --
// then the Zs through the LDE and the commitment path of the trace under the context's hasher, and their cap into the transcript
int ProveCall::permutation() {
    const AirProgram& P = air.prog;
    const size_t n = s.n, nZ = s.nZ;
    fs.start();
    perm_chal.resize((size_t)P.perm_batch_size() * 4);  // P1: B sets (not n_batches), each 2 x (beta, gamma), set-major, beta first
    for (gl_t& x : perm_chal) x = ch.get();
    fs.stop();
    perm_desc = perm_descriptor(P, true);
    const std::vector<uint32_t> by_col = perm_descriptor(P, false);
    perm_desc.insert(perm_desc.end(), by_col.begin(), by_col.end());
    Ctx::PermBufs& pb = c->perm;
    HIPCHK(hipMemcpyAsync(pb.desc.p, perm_desc.data(), perm_desc.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pb.chal.p, perm_chal.data(), perm_chal.size() * 8, hipMemcpyHostToDevice, st));
    gl_t* const d_closing = pb.scan.as<gl_t>() + perm_scratch_words(n, (unsigned)nZ);
    HIPCHK(launch_perm_zs(pb.desc.as<uint32_t>(), pb.cols.as<gl_t>(), n, pb.chal.as<gl_t>(), n, (unsigned)nZ, pb.zvals.as<gl_t>(), pb.scan.as<gl_t>(), d_closing, st));
    std::vector<gl_t> closing(nZ);
    HIPCHK(read_back(c, closing.data(), d_closing, nZ * 8, st));
    HIPCHK(stream_wait(c));
    for (gl_t v : closing)
        if (v != 1) return STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE;
    HIPCHK(run_lde(c, pb.zvals.as<gl_t>(), lde_long_supported(s.log_n) ? pb.zcoef.as<gl_t>() : nullptr, pb.zlde.as<gl_t>(), nZ, s.log_n, s.r, 0));
    if (int rc = commit_narrow(mats[1], nZ)) return rc;
    HIPCHK(stream_wait(c));
    fs.start();
    ch.observe_many(mats[1].cap.data(), mats[1].cap.size());
    fs.stop();
    return 0;
}

// ---- phase 3, for an AIR with LogUp lookups (COMPAT.md L1 - L3; timed with the quotient), the twin of permutation(): the two challenges,
// the auxiliary polynomials from the copy of the named columns, their closing values and the count of zero denominators in one wait --
// a sum that does not close, or any zero denominator, ends the proof here with QUOTIENT_NOT_DIVISIBLE before anything is committed --
// then the LDE, the commitment under the context's hasher and the cap into the transcript
int ProveCall::logup() {
    const AirProgram& P = air.prog;
    const size_t n = s.n;
    const unsigned nzs = (unsigned)s.nLZ;
    fs.start();
    for (gl_t& x : logup_chal) x = ch.get();  // L1
    fs.stop();
    perm_desc = logup_descriptor(P, true, s.logup_general);  // by copy slot, by trace column, the Zs' polynomial indices
    for (const std::vector<uint32_t>& more : {logup_descriptor(P, false, s.logup_general), logup_z_polys(P)}) perm_desc.insert(perm_desc.end(), more.begin(), more.end());
    Ctx::PermBufs& pb = c->perm;
    HIPCHK(hipMemcpyAsync(pb.desc.p, perm_desc.data(), perm_desc.size() * 4, hipMemcpyHostToDevice, st));
    gl_t* const d_results = pb.scan.as<gl_t>() + logup_scratch_words(n, nzs);
    HIPCHK(launch_logup_polys(pb.desc.as<uint32_t>(), s.logup_general, pb.desc.as<uint32_t>() + 2 * s.perm_desc_words, pb.cols.as<gl_t>(), n, logup_chal[0], logup_chal[1], n, nzs,
                              pb.zvals.as<gl_t>(), pb.scan.as<gl_t>(), d_results, st));
    std::vector<gl_t> results(logup_result_words(nzs));
    HIPCHK(read_back(c, results.data(), d_results, results.size() * 8, st));
    HIPCHK(stream_wait(c));
    for (gl_t v : results)  // the closing values, then the zero denominators
        if (v != 0) return STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE;
    return 0;
}

// ... and the end of it, for LogUp lookups, CTL endpoints or both: the middle matrix LogUp || CTL through the LDE, one commitment under the
// context's hasher, its cap into the transcript (L3, C3), then the table's sums (C2)
int ProveCall::aux_commit() {
    Ctx::PermBufs& pb = c->perm;
    const size_t nM = s.nA + s.nC;
    HIPCHK(run_lde(c, pb.zvals.as<gl_t>(), lde_long_supported(s.log_n) ? pb.zcoef.as<gl_t>() : nullptr, pb.zlde.as<gl_t>(), nM, s.log_n, s.r, 0));
    if (int rc = commit_narrow(mats[1], nM)) return rc;
    HIPCHK(stream_wait(c));
    fs.start();
    ch.observe_many(mats[1].cap.data(), mats[1].cap.size());
    if (s.nC) ch.observe_many(ctl_sums.data(), ctl_sums.size());
    fs.stop();
    return 0;
}

// Between the halves of a table's proof (C3): the CTL polynomials h and Z of every endpoint under both challenge pairs, from the copy of
// the named columns, behind where logup() will put its own; the sums and the count of zero denominators come back to the host, and the
// sums stay on the device for the quotient.  The caller (the system) checks the balances before anything auxiliary is committed.
int ProveCall::ctl_polys(const gl_t chal[4]) {
    const size_t n = s.n;
    const unsigned E = (unsigned)s.nE;
    ctl_chal = {chal[0], chal[1], chal[2], chal[3]};
    ctl_sums.assign(2 * E, 0);
    ctl_zero_denominators.assign(E, 0);
    if (!E) return 0;
    Ctx::PermBufs& pb = c->perm;
    std::vector<uint32_t> desc = ctl_descriptor(*ctl, true, (uint32_t)s.perm_cols);
    for (const std::vector<uint32_t>& more : {ctl_z_polys(*ctl, (uint32_t)s.nA), ctl_descriptor(*ctl, false)}) desc.insert(desc.end(), more.begin(), more.end());
    uint32_t* const d_desc = pb.desc.as<uint32_t>() + ctl_desc_at();
    HIPCHK(hipMemcpyAsync(d_desc, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(launch_ctl_polys(d_desc, d_desc + s.ctl_desc_words, pb.cols.as<gl_t>(), n, ctl_chal, n, E, pb.zvals.as<gl_t>(), (unsigned)s.nA, pb.scan.as<gl_t>(),
                            pb.chal.as<gl_t>(), st));
    std::vector<gl_t> results(ctl_result_words(E));
    HIPCHK(read_back(c, results.data(), pb.chal.p, results.size() * 8, st));
    HIPCHK(stream_wait(c));  // desc goes out of scope
    std::copy(results.begin(), results.begin() + 2 * E, ctl_sums.begin());
    ctl_zero_denominators.assign(results.begin() + 2 * E, results.end());
    return 0;
}

// ---- phase 3: quotient polynomials (App. A.6)
int ProveCall::quotient() {
    const size_t n = s.n, size = s.size, factor = s.factor;
    HIPCHK(stream_wait(c));  // the trace cap
    fs.start();
    if (ch_initial) {  // a table of a system starts from the system transcript, which has observed every table's trace cap (C2)
        const int hasher = ch.hasher;
        ch = *ch_initial;
        ch.hasher = hasher;
    } else {
        ch.observe_many(mats[0].cap.data(), mats[0].cap.size());  // public inputs are NOT observed (App. A.5)
    }
    fs.stop();
    if (s.nZ)
        if (int rc = permutation()) return rc;
    if (s.nA)
        if (int rc = logup()) return rc;
    if (s.nA + s.nC)
        if (int rc = aux_commit()) return rc;
    fs.start();
    alphas[0] = ch.get();
    alphas[1] = ch.get();
    fs.stop();
    if (s.pl.n_pis) HIPCHK(hipMemcpyAsync(c->pis.p, pis_host, s.pl.n_pis * 8, hipMemcpyHostToDevice, st));
    const unsigned debug = (unsigned)((c->opt_quotient_debug <= 4 || c->opt_quotient_debug == 8) ? c->opt_quotient_debug : 0);
    if (tiled && c->plan->by_class) {  // the classes' sums on their cosets, recombined: the coefficients are in qvals
        if (int rc = run_quotient_classes()) return rc;
    } else {
        if (int rc = tiled ? run_quotient_tiles(debug, c->qvals.as<gl_t>(), true) : run_quotient_ops()) return rc;
        if (c->opt_quotient_debug == 9 && !tiled)
            if (int rc = compare_quotient_evaluators()) return rc;
        if (s.nZ)  // P4: the permutation constraints join the fold where its values are (kernels_permutation.hip)
            HIPCHK(launch_perm_quotient(c->perm.desc.as<uint32_t>() + s.perm_desc_words, c->lde.as<gl_t>(), c->perm.zlde.as<gl_t>(), c->perm.chal.as<gl_t>(),
                                        c->tab->qtab.as<gl_t>(), c->qvals.as<gl_t>(), alphas[0], alphas[1], gl_pow(alphas[0], 2 * s.nZ), gl_pow(alphas[1], 2 * s.nZ),
                                        s.log_n, s.r, s.qdb, st));
        if (s.nA) {  // L4: the LogUp constraints likewise (kernels_logup.hip)
            const uint64_t nL = air.prog.logup_constraints();
            HIPCHK(launch_logup_quotient(c->perm.desc.as<uint32_t>() + s.perm_desc_words, s.logup_general, c->lde.as<gl_t>(), c->perm.zlde.as<gl_t>(), logup_chal[0], logup_chal[1],
                                         c->tab->qtab.as<gl_t>(), c->qvals.as<gl_t>(), alphas[0], alphas[1], gl_pow(alphas[0], nL), gl_pow(alphas[1], nL), s.log_n, s.r,
                                         s.qdb, st));
        }
        if (s.nC) {  // C4: the CTL constraints after them (kernels_ctl.hip)
            const uint64_t nK = ctl->constraints() / 2;  // one challenge's share: the kernel scales what is there by its square
            HIPCHK(launch_ctl_quotient(c->perm.desc.as<uint32_t>() + ctl_desc_at() + s.ctl_desc_words + 2 * s.nE, c->lde.as<gl_t>(), c->perm.zlde.as<gl_t>() + s.nA * s.N, ctl_chal,
                                       c->perm.chal.as<gl_t>(), c->tab->qtab.as<gl_t>(), c->qvals.as<gl_t>(), alphas[0], alphas[1], gl_pow(alphas[0], nK), gl_pow(alphas[1], nK),
                                       s.log_n, s.r, s.qdb, st));
        }
        // coset_ifft(7): inverse transform, scale by size^-1 and by 7^-i
        if (int rc = run_ntt(c, c->qvals.as<gl_t>(), c->partial.as<gl_t>(), 2, size, s.log_n + s.qdb, true, nullptr, c->tab->qshift_inv.as<gl_t>()))  // (the chunks' partial sums are spent)
            return rc;
    }
    // trim_to_len(n * factor) must succeed (quotient_commit() looks at the tail), then chunks of n: [alpha0: c0..cf-1, alpha1: c0..cf-1]
    if (size > factor * n) {
        quot_tail.resize(2 * (size - factor * n));
        for (int j = 0; j < 2; j++)
            HIPCHK(read_back(c, quot_tail.data() + j * (size - factor * n), c->qvals.as<gl_t>() + j * size + factor * n, (size - factor * n) * 8, st));
    }
    for (int j = 0; j < 2; j++)
        HIPCHK(hipMemcpyAsync(c->qcoef.as<gl_t>() + (size_t)j * factor * n, c->qvals.as<gl_t>() + j * size, factor * n * 8, hipMemcpyDeviceToDevice, st));
    return 0;
}

// ---- phase 4: quotient commit (PolynomialBatch::from_coeffs)
int ProveCall::quotient_commit() {
    HIPCHK(stream_wait(c));  // the quotient's coefficients beyond n * factor
    for (gl_t v : quot_tail)
        if (v != 0) return STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE;
    HIPCHK(run_lde(c, c->qcoef.as<gl_t>(), nullptr, c->qlde.as<gl_t>(), s.Q, s.log_n, s.r, 1));
    return commit_narrow(mats[s.pl.n_mats - 1], s.Q);
}

// ---- phase 5: openings (App. A.7)
int ProveCall::openings() {
    const size_t n = s.n;
    HIPCHK(stream_wait(c));  // the quotient cap
    fs.start();
    ch.observe_many(mats[s.pl.n_mats - 1].cap.data(), 4 * s.ncap);
    zeta = ch.get_ext();
    fs.stop();
    if (c->opt_zeta_on_coset > 0)  // test hook ("zeta_on_coset" = k + 1): zeta = 7 w_n^k, a point of coset 0 itself (probability 2^-115 in a real transcript)
        zeta = gl2_make(gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(s.log_n), (uint64_t)(c->opt_zeta_on_coset - 1) & (n - 1))), 0);
    if (gl2_eq(gl2_pow(zeta, n), gl2_one())) return STARKHIP_ERR_ZETA_IN_SUBGROUP;
    // the trace polynomials from their values on coset 0 of the LDE (kernels_fri.hip: the context keeps no coefficients of them), the
    // quotient polynomials from their coefficients
    const gl_t shift_n = gl_pow(GL_GENERATOR, n);  // 7^n
    const gl2_t zh = gl2_sub(gl2_pow(zeta, n), gl2_make(shift_n, 0));
    // (zh = 0: zeta lies on the coset 7 H itself -- the weights are then an indicator vector, coset_weights_kernel; starky proves there too)
    const gl2_t w_scale = gl2_mul_base(zh, gl_inv(gl_mul((gl_t)n, shift_n)));
    HIPCHK(launch_ext_powers(c->zpow.as<gl2_t>(), zeta, n, st));
    HIPCHK(launch_coset_weights(c->zpow.as<gl2_t>() + n, c->gzpow.as<gl2_t>(), zeta, w_scale, s.log_n, st));
    for (size_t k = 0; k < s.pl.n_mats; k++) {  // (P5: the Zs like the trace)
        const Committed& m = mats[k];
        if (m.coef) HIPCHK(launch_openings(m.coef->as<gl_t>(), n, s.pl.mat[k].cols, n, c->zpow.as<gl2_t>(), nullptr, m.d_open[0]->as<gl2_t>(), nullptr, st));
        else HIPCHK(launch_openings(m.lde->as<gl_t>(), s.N, s.pl.mat[k].cols, n, c->zpow.as<gl2_t>() + n, c->gzpow.as<gl2_t>(), m.d_open[0]->as<gl2_t>(), m.d_open[1]->as<gl2_t>(), st));
    }
    for (size_t k = 0; k < s.pl.n_mats; k++)
        for (size_t b = 0, cnt; b < 2 && (cnt = s.pl.mat[k].n_open[b]); b++) {
            mats[k].open[b].resize(cnt);
            HIPCHK(read_back(c, mats[k].open[b].data(), mats[k].d_open[b]->p, cnt * 16, st));
        }
    return 0;
}

// ---- phase 6: FRI batch combination (prove_openings, App. A.8)
int ProveCall::fri_combine() {
    const size_t n = s.n, N = s.N;
    HIPCHK(stream_wait(c));  // the openings
    fs.start();  // 2 (2 C + Q) field elements through the sponge, one permutation per 8: the longest host stretch of a proof
    for (int b = 0; b < 2; b++)  // batch 0: every matrix at zeta -- local || zs || quotient, batch 1: at g zeta -- next || zs_next (P5)
        for (size_t k = 0; k < s.pl.n_mats; k++)
            for (const gl2_t& v : mats[k].open[b]) ch.observe_ext(v);
    const gl2_t fri_alpha = ch.get_ext();
    fs.stop();
    const gl2_t gzeta = gl2_mul_base(zeta, gl_root_of_unity(s.log_n));
    HIPCHK(launch_ext_powers(c->ext_apow.as<gl2_t>(), fri_alpha, s.pl.batch_cols[0], st));
    // sum_j alpha^j trace_j: the sum is taken on coset 0 of the LDE (n values a column) and turned into coefficients by ONE inverse
    // coset transform of its two words -- linear, so these are the coefficients of the reference's sum of coefficient vectors
    gl_t* comb_t = c->comb_out.as<gl_t>();        // [2][n] words
    gl2_t* comb_q = c->comb_out.as<gl2_t>() + n;  // [n] extension elements
    // every matrix kept as an LDE, up to the quotient: its run of powers of alpha, its chunks of the sum (the Zs, at most 128 < COMB_PPC: one more)
    size_t k = 0, col = 0, chunk = 0;
    for (; !mats[k].coef; k++) {
        const size_t cols = s.pl.mat[k].cols;
        HIPCHK(launch_fri_combine(mats[k].lde->as<gl_t>(), N, cols, n, c->ext_apow.as<gl2_t>() + col, COMB_PPC, comb_chunks(cols), c->comb_partial.as<gl2_t>() + chunk * n, st));
        col += cols;
        chunk += comb_chunks(cols);
    }
    HIPCHK(launch_ext_reduce(c->comb_partial.as<gl2_t>(), chunk, n, comb_t, st));
    if (int rc = run_ntt(c, comb_t, c->fri_vals.as<gl_t>(), 2, n, s.log_n, true, nullptr, c->tab->qshift_inv.as<gl_t>())) return rc;  // (fri_vals: idle until fri_commit)
    HIPCHK(launch_fri_combine(mats[k].coef->as<gl_t>(), n, s.Q, n, c->ext_apow.as<gl2_t>() + col, s.Q, 1, comb_q, st));  // alpha^(C+nZ+q) quotient_q
    std::vector<gl_t> F1w(2 * n);
    std::vector<gl2_t> F1(n), tailq(n), F0(n), q0(n), q1(n), fin(n);
    HIPCHK(read_back(c, F1w.data(), comb_t, n * 16, st));
    HIPCHK(read_back(c, tailq.data(), comb_q, n * 16, st));
    HIPCHK(stream_wait(c));
    host_other.start();
    for (size_t k = 0; k < n; k++) F1[k] = gl2_make(F1w[k], F1w[n + k]);
    for (size_t k = 0; k < n; k++) F0[k] = gl2_add(F1[k], tailq[k]);
    divide_by_linear(F0.data(), n, zeta, q0.data());  // batch 0: trace ++ Zs ++ quotient at zeta
    divide_by_linear(F1.data(), n, gzeta, q1.data());   // batch 1: trace ++ Zs at g*zeta
    const gl2_t shift = gl2_pow(fri_alpha, s.pl.batch_cols[1]);  // alpha^{|batch 1|}
    for (size_t k = 0; k < n; k++) fin[k] = gl2_add(gl2_mul(q0[k], shift), q1[k]);
    // upload as SoA, zero padded to N (lde(rate_bits))
    std::vector<gl_t> soa(2 * N, 0);
    for (size_t k = 0; k < n; k++) {
        soa[k] = fin[k].a0;
        soa[N + k] = fin[k].a1;
    }
    host_other.stop();
    HIPCHK(hipMemcpyAsync(c->fri_coef.p, soa.data(), 2 * N * 8, hipMemcpyHostToDevice, st));
    HIPCHK(stream_wait(c));  // soa goes out of scope
    return 0;
}

// ---- phase 7: FRI commit phase (fri_committed_trees)
int ProveCall::fri_commit() {
    const size_t ncap = s.ncap;
    fri_caps.resize(s.L * 4 * ncap);
    final_poly.resize(s.geo.final_poly_len);
    size_t len = s.N;
    unsigned log_len = s.log_N;
    gl_t shift = GL_GENERATOR;
    gl_t* coef = c->fri_coef.as<gl_t>();
    gl_t* vals = c->fri_vals.as<gl_t>();
    for (size_t l = 0; l < s.L; l++) {
        // values on shift * <w_len>
        HIPCHK(launch_fill_powers(c->scale_tab.as<gl_t>(), 1, shift, len, st));
        if (long_vector(log_len)) {  // coef -> vals in the transform's first pass, the second in place
            LdeLongTables tb;
            if (int rc = ensure_long_tw(c, log_len, &tb)) return rc;
            HIPCHK(launch_ntt_long(coef, vals, vals, 2, len, log_len, false, c->scale_tab.as<gl_t>(), nullptr, tb, st));
        } else {
            HIPCHK(hipMemcpyAsync(vals, coef, len * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(vals + len, coef + len, len * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(launch_ntt_global(vals, 2, len, log_len, c->tab->tw_fwd.as<gl_t>(), s.log_N, c->scale_tab.as<gl_t>(), nullptr, 1, st));
        }
        const unsigned ab = s.geo.arities[l];
        const size_t n_leaves = len >> ab, width = 2 << ab;
        HIPCHK(launch_fri_leaves(vals, log_len, ab, c->fri_rows[l].as<gl_t>(), st));
        HIPCHK(launch_leaf_hash_rows_by((int)c->opt_hasher, c->fri_rows[l].as<gl_t>(), width, n_leaves, c->fri_digests[l].as<gl_t>(), st));
        HIPCHK(launch_merkle_levels_by((int)c->opt_hasher, c->fri_digests[l].as<gl_t>(), log_len - ab, s.cap_h, st));
        // leaves and digests stay on the device (the query phase gathers from them); only the cap feeds the transcript
        gl_t* cap = fri_caps.data() + l * 4 * ncap;
        HIPCHK(read_back(c, cap, c->fri_digests[l].as<gl_t>() + 4 * level_off(n_leaves, log_len - ab - s.cap_h), 4 * ncap * 8, st));
        HIPCHK(stream_wait(c));
        fs.start();
        ch.observe_many(cap, 4 * ncap);
        const gl2_t beta = ch.get_ext();
        fs.stop();
        // fold the coefficients into the other buffer, which then holds them SoA [2][len >> ab], and swap the two
        HIPCHK(launch_fri_fold(coef, len, ab, beta, vals, st));
        std::swap(coef, vals);
        len >>= ab;
        log_len -= ab;
        for (unsigned b = 0; b < ab; b++) shift = gl_sqr(shift);
    }
    // final polynomial: truncate to len >> rate_bits; the dropped coefficients must be zero
    std::vector<gl_t> fc(2 * len);
    HIPCHK(read_back(c, fc.data(), coef, len * 8, st));
    HIPCHK(read_back(c, fc.data() + len, coef + len, len * 8, st));
    HIPCHK(stream_wait(c));
    if ((len >> s.r) != s.geo.final_poly_len) return STARKHIP_ERR_BAD_SHAPE;
    for (size_t k = 0; k < len; k++) {
        if (k < s.geo.final_poly_len) final_poly[k] = gl2_make(fc[k], fc[len + k]);
        else if (fc[k] || fc[len + k]) return STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE;
    }
    fs.start();
    for (auto& e : final_poly) ch.observe_ext(e);
    fs.stop();
    return 0;
}

// ---- phase 8: proof of work (fri_proof_of_work): smallest nonce unless one is supplied
int ProveCall::pow() {
    if (pow_witness == STARKHIP_POW_SEARCH) {
        if (cfg.proof_of_work_bits == 0) {
            pow_witness = 0;
        } else {
            gl_t base[12];
            memcpy(base, ch.state, sizeof base);
            for (int i = 0; i < ch.n_in; i++) base[i] = ch.in[i];
            HIPCHK(hipMemcpyAsync(c->pow_state.p, base, sizeof base, hipMemcpyHostToDevice, st));
            unsigned long long best = ~0ULL;
            const uint64_t batch = 1ULL << 20;
            for (uint64_t start = 0; best == ~0ULL; start += batch) {
                if (start >= GL_P - batch) return STARKHIP_ERR_HIP;
                HIPCHK(hipMemcpyAsync(c->pow_best.p, &best, 8, hipMemcpyHostToDevice, st));
                if (c->opt_hasher == STARKHIP_HASHER_KECCAK)
                    HIPCHK(launch_pow_grind_keccak(c->pow_state.as<gl_t>(), ch.n_in, cfg.proof_of_work_bits, start, batch, c->pow_best.as<unsigned long long>(), st));
                else
                    HIPCHK(launch_pow_grind(c->pow_state.as<gl_t>(), ch.n_in, cfg.proof_of_work_bits, start, batch, c->pow_best.as<unsigned long long>(), st));
                HIPCHK(read_back(c, &best, c->pow_best.p, 8, st));
                HIPCHK(stream_wait(c));
            }
            pow_witness = best;
        }
    }
    ch.observe(pow_witness);
    (void)ch.get();  // pow_response
    return 0;
}

// ---- phase 9: query rounds (fri_prover_query_rounds) and the proof's assembly.  From blob_alloc on a failing HIP call is noted, not
// returned from (HIPCHK_FREE): the copy into the blob may be in flight, so the stream is waited for before the blob is freed.
int ProveCall::queries() {
    const ProofLayout& pl = s.pl;
    const size_t N = s.N, L = s.L, ncap = s.ncap;
    if (!c->hs && !c->blob_airs.count(air.id)) {
        // a context on its own (not a pool's: those reserve at warm-up) gets its two page-locked blobs with its first proof of an AIR,
        // the proof that also grows the work buffers -- hipHostMalloc waits for the device like the hipMallocs before it
        static const bool pinned = [] { const char* e = getenv("STARKHIP_PINNED_PROOFS"); return !(e && *e == '0'); }();
        if (pinned) (void)blob_arena_add(c, pl.total * 8, 2);  // failure: malloc serves the proof
        c->blob_airs.insert(air.id);
    }
    out = blob_alloc(pl.total * 8);  // page-locked if the context has reserved blobs (blob_arena.h)
    if (!out) return STARKHIP_ERR_OOM;
    const size_t nq = pl.n_queries;
    std::vector<uint32_t> xs(nq);
    for (size_t q = 0; q < nq; q++) xs[q] = (uint32_t)(ch.get() % N);
    // every round's leaves and Merkle paths are gathered on the device, already in proof layout
    const size_t stride = pl.query_words;
    const unsigned d0 = s.log_N - s.cap_h;
    int err = 0;
#define HIPCHK_FREE(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { fprintf(stderr, "starkhip: HIP error %s (%s)\n", hipGetErrorString(_e), #expr); err = 1; } } while (0)
    gl_t* dq = c->gather_t.as<gl_t>();
    if (nq) HIPCHK_FREE(hipMemcpyAsync(c->qidx.p, xs.data(), nq * 4, hipMemcpyHostToDevice, st));
    const uint32_t* dxs = c->qidx.as<uint32_t>();
    size_t off = pl.quotient().q_sib + 4 * d0;  // the FRI steps follow the matrices' leaves and paths
    if (!err) {
        for (size_t k = 0; k < pl.n_mats; k++) {  // P6: trace, zs, quotient
            const MatrixLayout& e = pl.mat[k];
            HIPCHK_FREE(launch_query_leaf_colmajor(mats[k].lde->as<gl_t>(), e.cols, s.log_n, s.r, dxs, nq, dq, stride, e.q_leaf, st));
            HIPCHK_FREE(launch_query_path(mats[k].digests->as<gl_t>(), N, d0, dxs, 0, nq, dq, stride, e.q_sib, st));
        }
        size_t len = N;
        unsigned shift_bits = 0;
        for (size_t l = 0; l < L; l++) {
            const unsigned ab = s.geo.arities[l];
            const size_t width = 2 << ab, n_leaves = len >> ab;
            shift_bits += ab;
            HIPCHK_FREE(launch_query_leaf_rows(c->fri_rows[l].as<gl_t>(), width, dxs, shift_bits, nq, dq, stride, off, st)); off += width;
            HIPCHK_FREE(launch_query_path(c->fri_digests[l].as<gl_t>(), n_leaves, (unsigned)pl.layer_depth[l], dxs, shift_bits, nq, dq, stride, off, st));
            off += 4 * pl.layer_depth[l];
            len = n_leaves;
        }
        if (nq) HIPCHK_FREE(hipMemcpyAsync(out + pl.off_queries, dq, nq * stride * 8, hipMemcpyDeviceToHost, st));
    }
    pl.write_header(out);
    for (size_t k = 0; k < pl.n_mats; k++) {
        const MatrixLayout& e = pl.mat[k];
        memcpy(out + e.off_cap, mats[k].cap.data(), 4 * ncap * 8);
        for (size_t b = 0; b < 2 && e.n_open[b]; b++) memcpy(out + e.off_open[b], mats[k].open[b].data(), e.n_open[b] * 16);
    }
    if (L) memcpy(out + pl.off_fri_caps, fri_caps.data(), L * 4 * ncap * 8);
    HIPCHK_FREE(stream_wait(c));  // xs goes out of scope
#undef HIPCHK_FREE
    if (err || off != stride) {
        blob_free(out);
        return STARKHIP_ERR_HIP;
    }
    memcpy(out + pl.off_final, final_poly.data(), s.geo.final_poly_len * 16);
    out[pl.off_pow] = pow_witness;
    if (pl.n_pis) memcpy(out + pl.off_pis, pis_host, pl.n_pis * 8);
    if (pl.nC) memcpy(out + pl.off_sums, ctl_sums.data(), ctl_sums.size() * 8);  // C6: the table's sums, the last section
    return 0;
}

}  // namespace

// One proof between its two halves: the shape, the copies of the arguments its phases keep pointing at, the phases' state and where the
// list of phases stands.  The guard of the read-backs lives as long as the proof does.
struct ProveJob {
    Ctx* c;
    const AirInfo& air;
    starkhip_config_t cfg;
    TraceInput in;
    std::vector<uint64_t> pis;
    CtlTable ctl;
    ProofShape s;
    std::unique_ptr<ProveCall> p;
    int evi = 0;
    bool quotient_started = false;  // prove_ctl_polys has recorded the quotient phase's boundary
    PhaseRanges ranges;
    ProveJob(Ctx* c_, const AirInfo& air_, const starkhip_config_t& cfg_, const TraceInput& in_, const uint64_t* pis_, size_t n_pis, const CtlTable* ctl_)
        : c(c_), air(air_), cfg(cfg_), in(in_), pis(pis_, pis_ + n_pis) {
        if (ctl_) ctl = *ctl_;
    }
    ~ProveJob() {  // an early return between a read_back() and its stream_wait() must not leave destinations of this proof behind
        c->rb_pending.clear();
        c->rb_used = 0;
    }
};

namespace {
// before each phase: the boundary event of starkhip_last_timings on the stream and the phase's rocTX range (rocprofv3 --marker-trace)
const struct { const char* range; int (ProveCall::*run)(); } PHASES[STARKHIP_N_PHASES - 1] = {
    {"starkhip:upload", &ProveCall::upload}, {"starkhip:ifft_lde", &ProveCall::ifft_lde}, {"starkhip:trace_merkle", &ProveCall::trace_merkle},
    {"starkhip:quotient", &ProveCall::quotient}, {"starkhip:quotient_commit", &ProveCall::quotient_commit}, {"starkhip:openings", &ProveCall::openings},
    {"starkhip:fri_combine", &ProveCall::fri_combine}, {"starkhip:fri_commit", &ProveCall::fri_commit}, {"starkhip:pow", &ProveCall::pow},
    {"starkhip:queries", &ProveCall::queries}};
const int FIRST_HALF_PHASES = 3;  // upload, ifft_lde, trace_merkle

// phases [from, to) of the job; a refused trace hands its check blob out
int run_phases(ProveJob* j, int from, int to, uint64_t** proof_out, size_t* proof_words) {
    ProveCall& p = *j->p;
    for (int k = from; k < to; k++) {
        if (!(k == FIRST_HALF_PHASES && j->quotient_started)) {
            HIPCHK(hipEventRecord(j->c->ev[j->evi++], p.st));
            j->ranges.next(PHASES[k].range);
        }
        if (int rc = (p.*PHASES[k].run)()) {
            if (rc == STARKHIP_ERR_TRACE) {  // the check blob instead of a proof
                *proof_out = p.out;
                *proof_words = p.check_words;
            }
            return rc;
        }
    }
    return 0;
}
}  // namespace

// The transcript of SURVEY.md App. A.5 in two halves over one ProveCall.  The first: argument checks, tables and plan, buffers, then the
// phases upload .. trace_merkle.  The order of what the phases enqueue on the context's stream and the places where the host waits for it
// make the phase timings mean what starkhip.h says; a pool's overlap depends on it.  `ctl`: the endpoints of a table of a system, or null.
int prove_first_half(Ctx* c, const AirInfo& air, const starkhip_config_t& cfg, const TraceInput& in_arg, const uint64_t* pis_arg, size_t n_pis, uint64_t pow_witness,
                     const CtlTable* ctl, ProveJob** job_out, uint64_t** proof_out, size_t* proof_words) {
    *job_out = nullptr;
    if (n_pis != air.prog.n_pis || in_arg.n_cols != air.prog.n_cols) return STARKHIP_ERR_BAD_SHAPE;
    std::unique_ptr<ProveJob> job(new ProveJob(c, air, cfg, in_arg, pis_arg, n_pis, ctl));
    ProofShape& s = job->s;
    const TraceInput& in = job->in;
    const uint64_t* pis_host = job->pis.data();
    if (ProofShape::make(air, cfg, in.n_rows, &s, ctl ? &job->ctl : nullptr) != STARKHIP_OK) return STARKHIP_ERR_BAD_SHAPE;
    s.pl.hasher = (size_t)c->opt_hasher;  // header word 12
    for (size_t i = 0; i < n_pis; i++)
        if (pis_host[i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->st;
    if (int rc = ensure_tables(c, s.log_n, s.r, s.qdb)) return rc;
    const bool tiled = c->opt_quotient_impl == 0;
    // the profiling modes and the evaluators' comparison run every constraint on every coset, like "quotient_cosets" = 1
    // ... and so does an AIR with permutation pairs: their constraints join the quotient's values, which the classes never form
    const bool by_class = tiled && c->opt_quotient_cosets == 0 && c->opt_quotient_debug == 0 && s.mid == 0;
    if (int rc = tiled ? ensure_plan(c, air, s.size, by_class) : ensure_program(c, air, s.size)) return rc;
    const unsigned n_chunks = tiled ? c->plan->chunks : c->prog.chunks;

    // ---- buffers
    // The trace waits for the LDE INSIDE the buffer the LDE is written to, as its last C n words (trace_in_lde: run_lde_trace);
    // a separate buffer only when there is no room beside it (rate_bits == 0, or a recording longer than the rest of the buffer).
    const size_t n = s.n, N = s.N, C = s.C;
    const bool fill = c->opt_fill_lookups && !air.lookups.empty();
    const bool fill_freq = c->opt_fill_frequencies && !air.prog.logups.empty();
    if (fill_freq && !logup_fillable(air.prog, nullptr)) return STARKHIP_ERR_BAD_AIR;
    const bool callers_columns = in.callers_columns() && !fill && !fill_freq;  // (a fill works on the prover's own copy of the columns)
    const size_t park_words = in.park_words(C);  // what the upload parks at the start of the LDE buffer, in 64-bit words
    // A long trace (2^14 rows and more) is not parked there: its transform goes through the LDE buffer between its two passes and keeps
    // the coefficients in `values`, a whole trace of words, whoever owns the input (run_lde).
    const bool long_trace = lde_long_supported(s.log_n);
    const bool trace_in_lde = s.r >= 1 && park_words <= (((size_t)1 << s.r) - 1) * C * n && !callers_columns && !long_trace;
    // `values`: the columns the last LDE launch reads (run_lde_trace), a whole trace, or nothing this proof needs
    const size_t values_bytes = values_bytes_for(s, trace_in_lde, callers_columns);
    for (const BufWant& w : work_buffers(c, s, n_chunks, tiled ? c->plan : nullptr, values_bytes, park_words * 8, fill ? air.lookups.size() : 0, fill_freq ? &air.prog : nullptr)) HIPCHK(w.b->ensure(w.bytes));
    if (int rc = ensure_long_tables(c, s)) return rc;
    const bool prefix = leaf_prefix_wanted(c, C, s.log_n, s.r);
    if (prefix)
        if (int rc = ensure_leaf_prefix(c, s.log_n, s.r)) return rc;

    job->p.reset(new ProveCall{c, air, job->cfg, s, st, in, pis_host, pow_witness, tiled, n_chunks, trace_in_lde, fill, fill_freq, prefix,
                               trace_in_lde ? c->lde.as<gl_t>() + (N - n) * C : c->values.as<gl_t>()});
    job->p->ch.hasher = (int)c->opt_hasher;  // the transcript's sponge duplexes through the context's hasher
    if (ctl) job->p->ctl = &job->ctl;
    if (int rc = run_phases(job.get(), 0, FIRST_HALF_PHASES, proof_out, proof_words)) return rc;
    *job_out = job.release();
    return STARKHIP_OK;
}

// what a system needs of a table between the halves: its trace cap (the wait for it is the one quotient() would have made) ...
int prove_trace_cap(ProveJob* j, const uint64_t** cap, size_t* words) {
    HIPCHK(stream_wait(j->c));
    *cap = j->p->mats[0].cap.data();
    *words = j->p->mats[0].cap.size();
    return STARKHIP_OK;
}
int prove_job_hasher(ProveJob* j) { return j->p->ch.hasher; }
// ... and its CTL polynomials under the system's challenges: sums [2 E] challenge-major and, per endpoint, the count of zero denominators [E]
int prove_ctl_polys(ProveJob* j, const uint64_t chal[4], uint64_t* sums, uint64_t* zero_denominators) {
    HIPCHK(hipSetDevice(j->c->device));
    // the quotient phase starts here: the CTL polynomials are timed with it, as the LogUp ones are (the second half does not record the
    // boundary again).  What the stream idled since its trace commitment -- the other tables' first halves -- ends up in trace_merkle.
    if (!j->quotient_started) {
        HIPCHK(hipEventRecord(j->c->ev[j->evi++], j->p->st));
        j->ranges.next(PHASES[FIRST_HALF_PHASES].range);
        j->quotient_started = true;
    }
    if (int rc = j->p->ctl_polys(chal)) return rc;
    std::copy(j->p->ctl_sums.begin(), j->p->ctl_sums.end(), sums);
    std::copy(j->p->ctl_zero_denominators.begin(), j->p->ctl_zero_denominators.end(), zero_denominators);
    return STARKHIP_OK;
}

// The second half: quotient .. queries.  `initial`: the challenger the table's transcript starts from (a table of a system), or null: the
// proof observes its own trace cap, as a proof on its own does.  The job is spent either way.
int prove_second_half(ProveJob* job_in, const Challenger* initial, uint64_t** proof_out, size_t* proof_words) {
    std::unique_ptr<ProveJob> job(job_in);
    Ctx* c = job->c;
    ProveCall& p = *job->p;
    const ProofShape& s = job->s;
    HIPCHK(hipSetDevice(c->device));
    p.ch_initial = initial;
    if (int rc = run_phases(job.get(), FIRST_HALF_PHASES, STARKHIP_N_PHASES - 1, proof_out, proof_words)) return rc;
    hipStream_t st = p.st;
    uint64_t* const out = p.out;
    if (hipEventRecord(c->ev[job->evi++], st) != hipSuccess || stream_wait(c) != hipSuccess) {
        blob_free(out);
        return STARKHIP_ERR_HIP;
    }
    for (int i = 0; i < STARKHIP_N_PHASES - 1; i++) (void)hipEventElapsedTime(&c->timings[i], c->ev[i], c->ev[i + 1]);
    (void)hipEventElapsedTime(&c->timings[STARKHIP_N_PHASES - 1], c->ev[0], c->ev[STARKHIP_N_PHASES - 1]);
    (void)hipEventElapsedTime(&c->ktimings[2], c->kev[2], c->kev[3]);
    if (c->opt_quotient_debug >= 1 && c->opt_quotient_debug <= 8) {  // profiling build only: timings are valid, the proof is not
        blob_free(out);
        return STARKHIP_ERR_VERIFY;
    }
    c->htimings[0] = (float)p.fs.ms;
    c->htimings[1] = (float)p.host_other.ms;
    (void)hipEventElapsedTime(&c->ktimings[0], c->kev[4], c->kev[5]);
    // pooled: the commitment kernel's own duration on the scheduler's launch stream (kev[0] .. kev[1] on this context's stream would
    // include the wait for its group to form)
    if (c->hs && c->hash_timing.form != SENT_HOST && c->hash_timing.form != SENT_KECCAK) (void)hipEventElapsedTime(&c->ktimings[1], c->hash_timing.t0, c->hash_timing.t1);
    else (void)hipEventElapsedTime(&c->ktimings[1], c->kev[0], c->kev[1]);
    *proof_out = out;
    *proof_words = s.pl.total;
    return STARKHIP_OK;
}
void prove_job_free(ProveJob* job) { delete job; }

// A proof on its own: the two halves back to back, no endpoints, no initial challenger
int prove(Ctx* c, const AirInfo& air, const starkhip_config_t& cfg, const TraceInput& in, const uint64_t* pis_host, size_t n_pis, uint64_t pow_witness,
          uint64_t** proof_out, size_t* proof_words) {
    ProveJob* job = nullptr;
    if (int rc = prove_first_half(c, air, cfg, in, pis_host, n_pis, pow_witness, nullptr, &job, proof_out, proof_words)) return rc;
    return prove_second_half(job, nullptr, proof_out, proof_words);
}

// Everything a proof of `air` (default rows, config `cfg`) will ask of this context, allocated NOW: shape tables, the constraint
// plan, every work buffer, the page-locked staging of a recording of `log_bytes`.  A pool warms its contexts with this before the
// first job: growing a buffer later means hipFree + hipMalloc (or hipHostFree + hipHostMalloc), and those wait for EVERY stream of
// the device -- measured in a batch of 8 signatures: a PairingPrecomp proof with 212 ms of device time held its context for 2.3 s
// because its buffers grew while four FinalExp proofs kept the device busy.
int ctx_reserve(Ctx* c, const AirInfo& air, const starkhip_config_t& cfg, size_t log_bytes, unsigned proof_blobs, bool device_traces) {
    ProofShape s;
    if (ProofShape::make(air, cfg, air.default_rows, &s) != STARKHIP_OK) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = ensure_tables(c, s.log_n, s.r, s.qdb)) return rc;
    if (int rc = ensure_plan(c, air, s.size, c->opt_quotient_cosets == 0 && c->opt_quotient_debug == 0 && s.mid == 0)) return rc;
    // `values`: a trace waits for its LDE inside the LDE buffer (prove(): trace_in_lde) but for the tail of run_lde_trace; rate_bits == 0
    // makes prove() ask for a whole trace.  The LDE buffer also stages the upload: a recording of log_bytes.
    const size_t values_bytes = values_bytes_for(s, s.r >= 1, false);
    // the buffers of "fill_frequencies" only for a context that has the option on: others hold nothing more than before
    const bool fill_freq = c->opt_fill_frequencies && !air.prog.logups.empty() && logup_fillable(air.prog, nullptr);
    for (const BufWant& w : work_buffers(c, s, c->plan->chunks, c->plan, values_bytes, log_bytes + 64, air.lookups.size(), fill_freq ? &air.prog : nullptr)) HIPCHK(w.b->ensure(w.bytes));
    if (int rc = ensure_long_tables(c, s)) return rc;
    if (leaf_prefix_wanted(c, s.C, s.log_n, s.r))
        if (int rc = ensure_leaf_prefix(c, s.log_n, s.r)) return rc;
    if (log_bytes && !device_traces) HIPCHK(ensure_host_staging(c, log_bytes, log_bytes));
    if (proof_blobs && !c->blob_airs.count(air.id)) {  // page-locked blobs for this AIR's proofs, once per context
        if (blob_arena_add(c, s.pl.total * 8, proof_blobs) != 0) return STARKHIP_ERR_OOM;
        c->blob_airs.insert(air.id);
    }
    return stream_wait(c) == hipSuccess ? STARKHIP_OK : STARKHIP_ERR_HIP;
}

}  // namespace starkhip
