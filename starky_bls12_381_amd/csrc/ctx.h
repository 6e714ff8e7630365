// The prover context and what the host files around it share: Ctx and its device buffers (DevBuf), the error macro of every HIP call
// (HIPCHK), and the declarations of ctx.hip -- the sleeping wait and the read-back arena, the per-shape table cache, the per-AIR plan and
// op-stream program caches, the transform dispatch and the uploads that proof, trace checkers and test entries have in common.
// Internal to the .hip files that define prover.h's functions (ctx.hip, prover.hip, check_trace.hip, permutation_check.hip, lookup_columns.hip, kernel_entries.hip): prover.h stays
// the opaque interface for capi.cpp, the pools and the verifier.
#pragma once
#include <hip/hip_runtime.h>

#include <stdio.h>

#include <atomic>
#include <memory>
#include <set>
#include <system_error>
#include <thread>
#include <vector>

#include "airs.h"
#include "kernels.h"
#include "prover.h"
#include "scheduler.h"
#include "trace_log.h"

namespace starkhip {

#define HIPCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) {                                                                            \
            fprintf(stderr, "starkhip: HIP error %s at %s:%d (%s)\n", hipGetErrorString(_e), __FILE__, __LINE__, #expr); \
            (void)hipDeviceSynchronize(); /* pending async copies target host buffers that are about to go out of scope */ \
            return _e == hipErrorOutOfMemory ? STARKHIP_ERR_OOM : STARKHIP_ERR_HIP;                        \
        }                                                                                                  \
    } while (0)

struct DevBuf {  // device memory that goes with its owner (a Ctx, or cached tables / a plan that were never finished); not copied anywhere
    void* p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    template <class T>
    T* as() const { return (T*)p; }
};

struct Ctx {
    int device = 0;
    hipStream_t st = nullptr;       // the stream of the current proof: st_normal, or st_high for a proof the pool marks urgent
    hipStream_t st_normal = nullptr, st_high = nullptr;
    hipEvent_t ev[STARKHIP_N_PHASES + 1] = {};
    float timings[STARKHIP_N_PHASES] = {0};
    hipEvent_t kev[6] = {};       // the three heavy kernels bracketed on their own: leaf hash, quotient evaluation, trace LDE
    float ktimings[3] = {0};      // lde_columns, leaf_hash (trace), quotient_eval
    float htimings[2] = {0};      // host time inside the last prove: Fiat-Shamir hashing (the challenger's sequential sponge), other host arithmetic
    HashService* hs = nullptr;    // a pooled context's trace commitments are launched by the pool's scheduler (scheduler.h)
    hipEvent_t hash_ready = nullptr, hash_done = nullptr;
    HashService::Timing hash_timing;  // pooled: the commitment kernel's own start / stop on ITS launch stream, its form and group
    hipEvent_t wait_ev = nullptr;  // hipEventBlockingSync: see stream_wait()
    // Read-backs (caps, openings, FRI batches, the nonce) land in a page-locked arena and are copied to where prove() wants them when the
    // host next waits for the stream (read_back() / stream_wait()): hipMemcpyAsync into PAGEABLE memory does not return until the copy has
    // run, and the runtime waits for it spinning -- every context thread of a pool burned a CPU for as long as its proof's kernels ran
    // (0.84 CPU-seconds per FinalExp proof with eight in flight against 0.27 with the arena; bench.py: host.cpu_seconds_per_proof_by_role).
    void* rb = nullptr;
    size_t rb_cap = 0, rb_used = 0;
    struct Pending { void* dst; const void* src; size_t bytes; };
    std::vector<Pending> rb_pending;
    void* host_staging = nullptr;  // page-locked: a recording's parts gathered for one upload (prove()); a column table's scattered columns
    size_t host_staging_cap = 0;
    hipEvent_t col_ev[2] = {nullptr, nullptr};  // a column table: the two halves of host_staging, each free again when its copy has run
    std::set<int> blob_airs;  // AIRs this context has reserved page-locked proof blobs for (blob_arena.h)
    bool hash_requested = false;
    bool urgent = false;  // ctx_set_urgent
    // tuning (starkhip_set_option; defaults are the measured best)
    long opt_quotient_impl = 0;   // 0: tiled evaluator (quotient_plan.h), 1: op-stream interpreter (quotient_ops.h)
    long opt_quotient_cosets = 0; // 0: every constraint on the cosets its class needs (QTClassPlan), 1: every constraint on every coset
    long opt_quotient_waves = 65536, opt_quotient_slots = 0, opt_quotient_chunks = 0, opt_quotient_debug = 0, opt_zeta_on_coset = 0;
    // Shape-dependent tables and the per-AIR constraint plan are CACHED per context: a pooled context that alternates between
    // AIRs (a PairingPrecomp proof, then an FP12Mul one) finds both again instead of rebuilding the plan on the host and
    // re-allocating device buffers -- hipFree synchronises the whole device, i.e. waits for every other proof's kernels.
    struct Tables {
        int log_n = -1, rate = -1, qdb = -1;
        DevBuf tw_fwd, tw_inv, coset_scale, qtab, qshift_inv;
        DevBuf qsolve;  // quotient_solve_table: the constants of the recombination of the classes' chunks
        DevBuf lde2_fwd, lde2_inv, lde2_cs, lde2_oh;  // kernels_lde.hip tables (log_n >= 8)
        DevBuf lde_wave;                               // ... and of its wave-resident kernel (log_n == 13)
        // beside lde2_oh, from which it is built: the leaf hash's saved capacity past an identity prefix, cap[4][N], then the word in
        // which the LDE kernels count a proof's columns e_c (kernels.h: LeafPrefix).  Allocated and built for the first Poseidon-hashed
        // proof of this shape that can use it (leaf_prefix_wanted, ensure_leaf_prefix); empty otherwise.
        DevBuf leaf_prefix;
        bool leaf_prefix_built = false;
        // kernels_lde_long.hip (log_n >= 14, and the proof's other vectors of 2^16 .. 2^20 words): the coset powers (7 w_N^s)^j, the
        // sub-transforms' twiddles, and the inter-pass twiddles of every length this shape has transformed (ensure_long_tw)
        DevBuf long_cs, long_sub;
        struct LongTw { unsigned log_len; DevBuf fwd, inv; };
        std::vector<std::unique_ptr<LongTw>> long_tw;
        std::vector<DevBuf*> bufs() {
            std::vector<DevBuf*> v = {&tw_fwd, &tw_inv, &coset_scale, &qtab, &qshift_inv, &qsolve, &lde2_fwd, &lde2_inv, &lde2_cs, &lde2_oh, &lde_wave, &leaf_prefix, &long_cs, &long_sub};
            for (auto& t : long_tw) {
                v.push_back(&t->fwd);
                v.push_back(&t->inv);
            }
            return v;
        }
    };
    struct PlanDev {  // tiled plan (quotient_plan.h) of one AIR on the device
        int air = -1;
        unsigned chunks = 0, want = 0;
        uint32_t recs = 0;
        // by class (QTClassPlan): the work rows (chunk, coset), the (coset, slot) pairs that run -- each a vector of the recombination --
        // and the rows of each; by_class is part of the cache key
        bool by_class = false;
        unsigned n_work = 0, n_vecs = 0, n_classes = 0;
        DevBuf q_recs, q_streams, q_chunk_tile_off, q_tile_list, q_contrib_off, q_contribs, q_consts, q_apow, q_work, q_sum_off, q_vec_slot, q_vec_of;
        std::vector<DevBuf*> bufs() {
            return {&q_recs, &q_streams, &q_chunk_tile_off, &q_tile_list, &q_contrib_off, &q_contribs, &q_consts, &q_apow, &q_work, &q_sum_off, &q_vec_slot, &q_vec_of};
        }
    };
    std::vector<std::unique_ptr<Tables>> table_cache;
    std::vector<std::unique_ptr<PlanDev>> plan_cache;
    Tables* tab = nullptr;    // the current shape's (ensure_tables)
    PlanDev* plan = nullptr;  // the current AIR's (ensure_plan)
    long opt_leaf_hash_form = FORM_AUTO;  // a LeafHashForm (kernels.h).  0: a lone context's commitments: row form for <= 4096 leaves, pair form for >= 32 768, quad form between; 1: quad always; 2: row always; 3: lane always; 4: pair always
    long opt_hasher = 0;             // STARKHIP_HASHER_POSEIDON / _KECCAK: the hash of this context's commitments, Merkle trees, proof of work and transcript
    long opt_lde_impl = 0;           // 0: 8192-row traces take lde_columns_wave_kernel; 1: lde_columns_v2_kernel for every shape (the cross-check)
    long opt_lde_closed_forms = 1;   // constant / unit-vector columns skip their transforms (kernels_lde.hip); 0: every column is transformed
    long opt_leaf_hash_prefix = 1;   // lane and pair forms start a trace whose first n columns are e_0 .. e_{n-1} from the saved state past them (kernels.h: LeafPrefix); 0: every block is hashed
    long opt_host_commit_leaves = 64; // trace commitments of at most this many leaves (and >= 64 columns) are hashed by host threads (0: never)
    long opt_verify_chunk_mb = 1024;  // device memory one chunk of starkhip_verify_batch may take (verifier_device.cpp)
    double verify_timings[4] = {0};   // the last starkhip_verify_batch: host prelude ms, upload ms, device ms, host CPU seconds
    // "check_trace": prove() checks the trace it has uploaded against the AIR before the LDE (check_trace_in_prove) and lists up to
    // "check_trace_list" violations in the blob of a refusal; a pool sets both per job (ctx_set_check_trace).  The counters are read by
    // other threads (starkhip_pool_check_stats).
    long opt_check_trace = 0, opt_check_trace_list = 16;
    // "fill_lookups": prove() fills the permuted columns of an AIR registered with its lookups (lookup_fill_in_prove) in its own copy of
    // the trace, before the check and before the pair columns are copied aside; a pool sets it per job (ctx_set_fill_lookups).
    // "lookup_batch": at most this many lookups share one set of launches (0: as many as lookup_batch_size allows)
    long opt_fill_lookups = 0, opt_lookup_batch = 0;
    // "fill_frequencies": prove() fills the frequencies columns of a fillable AIR's LogUp lookups (logup_fill_in_prove) in its own copy
    // of the trace, at the same place; a pool sets it per job (ctx_set_fill_frequencies).  "logup_count_combine": the count kernel adds
    // equal positions of a wave as one (1, the default) or every cell alone (0: the measurement's other form; the same bytes)
    long opt_fill_frequencies = 0, opt_logup_count_combine = 1;
    std::atomic<uint64_t> traces_checked{0}, traces_rejected{0};
    std::vector<gl_t> host_lde;      // their LDE on the host
    // op-stream program (quotient_impl = 1; kept as the cross-check)
    struct OpProgram {
        int air = -1;
        unsigned chunks = 0, slots = 0;
        DevBuf ops, loads, chunk_off;  // compile_quotient_ops() + attach_cell_cache() output for `air`
        std::vector<uint32_t> chunk_k_after;
        std::vector<DevBuf*> bufs() { return {&ops, &loads, &chunk_off}; }
    } prog;
    // trace checker (starkhip_check_trace): the op stream of `air` cut for `want` chunks (`chunks` of them came out), the chunks'
    // first ops and constraints, the results
    struct CheckProgram {
        int air = -1;
        unsigned want = 0, chunks = 0;
        std::vector<uint32_t> k0;  // [chunks + 1] the chunks' first constraints on the host, then n_constraints
        DevBuf ops, meta, out, rep, list;  // the last two: starkhip_check_trace_report's (check_trace_report)
        std::vector<DevBuf*> bufs() { return {&ops, &meta, &out, &rep, &list}; }
    } chk;
    // work buffers of a proof: work_buffers() in prover.hip is the one table of their sizes (prove() and ctx_reserve() allocate from it)
    // `lde` is the one big buffer (19.3 GB for FinalExp).  Before the LDE kernel writes it, it holds everything that waits for that
    // kernel: the trace columns as its LAST quarter (the LDE goes out in launches that overwrite only columns already transformed:
    // run_lde_trace) and, at its start, the upload staging (row-major rows before the transpose, a recording's words before the
    // expansion).  Coefficients are the LDE kernel's scratch inside a column's own block and are not kept: openings and the FRI
    // combination read coset 0 of the LDE (kernels_fri.hip).  `values` is the 1/64 of the columns the last LDE launch reads (75 MB), a
    // whole trace only for rate_bits == 0, and starkhip_lde_batch's in-place values / coefficients.  Together 19.6 GB per FinalExp
    // context; rounds 1-3: values + coefficients + staging + LDE = 33.7 GB.  `staging` serves the kernel-level test entries
    // (expand_log, permute_batch, field_ops) alone.
    DevBuf staging, values, lde, digests, pis, apow, chunk_scale, partial, qclass, qvals, qcoef, qlde, qdigests, zpow, gzpow, open_local,
        open_next, open_q, ext_apow, comb_partial, comb_out, fri_coef, fri_vals, fri_rows[16], fri_digests[16], scale_tab, pow_state,
        pow_best, qidx, gather_t;
    // every device buffer the context holds, cached tables and plans included: what ctx_destroy releases and ctx_device_bytes adds up
    std::vector<DevBuf*> dev_bufs() {
        std::vector<DevBuf*> v = {&staging, &values, &lde, &digests, &pis,
                                  &apow, &chunk_scale, &partial, &qclass, &qvals, &qcoef, &qlde, &qdigests, &zpow, &gzpow, &open_local, &open_next, &open_q,
                                  &ext_apow, &comb_partial, &comb_out, &fri_coef, &fri_vals, &scale_tab, &pow_state, &pow_best, &qidx, &gather_t};
        for (DevBuf& b : fri_rows) v.push_back(&b);
        for (DevBuf& b : fri_digests) v.push_back(&b);
        for (DevBuf* b : prog.bufs()) v.push_back(b);
        for (DevBuf* b : chk.bufs()) v.push_back(b);
        for (DevBuf* b : free_chk.bufs()) v.push_back(b);
        for (DevBuf* b : perm.bufs()) v.push_back(b);
        for (DevBuf* b : mset.bufs()) v.push_back(b);
        for (DevBuf* b : lookup.bufs()) v.push_back(b);
        for (DevBuf* b : logup_freq.bufs()) v.push_back(b);
        for (auto& t : table_cache)
            for (DevBuf* b : t->bufs()) v.push_back(b);
        for (auto& d : plan_cache)
            for (DevBuf* b : d->bufs()) v.push_back(b);
        return v;
    }
    // the free-cell entries (starkhip_check_trace_free_cell_classes, starkhip_check_trace_free_cells): compile_free_cells of the op
    // stream in `chk` -- same AIR, same `want` -- and the results of the one kernel behind both: the planes [3][C][(n + 63) / 64], and
    // per_column [C][3] followed by open_rows [K].  Last, so that the work buffers stay where they were.
    struct FreeCellsProgram {
        int air = -1;
        unsigned want = 0;
        DevBuf cons, pivots, planes, class_counts;
        std::vector<DevBuf*> bufs() { return {&cons, &pivots, &planes, &class_counts}; }
    } free_chk;
    // The middle matrix of a proof.  An AIR with LogUp lookups (COMPAT.md L1 - L7) uses the same slots, its auxiliary polynomials in the
    // Zs' place: cols the named columns, desc the two descriptors and then the Zs' polynomial indices, zvals / zcoef / zlde / zdigests
    // and the openings the auxiliary matrix, scan the spans' sums followed by the closing values and the count of zero denominators
    // (chal is not used: the two challenges travel as kernel arguments).
    // permutation arguments (an AIR with permutation pairs; COMPAT.md P1 - P8), all empty otherwise -- work buffers of a proof, sized
    // by work_buffers() like the ones above: the pair columns copied aside at upload (a short trace parked in the LDE buffer is
    // overwritten by its LDE), the two descriptors (by copy slot, by trace column) and the challenges, the Zs' values, their
    // coefficients (long traces: the transform's scratch), LDE and Merkle tree, the spans' products of the prefix scan followed by
    // the closing products, and the Z openings
    struct PermBufs {
        DevBuf cols, desc, chal, zvals, zcoef, zlde, zdigests, scan, open_z, open_zn;
        std::vector<DevBuf*> bufs() { return {&cols, &desc, &chal, &zvals, &zcoef, &zlde, &zdigests, &scan, &open_z, &open_zn}; }
    } perm;
    // The sorted items of ONE set (or of a batch of lookups, strided by set) and what starkhip_check_trace_permutations keeps beside them (permutation_check.hip), grown like the ones
    // above.  keys, idx, table: the two (key, idx) buffers of the sort (48 MB at 2^20 rows) and the digit table with its chunk sums --
    // sized, split and filled by sorted_items_reserve / sorted_items_run (ctx.hip) alone, for the permutation check and the lookups
    // alike.  desc: the pairs' columns as indices into perm.cols; masks: the two masks followed by the counters.  ms: the last call's
    // timings (starkhip_perm_check_timings).
    struct MultisetBufs {
        DevBuf desc, keys, idx, table, masks;
        float ms[4] = {0, 0, 0, 0};
        std::vector<DevBuf*> bufs() { return {&desc, &keys, &idx, &table, &masks}; }
    } mset;
    // starkhip_lookup_columns and "fill_lookups" (lookup_columns.hip over kernels_lookup.hip), sized for one BATCH of G lookups
    // (lookup_batch_size) with every per-lookup buffer strided by lookup, and grown like the ones above: what the placement needs beside
    // the sorted items, which are mset's (sorted_items_run).  desc: the descriptors of lookup_columns.hip's LookupDesc; cols: the staging
    // of a trace that is not column-major device memory, [G][4][n] -- input, table, then the two output columns of a host trace; flags:
    // what each sorted position is; sums: the tile counts [G][3][tiles]; slot: the non-heads' ranks [G][n]; mask: for a batch of g <= G
    // lookups the missing rows [g][W], then their g counts.  desc_air: the registered AIR whose list `desc` holds (-1: none).  ms: the last fill's timings (starkhip_lookup_timings).
    struct LookupBufs {
        DevBuf desc, cols, flags, sums, slot, mask;
        int desc_air = -1;
        size_t desc_G = 0;  // ... cut for batches of this many
        float ms[4] = {0, 0, 0, 0};
        std::vector<DevBuf*> bufs() { return {&desc, &cols, &flags, &sums, &slot, &mask}; }
    } lookup;
    // starkhip_logup_frequencies and "fill_frequencies" (logup_frequencies.hip over kernels_logup_freq.hip), sized for one BATCH of G
    // lookups (logup_freq_batch_size) and grown like the ones above: what the count needs beside the sorted tables, which are mset's
    // (n items per distinct table of a batch).  desc: a batch's descriptors -- its table columns, {table slot, frequencies column} per
    // lookup, {column, lookup, table slot} per looked-up column; cols: the staging of a host trace, the distinct columns the fill reads
    // and then one frequencies column per lookup, [K + L][n]; count: [G][n] uint32 by sorted table position; mask: for a batch of g
    // lookups the missing rows [g][W], then the missing cells of its g lookups and of its looked-up columns, uint32.  ms: the last
    // fill's timings (starkhip_logup_frequency_timings).
    struct LogupFreqBufs {
        DevBuf desc, cols, count, mask;
        float ms[5] = {0, 0, 0, 0, 0};
        std::vector<DevBuf*> bufs() { return {&desc, &cols, &count, &mask}; }
    } logup_freq;
};

// ---- ctx.hip
hipError_t stream_wait(Ctx* c);
hipError_t read_back(Ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st);
hipError_t ensure_host_staging(Ctx* c, size_t need, size_t grow_to);
int ensure_tables(Ctx* c, unsigned log_n, unsigned rate, unsigned qdb);
bool long_vector(unsigned log_len);
int ensure_long_tw(Ctx* c, unsigned log_len, LdeLongTables* out);
int ensure_plan(Ctx* c, const AirInfo& air, size_t quotient_points, bool by_class = false);
int ensure_program(Ctx* c, const AirInfo& air, size_t quotient_points);
// col_base, unit_count: the trace LDE of a proof that may use the leaf hash's saved prefix state (else 0, null: nothing is counted)
hipError_t run_lde(Ctx* c, const gl_t* values, gl_t* coeffs, gl_t* lde, size_t cols, unsigned log_n, unsigned rate, int from_coeffs, unsigned col_base = 0,
                   unsigned* unit_count = nullptr);
// The saved prefix state (kernels.h: LeafPrefix) with the current tables (ensure_tables).  wanted: this context would use it for a trace
// of n_cols columns under `hasher`; bytes: what its buffer takes then (work_buffers: prover.hip), else 0; ensure: the buffer holds the
// table (built once, on the context's stream); the counter word, null where the buffer is not there; reset: the counter cleared in
// stream order, before the first LDE launch of a proof; leaf_prefix: what the leaf-hash launches get (nulls unless built).
bool leaf_prefix_wanted(const Ctx* c, size_t n_cols, unsigned log_n, unsigned rate);
size_t leaf_prefix_bytes(const Ctx* c, size_t n_cols, unsigned log_n, unsigned rate);
int ensure_leaf_prefix(Ctx* c, unsigned log_n, unsigned rate);
unsigned* leaf_prefix_counter(const Ctx* c);
hipError_t leaf_prefix_reset(Ctx* c);
LeafPrefix leaf_prefix(const Ctx* c);
int run_ntt(Ctx* c, gl_t* data, gl_t* mid, size_t n_vecs, size_t vec_stride, unsigned log_len, bool inverse, const gl_t* pre_scale,
            const gl_t* post_scale);
int upload_dense(Ctx* c, const TraceInput& in, gl_t* dst, const gl_t** d_values);
// the sorted (key, idx) items of one set of 2 n items in c->mset: room for them, then keys and the stable sort on the context's stream
// (`sets` sets of that size side by side, set y's descriptor at desc + y * desc_stride: the lookups of a batch)
int sorted_items_reserve(Ctx* c, size_t items, size_t sets = 1);
int sorted_items_run(Ctx* c, const uint32_t* desc, const gl_t* cols, size_t stride, size_t n, gl_t seed, const gl_t** keys, const uint32_t** idx, size_t sets = 1,
                     uint32_t desc_stride = 0);
// ---- lookup_columns.hip
// "fill_lookups": the permuted columns of every lookup of `air` written into the prover's own column-major copy of the trace, before
// anything reads it.  STARKHIP_OK when every lookup holds; STARKHIP_ERR_TRACE and the lookup blob (lookup_columns.h) otherwise.
int lookup_fill_in_prove(Ctx* c, const AirInfo& air, gl_t* d_trace, size_t n_rows, uint64_t** blob, size_t* words);
// THE sizes of the buffers a fill of `n_lookups` lookups over n_rows takes (`staged`: of a trace that is not column-major device
// memory): work_buffers()' share for a proof that fills, and what starkhip_lookup_columns allocates from
struct LookupWant { DevBuf* b; size_t bytes; };
std::vector<LookupWant> lookup_work_buffers(Ctx* c, size_t n_rows, size_t n_lookups, bool staged);
// ---- logup_frequencies.hip
// "fill_frequencies": the frequencies column of every LogUp lookup of `air` (fillable) written into the prover's own column-major copy
// of the trace, before anything reads it.  STARKHIP_OK when every lookup holds; STARKHIP_ERR_TRACE and the LogUp blob otherwise.
int logup_fill_in_prove(Ctx* c, const AirInfo& air, gl_t* d_trace, size_t n_rows, uint64_t** blob, size_t* words);
// THE sizes of the buffers a fill of the LogUp lookups of `P` over n_rows takes (`staged`: of a host trace)
std::vector<LookupWant> logup_freq_work_buffers(Ctx* c, const AirProgram& P, size_t n_rows, bool staged);
// ---- check_trace.hip
int check_trace_in_prove(Ctx* c, const AirInfo& air, const gl_t* d_trace, size_t n_rows, const uint64_t* pis, uint64_t** blob, size_t* words);
// ---- ctx.hip
hipError_t launch_leaf_hash_lone(const Ctx* c, const gl_t* lde, size_t n_cols, unsigned log_n, unsigned rate, gl_t* digests, hipStream_t st, int* form,
                                 LeafPrefix prefix = LeafPrefix());

// digest buffer: level 0 (n_leaves nodes) followed by level 1, ... ; offset of level l in nodes
static inline size_t level_off(size_t n_leaves, unsigned l) { return 2 * n_leaves - (2 * n_leaves >> l); }
static inline size_t digest_words(size_t n_leaves) { return 8 * n_leaves; }

// fn(0) .. fn(n_threads - 1) side by side: fn(0) on the calling thread, the others on helper threads created for this call; where no
// thread is to be had the calling thread does that share too
template <class F>
static void run_on_helpers(unsigned n_threads, const F& fn) {
    std::vector<std::thread> helpers;
    for (unsigned w = 1; w < n_threads; w++) {
        try {
            helpers.emplace_back(fn, w);
        } catch (const std::system_error&) {
            fn(w);
        }
    }
    fn(0);
    for (std::thread& t : helpers) t.join();
}

// Where a recording lands in the ONE array of 32-bit words that expand_trace_kernel / zero_cells_kernel read.  A log recorded by several
// threads comes in parts (trace_log.h): each part's words land at its base, then the parts' offsets (already shifted by that base) back
// to back, then their late zeros.
struct LogPiece { size_t at; const uint32_t* src; size_t words; };
std::vector<LogPiece> recording_pieces(const TraceLog& log);

}  // namespace starkhip
