// The prover context (ctx.h): its creation and teardown, options and accessors, the sleeping wait for its stream and the read-back
// arena, the caches it keeps -- tables per shape, the tiled plan and the op-stream program per AIR -- and what proof, trace checkers and
// test entries share on top of those: the dispatch of the LDE and NTT kernels, the dense upload, a lone context's leaf hash.
#include <hip/hip_runtime.h>

#include <atomic>
#include <time.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "blob_arena.h"
#include "ctx.h"
#include "kernels_multiset.h"
#include "quotient_ops.h"
#include "quotient_plan.h"
#include "verifier.h"

namespace starkhip {

// Wait for everything enqueued on the context's stream -- SLEEPING, not spinning: the wait goes through an event created with
// hipEventBlockingSync (an interrupt-driven wait).  With several proofs in flight every context has a host thread waiting for
// its stream most of the time; hipStreamSynchronize spins by default (hipDeviceScheduleAuto on a many-core host), and spinning
// threads eat the CPUs -- in a container with a CPU quota, the quota -- that trace generation and the other proofs' Fiat-Shamir
// hashing need.  Per event, so nothing about the device's scheduling flags changes for other libraries in the process (RCCL).
// Waiting for an event WITHOUT a CPU: hipEventSynchronize on a hipEventBlockingSync event does not sleep on this runtime -- measured with
// eight proofs in flight, 0.80 of the 0.84 CPU-seconds a context thread spends per FinalExp proof were inside that call (it yields, so it
// only shows where CPUs are idle; where they are not, it takes them from the recordings, which run at nice 10).  The device phases it
// waits for are milliseconds long, so: look a few times, then sleep in steps that grow from 20 to 200 microseconds.
hipError_t event_wait_sleeping(hipEvent_t ev) {
    for (int spin = 0; spin < 8; spin++) {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
    }
    (void)hipGetLastError();  // hipErrorNotReady is not an error (and must not surface at the next launch)
    timespec ts = {0, 20000};
    for (;;) {
        nanosleep(&ts, nullptr);
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
        (void)hipGetLastError();
        if (ts.tv_nsec < 200000) ts.tv_nsec += ts.tv_nsec / 2;
    }
}

std::atomic<uint64_t> g_wait_cpu_ns(0);       // CPU time the context threads spend INSIDE their waits for the device (should be next to nothing)
hipError_t stream_wait(Ctx* c) {
    const uint64_t cpu0 = thread_cpu_ns();
    hipError_t e = hipEventRecord(c->wait_ev, c->st);
    if (e == hipSuccess) e = event_wait_sleeping(c->wait_ev);
    g_wait_cpu_ns.fetch_add(thread_cpu_ns() - cpu0);
    for (const Ctx::Pending& p : c->rb_pending)  // the read-backs requested since the last wait have landed in the arena
        if (e == hipSuccess) memcpy(p.dst, p.src, p.bytes);
    c->rb_pending.clear();
    c->rb_used = 0;
    return e;
}

// device -> host on the context's stream, complete after the next stream_wait(c); `dst` may be pageable
hipError_t read_back(Ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (!c->rb || c->rb_used + need > c->rb_cap || st != c->st) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);  // does not fit: the direct (blocking) way
    void* slot = (char*)c->rb + c->rb_used;
    c->rb_used += need;
    const hipError_t e = hipMemcpyAsync(slot, src, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) c->rb_pending.push_back({dst, slot, bytes});
    return e;
}

int ensure_tables(Ctx* c, unsigned log_n, unsigned rate, unsigned qdb) {
    for (auto& t : c->table_cache)
        if (t->log_n == (int)log_n && t->rate == (int)rate && t->qdb == (int)qdb) {
            c->tab = t.get();
            return 0;
        }
    std::unique_ptr<Ctx::Tables> fresh(new Ctx::Tables());  // a half-built set of tables is not kept: it goes with `fresh`, buffers and all
    Ctx::Tables* T = fresh.get();
    const unsigned log_N = log_n + rate;
    const size_t N = (size_t)1 << log_N, size = (size_t)1 << (log_n + qdb), n_rows = (size_t)1 << log_n;
    HIPCHK(T->tw_fwd.ensure(N / 2 * 8 + 8));
    HIPCHK(T->tw_inv.ensure(N / 2 * 8 + 8));
    HIPCHK(T->coset_scale.ensure(N * 8));
    HIPCHK(T->qtab.ensure(4 * size * 8));
    HIPCHK(T->qshift_inv.ensure(size * 8));
    gl_t w = gl_root_of_unity(log_N);
    HIPCHK(launch_fill_powers(T->tw_fwd.as<gl_t>(), 1, w, N / 2, c->st));
    HIPCHK(launch_fill_powers(T->tw_inv.as<gl_t>(), 1, gl_inv(w), N / 2, c->st));
    HIPCHK(launch_fill_coset_scale(T->coset_scale.as<gl_t>(), log_n, rate, c->st));
    HIPCHK(launch_quotient_tables(T->qtab.as<gl_t>(), log_n, qdb, c->st));
    HIPCHK(launch_fill_powers(T->qshift_inv.as<gl_t>(), 1, gl_inv(GL_GENERATOR), size, c->st));
    if (((size_t)1 << qdb) <= QT_MAX_COSETS) {
        const std::vector<gl_t> solve = quotient_solve_table(log_n, qdb);
        HIPCHK(T->qsolve.ensure(solve.size() * 8));
        HIPCHK(hipMemcpyAsync(T->qsolve.p, solve.data(), solve.size() * 8, hipMemcpyHostToDevice, c->st));
        HIPCHK(stream_wait(c));  // `solve` goes out of scope
    }
    if (lde_v2_supported(log_n)) {
        HIPCHK(T->lde2_fwd.ensure(lde_v2_tw_words(log_n) * 8));
        HIPCHK(T->lde2_inv.ensure(lde_v2_tw_words(log_n) * 8));
        HIPCHK(T->lde2_cs.ensure(N * 8));
        HIPCHK(T->lde2_oh.ensure(std::max<size_t>(1, lde_v2_oh_words(log_n, rate)) * 8));
        HIPCHK(lde_v2_upload_tables(log_n, rate, T->lde2_fwd.as<gl_t>(), T->lde2_inv.as<gl_t>(), T->lde2_cs.as<gl_t>(), T->lde2_oh.as<gl_t>(), c->st));
        if (lde_wave_supported(log_n)) {
            HIPCHK(T->lde_wave.ensure((lde_wave_table_words(rate) + 1) * 8));  // + the launches' column counter
            HIPCHK(lde_wave_upload_tables(rate, T->lde_wave.as<gl_t>(), c->st));
        }
    }
    if (lde_long_supported(log_n)) {
        HIPCHK(T->long_cs.ensure(N * 8));
        for (size_t s = 0; s < ((size_t)1 << rate); s++)
            HIPCHK(launch_fill_powers(T->long_cs.as<gl_t>() + s * n_rows, 1, gl_mul(GL_GENERATOR, gl_pow(w, s)), n_rows, c->st));
    }
    T->log_n = log_n;
    T->rate = rate;
    T->qdb = qdb;
    c->table_cache.push_back(std::move(fresh));
    c->tab = T;
    return 0;
}

// Vectors of 2^16 .. 2^26 words go through the multi-workgroup transform (kernels_lde_long.hip; above 2^20 words in tiles narrower than a
// cache line); shorter ones stay with the one-workgroup ntt_global_kernel (no proof of up to 8192 rows changes its kernels).  So does what
// is longer still: only 2^19 rows and more at rate_bits 8 have such a vector.  Trace columns take it from 2^14 rows on (run_lde).
bool long_vector(unsigned log_len) { return log_len > 15 && lde_long_supported(log_len); }

// The long transform's tables for vectors of 2^log_len words, cached with the current shape's tables
int ensure_long_tw(Ctx* c, unsigned log_len, LdeLongTables* out) {
    Ctx::Tables* T = c->tab;
    if (!T->long_sub.p) {
        HIPCHK(T->long_sub.ensure(lde_long_sub_words() * 8));
        if (hipError_t e = lde_long_upload_sub_tables(T->long_sub.as<gl_t>(), c->st); e != hipSuccess) {
            T->long_sub.release();
            HIPCHK(e);
        }
    }
    Ctx::Tables::LongTw* tw = nullptr;
    for (auto& t : T->long_tw)
        if (t->log_len == log_len) tw = t.get();
    if (!tw) {
        std::unique_ptr<Ctx::Tables::LongTw> fresh(new Ctx::Tables::LongTw());
        fresh->log_len = log_len;
        HIPCHK(fresh->fwd.ensure(((size_t)8) << log_len));
        HIPCHK(fresh->inv.ensure(((size_t)8) << log_len));
        HIPCHK(lde_long_fill_twiddles(fresh->fwd.as<gl_t>(), fresh->inv.as<gl_t>(), log_len, c->st));
        tw = fresh.get();
        T->long_tw.push_back(std::move(fresh));
    }
    if (out) *out = LdeLongTables{T->long_sub.as<gl_t>(), tw->fwd.as<gl_t>(), tw->inv.as<gl_t>()};
    return 0;
}

// IFFT + coset LDE of `cols` columns with the tables of ensure_tables(log_n, rate, .)
hipError_t run_lde(Ctx* c, const gl_t* values, gl_t* coeffs, gl_t* lde, size_t cols, unsigned log_n, unsigned rate, int from_coeffs, unsigned col_base,
                   unsigned* unit_count) {
    // 2^14 rows and more: a column is split over workgroups; `coeffs` is that transform's scratch as well (required unless from_coeffs).
    // No closed forms for constant / unit-vector columns there ("lde_closed_forms" has nothing to switch).
    if (lde_long_supported(log_n)) {
        LdeLongTables tb;
        if (const int rc = ensure_long_tw(c, log_n, &tb)) return rc == STARKHIP_ERR_OOM ? hipErrorOutOfMemory : hipErrorUnknown;
        return launch_lde_columns_long(values, coeffs, lde, cols, log_n, rate, tb, c->tab->long_cs.as<gl_t>(), from_coeffs, c->st);
    }
    // 8192-row traces (FinalExp, ECCAgg): values -> LDE with nothing kept in between goes through the wave-resident kernel
    if (lde_wave_supported(log_n) && !coeffs && !from_coeffs && c->opt_lde_impl == 0) {
        // the launch's column counter: the last word of the table buffer, cleared in stream order before every launch
        unsigned* next = (unsigned*)(c->tab->lde_wave.as<gl_t>() + lde_wave_table_words(rate));
        if (hipError_t e = hipMemsetAsync(next, 0, sizeof(unsigned), c->st); e != hipSuccess) return e;
        return launch_lde_columns_wave(values, lde, cols, rate, c->tab->lde_wave.as<gl_t>(),
                                       (c->opt_lde_closed_forms && lde_v2_oh_words(log_n, rate)) ? c->tab->lde2_oh.as<gl_t>() : nullptr, next, c->st, col_base, unit_count);
    }
    if (lde_v2_supported(log_n))
        return launch_lde_columns_v2(values, coeffs, lde, cols, log_n, rate, c->tab->lde2_fwd.as<gl_t>(), c->tab->lde2_inv.as<gl_t>(),
                                     c->tab->lde2_cs.as<gl_t>(),
                                     (c->opt_lde_closed_forms && lde_v2_oh_words(log_n, rate)) ? c->tab->lde2_oh.as<gl_t>() : nullptr, from_coeffs, c->st, col_base,
                                     unit_count);
    return launch_lde_columns(values, coeffs, lde, cols, log_n, rate, c->tab->tw_fwd.as<gl_t>(), c->tab->tw_inv.as<gl_t>(), log_n + rate,
                              c->tab->coset_scale.as<gl_t>(), from_coeffs, c->st);
}

// ---- the leaf hash's saved state past an identity prefix (kernels.h: LeafPrefix; declarations and what each is for: ctx.h)
bool leaf_prefix_wanted(const Ctx* c, size_t n_cols, unsigned log_n, unsigned rate) {
    return c->opt_leaf_hash_prefix && c->opt_hasher == STARKHIP_HASHER_POSEIDON && (log_n == 12 || log_n == 13) && leaf_prefix_words(log_n, rate) != 0 &&
           n_cols >= ((size_t)1 << log_n) + 8;
}
size_t leaf_prefix_bytes(const Ctx* c, size_t n_cols, unsigned log_n, unsigned rate) {
    return leaf_prefix_wanted(c, n_cols, log_n, rate) ? (leaf_prefix_words(log_n, rate) + 1) * 8 : 0;
}
int ensure_leaf_prefix(Ctx* c, unsigned log_n, unsigned rate) {
    Ctx::Tables* T = c->tab;
    if (T->leaf_prefix_built) return 0;
    const size_t words = leaf_prefix_words(log_n, rate);
    if (!words || T->log_n != (int)log_n || T->rate != (int)rate) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(T->leaf_prefix.ensure((words + 1) * 8));
    HIPCHK(hipMemsetAsync(T->leaf_prefix.as<gl_t>() + words, 0, 8, c->st));
    HIPCHK(launch_leaf_prefix_build(T->lde2_oh.as<gl_t>(), log_n, rate, T->leaf_prefix.as<gl_t>(), c->st));
    T->leaf_prefix_built = true;
    return 0;
}
unsigned* leaf_prefix_counter(const Ctx* c) {
    const Ctx::Tables* T = c->tab;
    return T && T->leaf_prefix_built ? (unsigned*)(T->leaf_prefix.as<gl_t>() + leaf_prefix_words((unsigned)T->log_n, (unsigned)T->rate)) : nullptr;
}
hipError_t leaf_prefix_reset(Ctx* c) {
    unsigned* const count = leaf_prefix_counter(c);
    return count ? hipMemsetAsync(count, 0, sizeof(unsigned), c->st) : hipSuccess;
}
LeafPrefix leaf_prefix(const Ctx* c) {
    LeafPrefix p;
    if (unsigned* const count = leaf_prefix_counter(c)) {
        p.count = count;
        p.cap = c->tab->leaf_prefix.as<gl_t>();
    }
    return p;
}

int ensure_program(Ctx* c, const AirInfo& air, size_t quotient_points) {
    // enough (point-block x chunk) waves to fill 256 CUs several times over
    size_t blocks = (quotient_points + 63) / 64;
    size_t target_waves = (size_t)std::max(64L, c->opt_quotient_waves);  // measured on FinalExp: 8 K waves 61.3 ms, 16 K 56.4, 32 K 54.3, 64 K 53.5, 128 K 52.9
    unsigned want = (unsigned)std::min<size_t>(256, std::max<size_t>(1, (target_waves + blocks - 1) / blocks));
    want = (unsigned)std::min<size_t>(want, air.prog.group_off.size());
    if (c->prog.air == air.id && c->prog.chunks == want) return 0;
    QProgram Q = compile_quotient_ops(air.prog, want);
    want = (unsigned)Q.chunk_k_after.size();
    // per-wave LDS cell cache, OFF by default: measured on FinalExp (MI355X) 0 slots 40 ms, 16: 44, 32: 67, 48: 94 ms.
    // The kernel is bound by memory (253 GB fetched per launch, 6.1 TB/s) and its throughput is proportional to the waves
    // in flight; Belady replacement would hit 38 / 56 / 64 % with 16 / 32 / 64 slots, but the LDS those slots take costs more
    // occupancy than the hits return.  Option "quotient_slots" (0..64) keeps the path testable.
    c->prog.slots = (unsigned)std::min(64L, std::max(0L, c->opt_quotient_slots));
    attach_cell_cache(Q, c->prog.slots);
    HIPCHK(c->prog.loads.ensure(Q.loads.size() * 4));
    HIPCHK(hipMemcpyAsync(c->prog.loads.p, Q.loads.data(), Q.loads.size() * 4, hipMemcpyHostToDevice, c->st));
    c->prog.chunk_k_after = Q.chunk_k_after;
    HIPCHK(c->prog.ops.ensure(Q.ops.size() * sizeof(QOp)));
    HIPCHK(hipMemcpyAsync(c->prog.ops.p, Q.ops.data(), Q.ops.size() * sizeof(QOp), hipMemcpyHostToDevice, c->st));
    HIPCHK(c->prog.chunk_off.ensure(Q.chunk_batch.size() * 4));
    HIPCHK(hipMemcpyAsync(c->prog.chunk_off.p, Q.chunk_batch.data(), Q.chunk_batch.size() * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(stream_wait(c));  // Q goes out of scope
    c->prog.air = air.id;
    c->prog.chunks = want;
    return 0;
}

// Tiled plan of `air` on the device.  Chunks: enough (64-point block x chunk) workgroups to fill 256 CUs several times over.
// by_class: the plans of the classes and the cosets' work rows (QTClassPlan), else one plan for every coset.
int ensure_plan(Ctx* c, const AirInfo& air, size_t quotient_points, bool by_class) {
    const size_t blocks = (quotient_points + 63) / 64;
    unsigned want = (unsigned)std::min<size_t>(512, std::max<size_t>(1, (8192 + blocks - 1) / blocks));  // FinalExp: 4 chunks 29.8 ms, 8: 29.4, 16: 29.0, 32: 28.9
    if (c->opt_quotient_chunks > 0) want = (unsigned)c->opt_quotient_chunks;
    by_class = by_class && quotient_factor(air.prog.degree) <= QT_MAX_ACCS;  // the kernel holds that many pairs of sums
    for (auto& pd : c->plan_cache)
        if (pd->air == air.id && pd->want == want && pd->by_class == by_class) {
            c->plan = pd.get();
            return 0;
        }
    QTClassPlan CP;
    const unsigned n_cosets = 1u << quotient_degree_bits(air.prog.degree);
    if (by_class) CP = build_quotient_class_plan(air.prog, want, quotient_factor(air.prog.degree), n_cosets);
    else CP.plan = build_quotient_plan(air.prog, want);
    const QTPlan& Q = CP.plan;
    std::vector<uint32_t> vec_slot, vec_of((size_t)CP.n_cosets * (CP.n_classes + 1) + 1, 0xFFFFFFFFu);  // the (coset, slot) pairs that run, in order, and back
    for (unsigned t = 0; t < CP.n_cosets; t++)
        for (unsigned s = 0; s <= CP.n_classes; s++)
            if (t < CP.n_classes ? (s >= t && s < CP.n_classes) : s == CP.n_classes) {
                vec_of[t * (CP.n_classes + 1) + s] = (uint32_t)vec_slot.size();
                vec_slot.push_back(t * (CP.n_classes + 1) + s);
            }
    std::unique_ptr<Ctx::PlanDev> fresh(new Ctx::PlanDev());
    Ctx::PlanDev* D = fresh.get();
    struct Up { DevBuf* b; const void* src; size_t bytes; };
    const std::vector<gl_t>& consts = air.prog.consts;
    const gl_t zero = 0;
    auto words = [&](const std::vector<uint32_t>& v) { return v.empty() ? (const void*)&zero : (const void*)v.data(); };
    const Up ups[] = {{&D->q_work, CP.work.empty() ? (const void*)&zero : (const void*)CP.work.data(), std::max<size_t>(1, CP.work.size()) * sizeof(QTClassPlan::Work)},
                      {&D->q_sum_off, words(CP.coset_chunk_off), std::max<size_t>(1, CP.coset_chunk_off.size()) * 4},
                      {&D->q_vec_slot, words(vec_slot), std::max<size_t>(1, vec_slot.size()) * 4},
                      {&D->q_vec_of, words(vec_of), std::max<size_t>(1, vec_of.size()) * 4},
                      {&D->q_recs, Q.recs.data(), Q.recs.size() * sizeof(QTRec)},
                      {&D->q_streams, Q.streams.data(), Q.streams.size() * sizeof(QTStream)},
                      {&D->q_chunk_tile_off, Q.chunk_tile_off.data(), Q.chunk_tile_off.size() * 4},
                      {&D->q_tile_list, Q.tile_list.empty() ? (const void*)&zero : (const void*)Q.tile_list.data(), std::max<size_t>(1, Q.tile_list.size()) * 4},
                      {&D->q_contrib_off, Q.contrib_off.data(), Q.contrib_off.size() * 4},
                      {&D->q_contribs, Q.contribs.empty() ? (const void*)&zero : (const void*)Q.contribs.data(), std::max<size_t>(1, Q.contribs.size()) * sizeof(QTContrib)},
                      {&D->q_consts, consts.empty() ? (const void*)&zero : (const void*)consts.data(), std::max<size_t>(1, consts.size()) * 8}};
    for (const Up& u : ups) {
        HIPCHK(u.b->ensure(u.bytes));
        HIPCHK(hipMemcpyAsync(u.b->p, u.src, u.bytes, hipMemcpyHostToDevice, c->st));
    }
    HIPCHK(D->q_apow.ensure(std::max<size_t>(1, air.prog.n_constraints) * 16));
    HIPCHK(stream_wait(c));  // Q goes out of scope
    D->air = air.id;
    D->want = want;
    D->by_class = by_class;
    D->n_work = (unsigned)CP.work.size();
    D->n_vecs = (unsigned)vec_slot.size();
    D->n_classes = CP.n_classes;
    D->chunks = Q.n_chunks;
    D->recs = (uint32_t)Q.recs.size();
    c->plan_cache.push_back(std::move(fresh));
    c->plan = D;
    return 0;
}

// Which leaf-hash form a LONE context uses (a pool's commitments go through its scheduler, which merges the small ones into quad
// launches): the quad form of a commitment with <= 4096 leaves is at most 256 waves on 1024 SIMDs, each a chain of up to 12 167
// sequential permutations, so the form with fewer instructions per wave and permutation wins (MillerLoop 119 -> ms, kernels_hash.hip).
static bool use_row_form(const Ctx* c, size_t n_cols, unsigned log_N) {
    if (c->opt_leaf_hash_form == FORM_QUAD) return false;
    if (c->opt_leaf_hash_form == FORM_ROW) return true;
    if (c->opt_leaf_hash_form == FORM_LANE || c->opt_leaf_hash_form == FORM_PAIR) return false;
    return log_N <= 12 && n_cols >= 64;
}
// The pair form (two lanes per leaf, 256 registers per wave) fills the chip from 32 768 leaves on: 1 024 waves, one per SIMD.
static bool use_pair_form(const Ctx* c, size_t n_cols, unsigned log_N) {
    if (c->opt_leaf_hash_form == FORM_PAIR) return true;
    if (c->opt_leaf_hash_form != FORM_AUTO) return false;
    return log_N >= 15 && n_cols >= 64;
}

// The one teardown: a context's device buffers, events, page-locked memory and streams, then the context itself.  Members never
// created are skipped, so ctx_create's failure branch ends here as ctx_destroy does.
static void ctx_release(Ctx* c) {
    for (DevBuf* b : c->dev_bufs()) b->release();
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->kev)
        if (e) (void)hipEventDestroy(e);
    if (c->rb) (void)hipHostFree(c->rb);
    for (hipEvent_t e : {c->hash_ready, c->hash_done, c->wait_ev, c->hash_timing.t0, c->hash_timing.t1, c->col_ev[0], c->col_ev[1]})
        if (e) (void)hipEventDestroy(e);
    if (c->host_staging) (void)hipHostFree(c->host_staging);
    blob_arena_drop(c);
    if (c->st_normal) (void)hipStreamDestroy(c->st_normal);
    if (c->st_high) (void)hipStreamDestroy(c->st_high);
    delete c;
}

int ctx_create(int device, Ctx** out, int priority) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return STARKHIP_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return STARKHIP_ERR_NO_DEVICE;
    HIPCHK(hipSetDevice(device));
    Ctx* c = new Ctx();
    c->device = device;
    bool ok;
    if (priority) {  // +1: the highest stream priority of the device, -1: the lowest (pooled contexts, starkhip_pool_config_t)
        int least = 0, greatest = 0;
        ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess &&
             hipStreamCreateWithPriority(&c->st_normal, hipStreamDefault, priority > 0 ? greatest : least) == hipSuccess;
    } else {
        ok = hipStreamCreate(&c->st_normal) == hipSuccess;
    }
    c->st = c->st_normal;
    for (auto& e : c->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    for (auto& e : c->kev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->hash_ready, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->hash_done, hipEventDisableTiming | hipEventBlockingSync) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->wait_ev, hipEventDisableTiming | hipEventBlockingSync) == hipSuccess;
    ok = ok && hipEventCreate(&c->hash_timing.t0) == hipSuccess && hipEventCreate(&c->hash_timing.t1) == hipSuccess;
    if (ok && hipHostMalloc(&c->rb, (size_t)8 << 20, hipHostMallocDefault) == hipSuccess) c->rb_cap = (size_t)8 << 20;  // (without it read-backs go the direct way)
    else c->rb = nullptr;
    if (!ok) {  // release whatever was created
        ctx_release(c);
        return STARKHIP_ERR_HIP;
    }
    *out = c;
    return 0;
}

void ctx_destroy(Ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    ctx_release(c);
}
void ctx_attach_hash_service(Ctx* c, HashService* hs) { c->hs = hs; }
// The next proofs of this context run on a high-priority stream (urgent = true) or on its ordinary one.  Between proofs only:
// a context's stream is idle then.
int ctx_set_urgent(Ctx* c, bool urgent) {
    if (urgent && !c->st_high) {
        HIPCHK(hipSetDevice(c->device));
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(&c->st_high, hipStreamDefault, greatest));
    }
    c->st = urgent ? c->st_high : c->st_normal;
    c->urgent = urgent;
    return STARKHIP_OK;
}
bool ctx_has_hash_service(Ctx* c) { return c->hs != nullptr; }
void ctx_hash_request_reset(Ctx* c) { c->hash_requested = false; }
bool ctx_hash_requested(Ctx* c) { return c->hash_requested; }

int ctx_set_option(Ctx* c, const char* name, long value) {
    if (!c || !name) return STARKHIP_ERR_BAD_SHAPE;
    const std::string k(name);
    if (k == "quotient_impl" && (value == 0 || value == 1)) c->opt_quotient_impl = value;
    else if (k == "quotient_waves" && value >= 64) { c->opt_quotient_waves = value; c->prog.air = -1; }
    else if (k == "quotient_slots" && value >= 0 && value <= 64) { c->opt_quotient_slots = value; c->prog.air = -1; }
#ifdef STARKHIP_DEBUG  // make DEBUG_KNOBS=1 only: modes 1..4, 8 switch arithmetic off (timing decomposition; the proof is then WRONG and
                       // prove() refuses to return it), 9 compares the two evaluators point by point on stderr
    else if (k == "quotient_debug" && value >= 0 && value <= 9) c->opt_quotient_debug = value;
#endif
    else if (k == "zeta_on_coset" && value >= 0) c->opt_zeta_on_coset = value;  // tests: substitute zeta = 7 w_n^(value - 1); the proof is not a transcript any more
    else if (k == "lde_closed_forms" && (value == 0 || value == 1)) c->opt_lde_closed_forms = value;
    else if (k == "lde_impl" && (value == 0 || value == 1)) c->opt_lde_impl = value;
    else if (k == "leaf_hash_prefix" && (value == 0 || value == 1)) c->opt_leaf_hash_prefix = value;
    else if (k == "host_commit_leaves" && value >= 0 && value <= 4096) c->opt_host_commit_leaves = value;
    else if (k == "leaf_hash_form" && value >= FORM_AUTO && value <= FORM_PAIR) c->opt_leaf_hash_form = value;
    else if (k == "quotient_cosets" && (value == 0 || value == 1)) c->opt_quotient_cosets = value;
    else if (k == "quotient_chunks" && value >= 0 && value <= 4096) c->opt_quotient_chunks = value;  // plans are cached by (AIR, chunks)
    else if (k == "verify_chunk_mb" && value >= 1) c->opt_verify_chunk_mb = value;
    else if (k == "hasher" && value >= STARKHIP_HASHER_POSEIDON && value <= STARKHIP_HASHER_KECCAK) c->opt_hasher = value;
    else if (k == "check_trace" && (value == 0 || value == 1)) c->opt_check_trace = value;
    else if (k == "check_trace_list" && value >= 0 && value <= (long)STARKHIP_CHECK_LIST_MAX) c->opt_check_trace_list = value;
    else if (k == "fill_lookups" && (value == 0 || value == 1)) c->opt_fill_lookups = value;
    else if (k == "lookup_batch" && value >= 0 && value <= (long)STARKHIP_LOOKUPS_MAX) c->opt_lookup_batch = value;
    else if (k == "fill_frequencies" && (value == 0 || value == 1)) c->opt_fill_frequencies = value;
    else if (k == "logup_count_combine" && (value == 0 || value == 1)) c->opt_logup_count_combine = value;
    else return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}
void ctx_set_check_trace(Ctx* c, bool on, size_t list_cap) {
    c->opt_check_trace = on;
    c->opt_check_trace_list = (long)std::min<size_t>(list_cap, STARKHIP_CHECK_LIST_MAX);
}
void ctx_set_fill_lookups(Ctx* c, bool on) { c->opt_fill_lookups = on; }
void ctx_set_fill_frequencies(Ctx* c, bool on) { c->opt_fill_frequencies = on; }
void ctx_set_hasher(Ctx* c, int hasher) { c->opt_hasher = hasher; }
void ctx_check_stats(Ctx* c, uint64_t out[2]) {
    out[0] = c->traces_checked.load();
    out[1] = c->traces_rejected.load();
}
size_t ctx_device_bytes(Ctx* c) {
    size_t total = 0;
    for (DevBuf* b : c->dev_bufs()) total += b->cap;
    return total;
}
size_t ctx_pinned_bytes(Ctx* c) { return c->host_staging_cap + c->rb_cap; }
const float* ctx_timings(Ctx* c) { return c->timings; }
long ctx_verify_chunk_mb(Ctx* c) { return c->opt_verify_chunk_mb; }
double* ctx_verify_timings(Ctx* c) { return c->verify_timings; }
int ctx_device(Ctx* c) { return c->device; }
const float* ctx_kernel_timings(Ctx* c) { return c->ktimings; }
const float* ctx_host_timings(Ctx* c) { return c->htimings; }
void ctx_commit_info(Ctx* c, int* form, unsigned* group) {
    *form = c->hash_timing.form;
    *group = c->hash_timing.group;
}

// The context's page-locked upload staging holds at least `need` bytes; where it does not, it is replaced by one of `grow_to` (>= need)
// bytes -- hipHostFree + hipHostMalloc wait for the device, so every caller grows by its own policy to make that rare
hipError_t ensure_host_staging(Ctx* c, size_t need, size_t grow_to) {
    if (c->host_staging_cap >= need) return hipSuccess;
    if (c->host_staging) (void)hipHostFree(c->host_staging);
    c->host_staging = nullptr;
    c->host_staging_cap = 0;
    const hipError_t e = hipHostMalloc(&c->host_staging, grow_to, hipHostMallocDefault);
    if (e == hipSuccess) c->host_staging_cap = grow_to;
    return e;
}

std::vector<LogPiece> recording_pieces(const TraceLog& log) {
    const size_t nw = log.total_words(), nr = log.total_records();
    std::vector<LogPiece> pieces;
    size_t at_r = 0, at_z = 0;
    log.for_each_part([&](const TraceLog& part) {
        if (!part.words.empty()) pieces.push_back({part.base, part.words.data(), part.words.size()});
        if (!part.offsets.empty()) pieces.push_back({nw + at_r, part.offsets.data(), part.offsets.size()});
        if (!part.late_zeros.empty()) pieces.push_back({nw + nr + at_z, part.late_zeros.data(), part.late_zeros.size()});
        at_r += part.offsets.size();
        at_z += part.late_zeros.size();
    });
    return pieces;
}

// A dense trace of n rows x C columns into column-major device memory: `*d_values` is where it is afterwards -- `dst`, or the caller's
// own column-major device memory (read only).  Row-major host rows go up into the start of the LDE buffer (idle until the LDE kernel
// writes it; C n words) and are transposed from there.
int upload_dense(Ctx* c, const TraceInput& in, gl_t* dst, const gl_t** d_values) {
    const size_t n = in.n_rows, C = in.n_cols;
    *d_values = dst;
    if (in.callers_columns()) *d_values = in.words;
    else if (in.on_device) HIPCHK(launch_transpose(in.words, dst, n, C, c->st));
    else if (in.form == TraceForm::ColMajor) HIPCHK(hipMemcpyAsync(dst, in.words, C * n * 8, hipMemcpyHostToDevice, c->st));
    else {
        HIPCHK(hipMemcpyAsync(c->lde.p, in.words, C * n * 8, hipMemcpyHostToDevice, c->st));
        HIPCHK(launch_transpose(c->lde.as<gl_t>(), dst, n, C, c->st));
    }
    return 0;
}

// The sorted (key, idx) items of `sets` sets of equal size on the context (c->mset.keys / idx / table; kernels_multiset.h has the kernels
// and how the sets lie strided in them).  reserve: room for sets of `items` each: each of keys and idx is the sort's two buffers, the
// digit tables are followed by their chunk sums.  run: the keys of the 2 n items of each set -- set y's descriptor at desc + y *
// desc_stride -- over `cols` under `seed` (launch_multiset_keys_batch) and their stable sort, enqueued on the context's stream; *keys
// and *idx are where the sorted items of set 0 lie, set y's 2 n items further each.  One set is what the permutation check takes.
int sorted_items_reserve(Ctx* c, size_t items, size_t sets) {
    HIPCHK(c->mset.keys.ensure(2 * sets * items * 8));
    HIPCHK(c->mset.idx.ensure(2 * sets * items * 4));
    HIPCHK(c->mset.table.ensure(sets * (multiset_table_words(items) + multiset_scan_chunks(items)) * 4));
    return 0;
}
int sorted_items_run(Ctx* c, const uint32_t* desc, const gl_t* cols, size_t stride, size_t n, gl_t seed, const gl_t** keys, const uint32_t** idx, size_t sets,
                     uint32_t desc_stride) {
    const size_t items = 2 * n;
    gl_t* k = c->mset.keys.as<gl_t>();
    uint32_t *i = c->mset.idx.as<uint32_t>(), *table = c->mset.table.as<uint32_t>();
    HIPCHK(launch_multiset_keys_batch(desc, desc_stride, sets, cols, stride, n, seed, k, i, c->st));
    HIPCHK(launch_multiset_sort_batch(k, i, k + sets * items, i + sets * items, items, sets, table, table + sets * multiset_table_words(items), c->st));
    *keys = k, *idx = i;
    return 0;
}

// The leaf hash of a LONE context's commitment in the form use_pair_form / use_row_form / "leaf_hash_form" pick; `*form` says which
// (HashService::Timing::form)
hipError_t launch_leaf_hash_lone(const Ctx* c, const gl_t* lde, size_t n_cols, unsigned log_n, unsigned rate, gl_t* digests, hipStream_t st, int* form,
                                 LeafPrefix prefix) {
    const LeafHashForm f = c->opt_leaf_hash_form == FORM_LANE ? FORM_LANE : use_pair_form(c, n_cols, log_n + rate) ? FORM_PAIR : use_row_form(c, n_cols, log_n + rate) ? FORM_ROW : FORM_QUAD;
    *form = leaf_hash_sent(f);
    return launch_leaf_hash_form(f, lde, n_cols, log_n, rate, digests, st, prefix);  // (the quad and row forms ignore the prefix)
}

// In-place transform of n_vecs vectors of 2^log_len words, vec_stride apart, as launch_ntt_global does it (inverse: tw_inv's direction and
// final_mul = 2^-log_len) -- through the multi-workgroup transform where the vectors are long, with `mid` (as many words, not `data`) between its passes
int run_ntt(Ctx* c, gl_t* data, gl_t* mid, size_t n_vecs, size_t vec_stride, unsigned log_len, bool inverse, const gl_t* pre_scale,
                   const gl_t* post_scale) {
    if (long_vector(log_len)) {
        LdeLongTables tb;
        if (int rc = ensure_long_tw(c, log_len, &tb)) return rc;
        HIPCHK(launch_ntt_long(data, mid, data, n_vecs, vec_stride, log_len, inverse, pre_scale, post_scale, tb, c->st));
        return 0;
    }
    HIPCHK(launch_ntt_global(data, n_vecs, vec_stride, log_len, inverse ? c->tab->tw_inv.as<gl_t>() : c->tab->tw_fwd.as<gl_t>(), (unsigned)c->tab->log_n + c->tab->rate,
                             pre_scale, post_scale, inverse ? gl_inv((gl_t)1 << log_len) : 1, c->st));
    return 0;
}

}  // namespace starkhip
