// Proof pool (starkhip_pool_* of include/starkhip.h): the jobs, the threads that record and prove them, and the pool's verifier.
//
// What the reference's caller does on one thread -- generate_trace, prove, verify, six times per signature
// (/root/reference/src/aggregate_proof.rs:23-179, :304-370) -- becomes jobs of a pool: generator threads record compact
// traces (trace_log.h), one host thread per prover context proves them, and a caller only submits and waits.  The pool owns the
// commitment scheduler its contexts share (scheduler.h).
#include "pool.h"

#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <sys/resource.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <atomic>
#include <memory>
#include <new>
#include <unordered_map>

#include "blob_arena.h"
#include "proof.h"
#include "prover.h"
#include "scheduler.h"
#include "verify_service.h"

namespace starkhip {

extern std::atomic<uint64_t> g_trace_worker_cpu_ns;       // CPU time of the recordings' helper threads
static std::atomic<uint64_t> g_gen_cpu_ns(0), g_prove_cpu_ns(0);  // ... of the generator threads inside a recording, of the context threads inside prove()
void host_cpu_seconds(double out[3]) {
    out[0] = (double)(g_gen_cpu_ns.load() + g_trace_worker_cpu_ns.load()) * 1e-9;
    out[1] = (double)g_prove_cpu_ns.load() * 1e-9;
    out[2] = (double)g_wait_cpu_ns.load() * 1e-9;
}

struct Pool {
    int device = 0;
    unsigned pools_on_device = 1;  // > 1: a multi-device handle was given this ordinal several times (starkhip_pool_host_info)
    double t0 = 0;
    std::unique_ptr<HashService> hs;
    std::vector<Ctx*> big_ctx, small_ctx;
    std::mutex mu;
    std::condition_variable cv_gen, cv_big, cv_small, cv_done;
    std::deque<Job*> q_gen, q_big, q_small;
    std::unordered_map<uint64_t, Job*> jobs;
    uint64_t next_id = 1;
    bool stop = false;
    unsigned gen_threads = 0, trace_threads_cfg = 0, gen_running = 0, cpus = 1;
    size_t big_recordings_started = 0;  // under mu
    size_t big_in_gen = 0;  // FinalExp-class witness jobs queued for, or in, their recording (under mu)
    double load = 0;        // sum of air_cost over the jobs that are not done (under mu): what a multi-device handle balances
    unsigned big_open = 0;  // FinalExp-class jobs that are not done (under mu)
    unsigned waiters = 0;   // callers inside pool_wait (under mu): pool_destroy lets them leave before it frees anything
    // the pool's device verifier (verify_service.h), made at the first verify work (or when "verify_proofs" is switched on in a warmed pool)
    std::mutex vs_mu;       // creation, submission and shutdown of `vs`; taken before mu, never after it
    std::unique_ptr<VerifyService> vs;
    bool vs_closed = false;       // pool_destroy has drained it (under vs_mu)
    bool verify_proofs = false;   // under mu
    size_t verify_arena_mb = 1024;  // under mu
    unsigned long verified_proofs = 0, verify_jobs = 0;  // under mu
    bool check_traces = false;    // under mu
    size_t check_trace_list = 16; // under mu
    bool fill_lookups = false;    // under mu
    bool fill_frequencies = false;  // under mu
    int hasher = 0;               // under mu: "hasher", read at submit
    double vload = 0;       // sum of air_verify_cost over the verify jobs that are not done (under mu)
    std::map<int, int> idle_big, idle_small;                 // idle contexts by the AIR they proved last (under mu)
    unsigned stream_priority = 0;
    bool warm_device_traces = false;  // warm_up == 2: the caller's traces are column-major device memory: no trace buffers are reserved
    int gen_nice = 10;  // STARKHIP_GEN_NICE: nice value of the generator threads (0: as the rest of the process)
#ifndef STARKHIP_GEN_AHEAD
#define STARKHIP_GEN_AHEAD 1
#endif
    static constexpr size_t gen_ahead = STARKHIP_GEN_AHEAD;  // FinalExp-class recordings made beyond the ones the contexts can take at once
    bool warm = false;        // contexts reserve the pipeline's AIRs when their threads start (pool_create waits for it)
    unsigned warmed = 0;
    int warm_rc = STARKHIP_OK;
    std::vector<std::thread> threads;

    double now() const { return now_s() - t0; }

    void tell_big_queued() {  // under mu
        if (hs) hs->set_big_queued((int)(q_big.size() + big_in_gen));
    }

    void finish(Job* j, int rc) {
        std::lock_guard<std::mutex> g(mu);
        j->rc = rc;
        j->state = JobState::Done;
        j->info.t_done = now();
        if (j->kind == JOB_VERIFY) vload = std::max(0.0, vload - j->cost);
        else load = std::max(0.0, load - j->cost);
        if (j->big && big_open > 0) big_open--;
        cv_done.notify_all();
    }

    // Threads one recording may use.  The long pole -- a FinalExp-class recording -- gets three quarters of the CPU budget (its
    // 53 tasks scale to 16 threads: 212 ms on one, 25 on 16), a small AIR's a quarter of it split over the small recordings
    // under way; the prover threads' Fiat-Shamir hashing and the natives need the rest.
    int trace_threads_for_call(bool big_job) {
        if (trace_threads_cfg) return (int)trace_threads_cfg;
        if (big_job) return (int)std::min(16u, std::max(1u, cpus * 3 / 4));
        return (int)std::min(4u, std::max(1u, cpus / 4));
    }

    // a verdict of the pool's verifier: a verify job's code, or a proving job's status once its proof has been checked
    void on_verdict(Job* j, int code, double t_prelude) {
        {
            std::lock_guard<std::mutex> g(mu);
            if (j->kind == JOB_VERIFY) j->info.t_prove_start = std::max(0.0, t_prelude - t0);
            else verified_proofs++;
        }
        finish(j, code);
    }

    // hands `proof` of job j to the verifier, making it first; false (and *rc) if it cannot be made
    bool verify_submit(Job* j, const uint64_t* proof, size_t words, int* rc) {
        std::lock_guard<std::mutex> g(vs_mu);
        if (vs_closed) {
            *rc = STARKHIP_ERR_BAD_SHAPE;
            return false;
        }
        if (!vs && (*rc = make_verifier()) != STARKHIP_OK) return false;
        vs->submit(j->air, j->cfg, proof, words, j);
        return true;
    }

    int make_verifier() {  // under vs_mu
        size_t mb;
        {
            std::lock_guard<std::mutex> g(mu);
            mb = verify_arena_mb;
        }
        const unsigned threads = std::min(4u, std::max(1u, cpus / 4));
        std::unique_ptr<VerifyService> v(new VerifyService(device, mb << 20, hs->cfg.gather_ms, threads, gen_nice,
                                                           [this](void* tag, int code, double tp) { on_verdict((Job*)tag, code, tp); }));
        const int rc = v->start();
        if (rc == STARKHIP_OK) vs = std::move(v);
        return rc;
    }

    void generator_loop() {
        pthread_setname_np(pthread_self(), "starkhip-gen");
        // Recording is the work that can wait: whenever the process is short of CPUs (16 per GPU on the measured boxes, and a batch
        // starts with four FinalExp recordings' worth of threads), the threads that feed the GPU -- the contexts' own: gathering a
        // recording for its upload, the challenger's hashing between two kernels -- must run first.  Per-thread nice value, inherited
        // by the recording's worker threads; measured on a batch of 8: the first FinalExp proofs' upload phase (the gather of a 153 MB recording) 90 - 127 -> 10 - 13 ms,
        // 3.88 -> 3.93 signatures/s over three alternating pairs.
        if (gen_nice > 0) (void)setpriority(PRIO_PROCESS, (id_t)syscall(SYS_gettid), gen_nice);
        while (true) {
            Job* j;
            int tt;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_gen.wait(lk, [&] { return stop || !q_gen.empty(); });
                if (q_gen.empty()) return;
                auto it = pick_recording(q_gen, big_recordings_started, big_ctx.size() + gen_ahead);
                j = *it;
                q_gen.erase(it);
                if (j->big) big_recordings_started++;
                tt = trace_threads_for_call(j->big);
                gen_running++;
                j->info.t_generate_start = now();
            }
            const uint64_t cpu0 = thread_cpu_ns();
            const int rc = record_witness(j, tt);
            g_gen_cpu_ns.fetch_add(thread_cpu_ns() - cpu0);
            if (rc != STARKHIP_OK) {
                {
                    std::lock_guard<std::mutex> g(mu);
                    gen_running--;
                    if (j->big && big_in_gen > 0) big_in_gen--;
                    tell_big_queued();
                    j->info.t_generate_end = now();
                }
                finish(j, rc);
                cv_big.notify_all();  // contexts that are shutting down re-check whether a generator may still feed them
                cv_small.notify_all();
                continue;
            }
            std::lock_guard<std::mutex> g(mu);
            gen_running--;
            j->info.t_generate_end = now();
            const AirInfo* a = air_get(j->air);
            j->kind = JOB_PROVE;
            j->in = j->own_log ? TraceInput::recording(j->own_log) : TraceInput::dense(j->own_rows.data(), a->default_rows, a->cols, 0, 0);
            j->pis = j->own_pis.data();
            j->n_pis = j->own_pis.size();
            if (j->big && big_in_gen > 0) big_in_gen--;
            (j->big ? q_big : q_small).push_back(j);
            cv_big.notify_all();
            cv_small.notify_all();
            // (the count of big jobs that have not started is unchanged: from recording to queued)
        }
    }

    // every context brings up what the BLS pipeline's AIRs of its class need, all contexts in parallel
    void warm_up(Ctx* c, bool big) {
        // proof blobs: a context's last proof is usually still with the caller when the next one ends, hence two per big context;
        // the small contexts' MillerLoop-sized blob (69 MB) also serves FP12Mul (42 MB) -- blob_alloc takes the smallest that fits
        static const struct { int air; size_t log_bytes; unsigned blobs; } BIG[] = {{STARKHIP_AIR_FINAL_EXP, (size_t)200 << 20, 2}},
            SMALL[] = {{STARKHIP_AIR_MILLER_LOOP, (size_t)110 << 20, 1}, {STARKHIP_AIR_PAIRING_PRECOMP, (size_t)44 << 20, 1}, {STARKHIP_AIR_FP12_MUL, (size_t)2 << 20, 0}};
        const char* pe = getenv("STARKHIP_PINNED_PROOFS");
        const bool pinned = !(pe && *pe == '0');
        int rc = STARKHIP_OK;
        auto one = [&](int air, size_t log_bytes, unsigned blobs) {
            const AirInfo* a = air_get(air);
            starkhip_config_t cfg;
            if (!a || starkhip_config_for_air((starkhip_air_t)air, &cfg) != STARKHIP_OK) return;
            try {
                const int r = ctx_reserve(c, *a, cfg, log_bytes, pinned ? blobs : 0, warm_device_traces);
                if (r != STARKHIP_OK) rc = r;
            } catch (const std::exception&) {
                rc = STARKHIP_ERR_OOM;
            }
        };
        if (big) for (const auto& w : BIG) one(w.air, w.log_bytes, w.blobs);
        else for (const auto& w : SMALL) one(w.air, w.log_bytes, w.blobs);
        std::lock_guard<std::mutex> g(mu);
        if (rc != STARKHIP_OK && warm_rc == STARKHIP_OK) warm_rc = rc;
        warmed++;
        cv_done.notify_all();
    }

    // one proof on context `c` between its hand-overs to the commitment scheduler; leaves the timings in the job and frees its recording
    int prove_job(Ctx* c, Job* j, bool big, bool announce_big) {
        int rc;
        const bool announce = !big && ctx_has_hash_service(c) && j->hasher == STARKHIP_HASHER_POSEIDON;
        if (announce) hs->announce_small();
        ctx_hash_request_reset(c);
        const uint64_t cpu0 = thread_cpu_ns();
        ctx_set_check_trace(c, j->check, j->check_list);
        ctx_set_fill_lookups(c, j->fill);
        ctx_set_fill_frequencies(c, j->fill_freq);
        ctx_set_hasher(c, j->hasher);
        try {
            const AirInfo* a = air_get(j->air);
            rc = prove(c, *a, j->cfg, j->in, j->pis, j->n_pis, j->pow, &j->proof, &j->words);
        } catch (const std::bad_alloc&) {
            rc = STARKHIP_ERR_OOM;
        } catch (const std::exception&) {
            rc = STARKHIP_ERR_BAD_SHAPE;
        }
        g_prove_cpu_ns.fetch_add(thread_cpu_ns() - cpu0);
        if (announce && !ctx_hash_requested(c)) hs->abandon_small();  // failed before its commitment: do not hold the window open
        if (announce_big && !ctx_hash_requested(c)) hs->abandon_big();
        if (big) {
            std::lock_guard<std::mutex> g(mu);
            if (big_recordings_started > 0) big_recordings_started--;  // a context is free again: the next FinalExp-class recording moves up
        }
        memcpy(j->info.phase_ms, ctx_timings(c), sizeof j->info.phase_ms);
        memcpy(j->info.kernel_ms, ctx_kernel_timings(c), sizeof j->info.kernel_ms);
        memcpy(j->info.host_ms, ctx_host_timings(c), sizeof j->info.host_ms);
        ctx_commit_info(c, &j->info.leaf_hash_form, &j->info.leaf_hash_group);
        if (j->own_log) {
            starkhip_trace_log_free(j->own_log);
            j->own_log = nullptr;
            j->in = TraceInput();
        }
        return rc;
    }

    void prover_loop(Ctx* c, bool big) {
        pthread_setname_np(pthread_self(), big ? "starkhip-ctx" : "starkhip-ctxs");
        std::deque<Job*>& q = big ? q_big : q_small;
        std::condition_variable& cv = big ? cv_big : cv_small;
        std::map<int, int>& idle = big ? idle_big : idle_small;
        int last_air = -1;
        bool urgent = false, announce_big = false;
        if (warm) warm_up(c, big);
        while (true) {
            Job* j = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                idle[last_air]++;
                while (true) {
                    if (!q.empty()) {
                        auto it = pick_job(q, last_air, idle, big);
                        if (it != q.end()) {
                            j = *it;
                            q.erase(it);
                            break;
                        }
                    } else if (stop && q_gen.empty() && gen_running == 0) {
                        // (a witness job still queued for, or in, its recording lands in q_big / q_small later: "runs what is queued
                        // to the end first" holds for those too, so a context leaves only when no generator can hand it anything)
                        idle[last_air]--;
                        return;
                    }
                    // shutting down: the queue may drain through other contexts without another notification
                    if (stop) cv.wait_until(lk, std::chrono::system_clock::now() + std::chrono::milliseconds(20));
                    else cv.wait(lk);
                }
                idle[last_air]--;
                last_air = j->air;
                j->state = JobState::Running;
                j->info.t_prove_start = now();
                // stream_priority 1: the LAST wave of FinalExp-class proofs -- no more of them waiting than there are contexts --
                // is the tail every other proof has finished before; it runs on high-priority streams.  The first wave does not:
                // strict priority starves the small proofs (a MillerLoop upload measured at 2 s behind four urgent FinalExp proofs)
                // (big jobs still queued for, or in, their recording count as waiting: with submit_witness they trickle into q_big
                // one at a time, and q_big alone would make the FIRST wave look like the last)
                urgent = big && stream_priority == 1 && q.size() + big_in_gen < big_ctx.size();
                // announced BEFORE it stops counting as queued: between the two a waiting lane group would see nobody on the way
                // and go out short, and this proof's commitment would follow it alone
                announce_big = big && ctx_has_hash_service(c) && j->hasher == STARKHIP_HASHER_POSEIDON;
                if (announce_big) hs->announce_big();
                if (big) tell_big_queued();
            }
            if (big && stream_priority == 1) (void)ctx_set_urgent(c, urgent);
            int rc = prove_job(c, j, big, announce_big);
            // "verify_proofs": the context is free already; the job waits for its verdict on the host blob the caller will receive
            // (a trace its context refused -- STARKHIP_ERR_TRACE, j->proof its check blob -- never gets there)
            if (rc == STARKHIP_OK && j->verify) {
                {
                    std::lock_guard<std::mutex> g(mu);
                    j->state = JobState::Verifying;
                }
                if (verify_submit(j, j->proof, j->words, &rc)) continue;
            }
            finish(j, rc);
        }
    }
};

int pool_create(const starkhip_pool_config_t& cfg_in, Pool** out, unsigned cpu_share) {
    starkhip_pool_config_t cfg = cfg_in;
    std::unique_ptr<Pool> p(new Pool());
    p->device = cfg.device;
    p->t0 = now_s();
    const unsigned n_big = cfg.big_contexts ? cfg.big_contexts : 3, n_small = cfg.small_contexts ? cfg.small_contexts : 16;
    // recording is host work the GPU waits for, but the CPU budget is shared with the prover threads (Fiat-Shamir hashing, kernel
    // launches): a quarter of the budget in recordings at once (at least 3), each on a few threads (trace_threads_for_call)
    p->cpus = std::max(1u, cpu_budget() / std::max(1u, cpu_share));  // cpu_share: pools of one multi-device handle share the process's CPUs
    // (the floor of three is capped by the budget itself: eight pools of a multi-device handle on sixteen CPUs plan with two each, and
    // three generator threads apiece would be 24 recording threads on those sixteen)
    p->gen_threads = cfg.generator_threads ? cfg.generator_threads : std::min(12u, std::max(std::min(3u, p->cpus), p->cpus / 4));
    p->trace_threads_cfg = cfg.trace_threads;
    int rc = STARKHIP_OK;
    for (unsigned i = 0; i < n_big + n_small && rc == STARKHIP_OK; i++) {
        Ctx* c = nullptr;
        const bool is_big = i < n_big;
        const int prio = cfg.stream_priority == 3 ? (is_big ? 1 : 0) : cfg.stream_priority == 2 ? (is_big ? 0 : 1) : 0;
        rc = ctx_create(cfg.device, &c, prio);
        if (rc == STARKHIP_OK) (i < n_big ? p->big_ctx : p->small_ctx).push_back(c);
    }
    if (rc != STARKHIP_OK) {
        for (Ctx* c : p->big_ctx) ctx_destroy(c);
        for (Ctx* c : p->small_ctx) ctx_destroy(c);
        return rc;
    }
    p->stream_priority = cfg.stream_priority;
    p->warm = cfg.warm_up != 0;
    p->warm_device_traces = cfg.warm_up == 2;
    HashService::Config hc;  // (row_leaves 64: a commitment this small is a handful of waves in either form: the shorter chain costs nothing -- FP12Mul: 32 leaves)
    {
        const char* n = getenv("STARKHIP_GEN_NICE");
        if (n && *n) p->gen_nice = atoi(n);
        const char* bl = getenv("STARKHIP_POOL_BIG_LANE");
        hc.big_lane = (bl && *bl) ? *bl == '1' : p->big_ctx.size() >= 5;  // with four or fewer in flight the quad form is faster (5.65 against 4.05 proofs/s)
        const char* rl = getenv("STARKHIP_POOL_ROW_LEAVES");
        if (rl && *rl) hc.row_leaves = (size_t)atol(rl);
        const char* lg = getenv("STARKHIP_POOL_LANE_GROUP");
        if (lg && *lg && atoi(lg) >= 2 && atoi(lg) <= 8) hc.lane_group = (unsigned)atoi(lg);
        const char* gr = getenv("STARKHIP_POOL_LANE_GROUPED");
        if (gr && *gr) hc.lane_grouped = *gr != '0';
        const char* bg = getenv("STARKHIP_POOL_BIG_GATHER_MS");
        if (bg && *bg && atof(bg) > 0) hc.big_gather_ms = atof(bg);
    }
    if (cfg.gather_ms > 0) hc.gather_ms = cfg.gather_ms;
    hc.policy = (int)cfg.commit_policy;
    hc.big_contexts = (int)p->big_ctx.size();
    p->hs.reset(new HashService(cfg.device, hc));
    if (cfg.commit_policy != 2) {  // 2: no commitment scheduling at all -- every context launches its own (A/B measurements)
        for (Ctx* c : p->big_ctx) ctx_attach_hash_service(c, p->hs.get());
        for (Ctx* c : p->small_ctx) ctx_attach_hash_service(c, p->hs.get());
    }
    Pool* raw = p.get();
    for (unsigned i = 0; i < p->gen_threads; i++) p->threads.emplace_back([raw] { raw->generator_loop(); });
    for (Ctx* c : p->big_ctx) p->threads.emplace_back([raw, c] { raw->prover_loop(c, true); });
    for (Ctx* c : p->small_ctx) p->threads.emplace_back([raw, c] { raw->prover_loop(c, false); });
    if (p->warm) {
        std::unique_lock<std::mutex> lk(p->mu);
        p->cv_done.wait(lk, [&] { return p->warmed == n_big + n_small; });
        const int wrc = p->warm_rc;
        lk.unlock();
        if (wrc != STARKHIP_OK) {
            pool_destroy(p.release());
            return wrc;
        }
    }
    *out = p.release();
    return STARKHIP_OK;
}

void pool_destroy(Pool* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(p->mu);
        p->stop = true;
    }
    p->cv_gen.notify_all();
    p->cv_big.notify_all();
    p->cv_small.notify_all();
    for (std::thread& t : p->threads) t.join();  // queued jobs are still run to completion: their callers may be waiting
    std::unique_ptr<VerifyService> vs;
    {   // ... and so is queued verify work (it may read the contexts' page-locked blobs: before the contexts go)
        std::lock_guard<std::mutex> g(p->vs_mu);
        p->vs_closed = true;
        vs = std::move(p->vs);
    }
    vs.reset();
    {   // every job is done now, so every caller blocked in pool_wait is on its way out: let them go before anything is freed
        std::unique_lock<std::mutex> lk(p->mu);
        p->cv_done.wait(lk, [&] { return p->waiters == 0; });
    }
    for (Ctx* c : p->big_ctx) ctx_destroy(c);
    for (Ctx* c : p->small_ctx) ctx_destroy(c);
    p->hs.reset();
    for (auto& kv : p->jobs) {
        blob_free(kv.second->proof);
        if (kv.second->own_log) starkhip_trace_log_free(kv.second->own_log);
        delete kv.second;
    }
    delete p;
}

static int pool_enqueue(Pool* p, Job* j, uint64_t* ticket) {
    const AirInfo* a = air_get(j->air);
    unsigned log_n = 0;
    const size_t rows = j->kind == JOB_RECORD ? a->default_rows : j->in.n_rows;
    while (((size_t)1 << log_n) < rows) log_n++;
    FriGeometry geo;  // a config prove() would refuse is refused here, before it takes a place in a queue
    if (!FriGeometry::make(j->cfg, log_n, &geo) || quotient_degree_bits(a->prog.degree) > j->cfg.rate_bits) {
        delete j;
        return STARKHIP_ERR_BAD_SHAPE;
    }
    j->big = HashService::is_big(log_n, j->cfg.rate_bits);
    std::lock_guard<std::mutex> g(p->mu);
    if (p->stop) {
        delete j;
        return STARKHIP_ERR_BAD_SHAPE;
    }
    j->id = p->next_id++;
    j->info.t_submit = p->now();
    j->verify = p->verify_proofs;
    j->check = p->check_traces;
    j->check_list = p->check_trace_list;
    j->fill = p->fill_lookups;
    j->fill_freq = p->fill_frequencies;
    j->hasher = p->hasher;
    j->cost = air_cost(j->air);
    p->load += j->cost;
    if (j->big) p->big_open++;
    p->jobs[j->id] = j;
    *ticket = j->id;
    if (j->kind == JOB_RECORD) {
        if (j->big) p->big_in_gen++;
        p->q_gen.push_back(j);
        p->cv_gen.notify_one();
    } else {
        (j->big ? p->q_big : p->q_small).push_back(j);
        (j->big ? p->cv_big : p->cv_small).notify_all();
    }
    if (j->big) p->tell_big_queued();
    return STARKHIP_OK;
}

// A trace the caller has: refused here as every entry refuses it (TraceInput::check), then queued for a context.  The caller keeps the
// trace's memory alive until the job is done; only a column table is copied, and the view re-pointed at the copy.
int pool_submit(Pool* p, int air, const starkhip_config_t* cfg, const TraceInput& in, const uint64_t* pis, size_t n_pis, uint64_t pow, uint64_t* ticket) {
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    if (in.check(*a) || !cfg || !ticket || (n_pis && !pis)) return STARKHIP_ERR_BAD_SHAPE;
    std::unique_ptr<Job> j(new (std::nothrow) Job());
    if (!j) return STARKHIP_ERR_OOM;
    j->air = air; j->cfg = *cfg; j->in = in; j->pis = pis; j->n_pis = n_pis; j->pow = pow;
    if (in.form == TraceForm::ColumnTable) {
        try {
            j->columns.assign(in.columns, in.columns + in.n_cols);
        } catch (const std::bad_alloc&) {
            return STARKHIP_ERR_OOM;
        }
        j->in.columns = j->columns.data();
    }
    return pool_enqueue(p, j.release(), ticket);
}

// A trace the pool records itself: its columns and public inputs come from the recording, its config may be the AIR's default
int pool_submit_witness(Pool* p, int air, const starkhip_config_t* cfg, const uint32_t* operands, size_t n_limbs, uint64_t pow, uint64_t* ticket) {
    if (!air_get(air) || witness_limbs(air) < 0) return STARKHIP_ERR_BAD_AIR;  // (a registered AIR: no generator to run)
    if (!operands || (size_t)witness_limbs(air) != n_limbs || !ticket) return STARKHIP_ERR_BAD_SHAPE;
    std::unique_ptr<Job> j(new (std::nothrow) Job());
    if (!j) return STARKHIP_ERR_OOM;
    j->air = air; j->kind = JOB_RECORD; j->pow = pow;
    if (cfg) j->cfg = *cfg;
    else if (int rc = starkhip_config_for_air((starkhip_air_t)air, &j->cfg)) return rc;
    j->operands.assign(operands, operands + n_limbs);
    return pool_enqueue(p, j.release(), ticket);
}

int pool_wait(Pool* p, uint64_t ticket, uint64_t** proof, size_t* words, starkhip_ticket_info_t* info) {
    Job* j;
    {
        std::unique_lock<std::mutex> lk(p->mu);
        auto it = p->jobs.find(ticket);
        if (it == p->jobs.end()) return STARKHIP_ERR_BAD_SHAPE;
        j = it->second;
        p->waiters++;
        p->cv_done.wait(lk, [&] { return j->state == JobState::Done; });
        p->jobs.erase(ticket);
        p->waiters--;
        if (p->stop) p->cv_done.notify_all();
    }
    const int rc = j->rc;
    if (info) *info = j->info;
    // (a verdict has no proof to hand over: j->proof is null; a refused trace hands over its check blob)
    if ((rc == STARKHIP_OK || (rc == STARKHIP_ERR_TRACE && j->proof)) && proof && words) {
        *proof = j->proof;
        *words = j->words;
    } else {
        blob_free(j->proof);
        if (proof) *proof = nullptr;
        if (words) *words = 0;
    }
    delete j;
    return rc;
}

// What the pool holds: device memory of all its contexts, their page-locked staging; per FinalExp-class context for sizing.
// Read between proofs (the contexts grow their buffers only inside prove()).
int pool_reservation(Pool* p, starkhip_pool_reservation_t* out) {
    memset(out, 0, sizeof *out);
    auto add = [&](const std::vector<Ctx*>& ctxs, uint64_t* largest) {
        for (Ctx* c : ctxs) {
            out->device_bytes += ctx_device_bytes(c);
            out->pinned_host_bytes += ctx_pinned_bytes(c);
            *largest = std::max<uint64_t>(*largest, ctx_device_bytes(c));
        }
    };
    add(p->big_ctx, &out->big_context_device_bytes);
    add(p->small_ctx, &out->small_context_device_bytes);
    out->big_contexts = (unsigned)p->big_ctx.size();
    out->small_contexts = (unsigned)p->small_ctx.size();
    return STARKHIP_OK;
}

int pool_host_info(Pool* p, starkhip_pool_host_info_t* out) {
    memset(out, 0, sizeof *out);
    out->cpu_budget = p->cpus;
    out->generator_threads = p->gen_threads;
    out->trace_threads_big = (unsigned)p->trace_threads_for_call(true);
    out->trace_threads_small = (unsigned)p->trace_threads_for_call(false);
    out->prover_threads = (unsigned)(p->big_ctx.size() + p->small_ctx.size());
    out->device = p->device;
    out->pools_on_device = p->pools_on_device;
    out->hw_queues = (unsigned)std::max(0, starkhip_hw_queues_in_effect());
    out->stream_budget = pool_stream_budget((unsigned)p->big_ctx.size(), (unsigned)p->small_ctx.size());
    return STARKHIP_OK;
}

PoolLoad pool_load(Pool* p) {
    std::lock_guard<std::mutex> g(p->mu);
    return PoolLoad{p->load, p->vload, p->big_open};
}

void pool_set_pools_on_device(Pool* p, unsigned n) { p->pools_on_device = n; }

int pool_stats(Pool* p, starkhip_pool_stats_t* out) {
    const HashService::Stats s = p->hs->stats();
    out->big_commit_launches = s.big_launches;
    out->small_commit_launches = s.small_launches;
    out->small_commit_requests = s.small_requests;
    out->max_merged_commitments = s.max_merged;
    out->big_commit_grids = s.big_grids;
    return STARKHIP_OK;
}
int pool_set_option(Pool* p, const char* name, long value) {
    if (!name) return STARKHIP_ERR_BAD_SHAPE;
    if (strcmp(name, "verify_proofs") == 0) {
        if (value != 0 && value != 1) return STARKHIP_ERR_BAD_SHAPE;
        std::lock_guard<std::mutex> g(p->vs_mu);
        {
            std::lock_guard<std::mutex> g2(p->mu);
            p->verify_proofs = value == 1;
        }
        if (value == 1 && p->warm && !p->vs && !p->vs_closed) return p->make_verifier();  // a warmed pool allocates now, not in its first proof
        return STARKHIP_OK;
    }
    if (strcmp(name, "check_traces") == 0 || strcmp(name, "check_trace_list") == 0) {  // read at submit, like "verify_proofs"
        const bool list = strcmp(name, "check_trace_list") == 0;
        if (value < 0 || value > (list ? (long)STARKHIP_CHECK_LIST_MAX : 1)) return STARKHIP_ERR_BAD_SHAPE;
        std::lock_guard<std::mutex> g(p->mu);
        if (list) p->check_trace_list = (size_t)value;
        else p->check_traces = value == 1;
        return STARKHIP_OK;
    }
    if (strcmp(name, "fill_lookups") == 0) {  // read at submit too
        if (value != 0 && value != 1) return STARKHIP_ERR_BAD_SHAPE;
        std::lock_guard<std::mutex> g(p->mu);
        p->fill_lookups = value == 1;
        return STARKHIP_OK;
    }
    if (strcmp(name, "fill_frequencies") == 0) {  // read at submit too
        if (value != 0 && value != 1) return STARKHIP_ERR_BAD_SHAPE;
        std::lock_guard<std::mutex> g(p->mu);
        p->fill_frequencies = value == 1;
        return STARKHIP_OK;
    }
    if (strcmp(name, "hasher") == 0) {  // read at submit too
        if (value < STARKHIP_HASHER_POSEIDON || value > STARKHIP_HASHER_KECCAK) return STARKHIP_ERR_BAD_SHAPE;
        std::lock_guard<std::mutex> g(p->mu);
        p->hasher = (int)value;
        return STARKHIP_OK;
    }
    if (strcmp(name, "verify_arena_mb") == 0) {
        if (value < 1 || value > (1l << 20)) return STARKHIP_ERR_BAD_SHAPE;
        std::lock_guard<std::mutex> g(p->vs_mu);
        if (p->vs) return STARKHIP_ERR_BAD_SHAPE;  // the arena exists already
        std::lock_guard<std::mutex> g2(p->mu);
        p->verify_arena_mb = (size_t)value;
        return STARKHIP_OK;
    }
    return STARKHIP_ERR_BAD_SHAPE;
}

int pool_submit_verify(Pool* p, int air, const starkhip_config_t* cfg, const uint64_t* proof, size_t words, uint64_t* ticket) {
    if (!ticket) return STARKHIP_ERR_BAD_SHAPE;
    Job* j = new (std::nothrow) Job();
    if (!j) return STARKHIP_ERR_OOM;
    j->kind = JOB_VERIFY;
    j->air = air;
    j->info.leaf_hash_group = 0;  // a verdict reports its three times and nothing else
    // an id without an AIR gets starkhip_verify's BAD_AIR without the verifier (and without a config to look up)
    int now_rc = STARKHIP_OK;
    if (!air_get(air)) now_rc = STARKHIP_ERR_BAD_AIR;
    else if (cfg) j->cfg = *cfg;
    else now_rc = starkhip_config_for_air((starkhip_air_t)air, &j->cfg);
    {
        std::lock_guard<std::mutex> g(p->mu);
        if (p->stop) {
            delete j;
            return STARKHIP_ERR_BAD_SHAPE;
        }
        j->id = p->next_id++;
        j->info.t_submit = p->now();
        j->cost = air_verify_cost(air);
        p->vload += j->cost;
        p->verify_jobs++;
        p->jobs[j->id] = j;
        *ticket = j->id;
    }
    if (now_rc == STARKHIP_OK && p->verify_submit(j, proof, words, &now_rc)) return STARKHIP_OK;
    p->finish(j, now_rc);
    return STARKHIP_OK;
}

int pool_verify_stats(Pool* p, starkhip_pool_verify_stats_t* out) {
    memset(out, 0, sizeof *out);
    {
        std::lock_guard<std::mutex> g(p->vs_mu);
        if (p->vs) {
            const VerifyService::Stats s = p->vs->stats();
            out->rejected = s.rejected;
            out->device_batches = s.batches;
            out->upload_ms = s.upload_ms;
            out->device_ms = s.device_ms;
            out->prelude_ms = s.prelude_ms;
            out->prelude_cpu_s = s.prelude_cpu_s;
            out->arena_bytes = s.arena_bytes;
        }
    }
    std::lock_guard<std::mutex> g(p->mu);
    out->proofs_checked = p->verified_proofs;
    out->verify_jobs = p->verify_jobs;
    return STARKHIP_OK;
}

int pool_check_stats(Pool* p, uint64_t out[2]) {
    out[0] = out[1] = 0;
    for (const std::vector<Ctx*>* ctxs : {&p->big_ctx, &p->small_ctx})
        for (Ctx* c : *ctxs) {
            uint64_t one[2];
            ctx_check_stats(c, one);
            out[0] += one[0];
            out[1] += one[1];
        }
    return STARKHIP_OK;
}

}  // namespace starkhip
