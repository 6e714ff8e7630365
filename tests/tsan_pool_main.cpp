// Sanitizer harness for the proof pool's host logic (csrc/pool.cpp, hash_service.cpp, multipool.cpp): generator threads, context workers, the commitment
// scheduler (gather window, merged launches, the two classes), job-to-context matching, failing jobs, shutdown with work queued.
// Built by `make tsan-test` / `make asan-test` WITHOUT a GPU against the stand-ins of csrc/host_only_stubs.cc
// (STARKHIP_FAKE_DEVICE=1: contexts exist, prove() sleeps and returns a blob that ends in the public inputs).  Test
// infrastructure only: it checks threading and memory, nothing about proofs.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <thread>
#include <vector>

#include "starkhip.h"

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "tsan_pool: %s failed at line %d\n", #cond, __LINE__); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static std::vector<uint32_t> limbs(size_t n, uint32_t seed) {
    std::vector<uint32_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (i % 12 == 11) ? 0x09000000u : seed * 0x9E3779B1u + 13u * (uint32_t)i;
    return v;
}

// A pool per device behind one handle (starkhip_multipool_*): three pretended devices, one of them twice; jobs placed by the library
// (longest first) and by the caller, from several threads; every proof must come from the device of the slot its ticket names.
static int multi_device_pass() {
    const int devices[4] = {0, 2, 5, 2};
    starkhip_pool_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.device = 7;  // ignored
    cfg.big_contexts = 2;
    cfg.small_contexts = 3;
    cfg.generator_threads = 2;
    cfg.trace_threads = 1;
    cfg.warm_up = 1;
    cfg.gather_ms = 3.0f;
    void* mp = nullptr;
    const int bad_dev[2] = {0, 9};
    CHECK(starkhip_multipool_create(bad_dev, 2, &cfg, &mp) == STARKHIP_ERR_NO_DEVICE && mp == nullptr);  // the good pool is taken down again
    CHECK(starkhip_multipool_create(devices, 4, &cfg, &mp) == STARKHIP_OK);
    CHECK(starkhip_multipool_size(mp) == 4 && starkhip_multipool_device(mp, 3) == 2 && starkhip_multipool_pool(mp, 4) == nullptr);
    // one signature's worth of jobs as ONE batch: the FinalExp-class job is placed first and alone, the rest fill the other pools
    std::vector<starkhip_air_t> airs = {STARKHIP_AIR_PAIRING_PRECOMP, STARKHIP_AIR_MILLER_LOOP, STARKHIP_AIR_PAIRING_PRECOMP,
                                        STARKHIP_AIR_MILLER_LOOP,     STARKHIP_AIR_FP12_MUL,    STARKHIP_AIR_FINAL_EXP};
    std::vector<std::vector<uint32_t>> ops = {limbs(72, 1), limbs(96, 2), limbs(72, 3), limbs(96, 4), limbs(288, 5), limbs(144, 6)};
    std::vector<int> plan(airs.size());
    CHECK(starkhip_plan_lpt(airs.size(), airs.data(), 4, plan.data()) == STARKHIP_OK);
    CHECK(plan[5] == 0 && plan[1] == 1 && plan[3] == 2 && plan[4] == 3 && plan[0] == 3 && plan[2] == 1);  // 128 | 24 + 10.8 | 24 | 15.4 + 10.8
    std::vector<const uint32_t*> op_ptr;
    std::vector<size_t> op_len;
    for (auto& o : ops) { op_ptr.push_back(o.data()); op_len.push_back(o.size()); }
    std::vector<uint64_t> tickets(airs.size());
    std::vector<int> rcs(airs.size());
    CHECK(starkhip_multipool_submit_witness_batch(mp, airs.size(), airs.data(), op_ptr.data(), op_len.data(), STARKHIP_POW_SEARCH, tickets.data(), rcs.data()) == STARKHIP_OK);
    for (size_t i = 0; i < airs.size(); i++) CHECK(rcs[i] == STARKHIP_OK && starkhip_multipool_ticket_slot(mp, tickets[i]) == plan[i]);
    // more jobs from four threads at once, some placed by the caller; a bad batch entry is reported per job
    struct Sub { starkhip_air_t air; std::vector<uint32_t> ops; int slot; uint64_t ticket; int rc; };
    std::vector<Sub> subs;
    for (int k = 0; k < 12; k++) subs.push_back({k % 3 == 0 ? STARKHIP_AIR_MILLER_LOOP : STARKHIP_AIR_FP12_MUL, limbs(k % 3 == 0 ? 96 : 288, 40 + k), k % 4 == 3 ? k % 4 : -1, 0, 0});
    std::vector<std::thread> th;
    for (int w = 0; w < 4; w++)
        th.emplace_back([&, w] {
            for (size_t i = w; i < subs.size(); i += 4)
                subs[i].rc = starkhip_multipool_submit_witness(mp, subs[i].slot, subs[i].air, nullptr, subs[i].ops.data(), subs[i].ops.size(), STARKHIP_POW_SEARCH, &subs[i].ticket);
        });
    for (auto& t : th) t.join();
    uint64_t t_bad = 0;
    CHECK(starkhip_multipool_submit_witness(mp, 4, STARKHIP_AIR_FP12_MUL, nullptr, ops[4].data(), 288, STARKHIP_POW_SEARCH, &t_bad) == STARKHIP_ERR_BAD_SHAPE);  // no such slot
    // rows in "device memory" need a slot
    const size_t fe_cols = (size_t)starkhip_air_columns(STARKHIP_AIR_FINAL_EXP), fe_pis = (size_t)starkhip_air_public_inputs(STARKHIP_AIR_FINAL_EXP);
    std::vector<uint64_t> pis(fe_pis, 7), fake_rows(16);
    starkhip_config_t fe_cfg;
    CHECK(starkhip_config_for_air(STARKHIP_AIR_FINAL_EXP, &fe_cfg) == STARKHIP_OK);
    CHECK(starkhip_multipool_submit(mp, -1, STARKHIP_AIR_FINAL_EXP, &fe_cfg, fake_rows.data(), 8192, fe_cols, 1, 1, pis.data(), pis.size(), STARKHIP_POW_SEARCH, &t_bad) == STARKHIP_ERR_BAD_SHAPE);
    uint64_t fe_t[5];
    for (int k = 0; k < 5; k++)  // host rows, placed by the library: FinalExp-class jobs spread over the pools before any pool gets a second
        CHECK(starkhip_multipool_submit(mp, -1, STARKHIP_AIR_FINAL_EXP, &fe_cfg, fake_rows.data(), 8192, fe_cols, 1, 0, pis.data(), pis.size(), STARKHIP_POW_SEARCH, &fe_t[k]) == STARKHIP_OK);
    int failures = 0;
    auto collect = [&](starkhip_air_t air, uint64_t ticket) {
        uint64_t* proof = nullptr;
        size_t words = 0;
        starkhip_ticket_info_t info;
        const int slot = starkhip_multipool_ticket_slot(mp, ticket);
        if (slot < 0 || starkhip_multipool_wait(mp, ticket, &proof, &words, &info) != STARKHIP_OK) { failures++; return; }
        if (words != 4 + (size_t)starkhip_air_public_inputs(air) || proof[1] != (uint64_t)air || (int)(proof[3] >> 8) != starkhip_multipool_device(mp, (size_t)slot)) failures++;
        starkhip_free(proof);
    };
    std::thread w1([&] { for (size_t i = 0; i < airs.size(); i++) collect(airs[i], tickets[i]); });
    std::thread w2([&] { for (auto& s : subs) { if (s.rc != STARKHIP_OK || (s.slot >= 0 && starkhip_multipool_ticket_slot(mp, s.ticket) != s.slot)) failures++; else collect(s.air, s.ticket); } });
    for (int k = 0; k < 5; k++) collect(STARKHIP_AIR_FINAL_EXP, fe_t[k]);
    w1.join();
    w2.join();
    CHECK(failures == 0);
    uint64_t* none = nullptr;
    size_t nw = 0;
    CHECK(starkhip_multipool_wait(mp, tickets[0], &none, &nw, nullptr) == STARKHIP_ERR_BAD_SHAPE);       // waited for once
    CHECK(starkhip_multipool_wait(mp, 12345, &none, &nw, nullptr) == STARKHIP_ERR_BAD_SHAPE);            // not a ticket of this handle
    // every pool proved something, and the FinalExp-class jobs went 2 + 2 + 1 + 1 (one from the batch, five placed one by one)
    unsigned long big[4], total_big = 0;
    for (size_t s = 0; s < 4; s++) {
        starkhip_pool_stats_t st;
        CHECK(starkhip_pool_stats(starkhip_multipool_pool(mp, s), &st) == STARKHIP_OK);
        big[s] = st.big_commit_launches;
        total_big += big[s];
        CHECK(st.small_commit_requests > 0 || big[s] > 0);
    }
    CHECK(total_big == 6);
    for (size_t s = 0; s < 4; s++) CHECK(big[s] >= 1 && big[s] <= 2);
    // shutdown with work queued on several pools
    for (int k = 0; k < 8; k++) {
        uint64_t t = 0;
        CHECK(starkhip_multipool_submit_witness(mp, -1, STARKHIP_AIR_MILLER_LOOP, nullptr, ops[1].data(), 96, STARKHIP_POW_SEARCH, &t) == STARKHIP_OK);
    }
    starkhip_multipool_destroy(mp);
    uint64_t bs[5];
    starkhip_proof_blob_stats(bs);
    CHECK(bs[0] == 0 && bs[2] == 0);
    printf("multi-device: ok (FinalExp-class proofs per pool %lu %lu %lu %lu)\n", big[0], big[1], big[2], big[3]);
    return 0;
}

// What every entry that takes a trace refuses, and with which code: starkhip_prove*, starkhip_pool_submit* and starkhip_multipool_submit*
// for a dense trace, a column table and a recording.  Every case starts from arguments that are accepted (asserted first) and has exactly
// one thing wrong; the doubly-wrong cases at the end pin the order of the checks.
enum Entry { E_PROVE, E_POOL, E_MULTI };
struct Handles { void *ctx, *pool, *mp; };
struct TraceArgs {
    starkhip_air_t air;
    const starkhip_config_t* cfg;
    const void* trace;  // dense words, a column table or a log, by the family of the entry
    size_t n_rows, n_cols;
    int layout, on_device;
    const uint64_t* pis;
    size_t n_pis;
    bool handle, out;  // false: a null context / pool / handle; a null ticket (proof pointer for starkhip_prove*)
    int slot;
};
enum Family { F_DENSE, F_COLUMNS, F_COMPACT };

// the status of the entry; of the wait, and of a look at the fake proof, where the submit was accepted
static int call_entry(const Handles& h, Entry e, Family f, const TraceArgs& a) {
    uint64_t* proof = nullptr;
    size_t words = 0;
    uint64_t ticket = 0;
    const uint64_t pow = 0;
    const uint64_t* dense = (const uint64_t*)a.trace;
    const uint64_t* const* table = (const uint64_t* const*)a.trace;
    int rc;
    if (e == E_PROVE) {
        void* ctx = a.handle ? h.ctx : nullptr;
        uint64_t** pp = a.out ? &proof : nullptr;
        rc = f == F_DENSE     ? starkhip_prove(ctx, a.air, a.cfg, dense, a.n_rows, a.n_cols, a.layout, a.on_device, a.pis, a.n_pis, pow, pp, &words)
             : f == F_COLUMNS ? starkhip_prove_columns(ctx, a.air, a.cfg, table, a.n_rows, a.n_cols, a.pis, a.n_pis, pow, pp, &words)
                              : starkhip_prove_compact(ctx, a.air, a.cfg, a.trace, a.pis, a.n_pis, pow, pp, &words);
    } else if (e == E_POOL) {
        void* pool = a.handle ? h.pool : nullptr;
        uint64_t* t = a.out ? &ticket : nullptr;
        rc = f == F_DENSE     ? starkhip_pool_submit(pool, a.air, a.cfg, dense, a.n_rows, a.n_cols, a.layout, a.on_device, a.pis, a.n_pis, pow, t)
             : f == F_COLUMNS ? starkhip_pool_submit_columns(pool, a.air, a.cfg, table, a.n_rows, a.n_cols, a.pis, a.n_pis, pow, t)
                              : starkhip_pool_submit_compact(pool, a.air, a.cfg, a.trace, a.pis, a.n_pis, pow, t);
        if (rc == STARKHIP_OK) rc = starkhip_pool_wait(pool, ticket, &proof, &words, nullptr);
    } else {
        void* mp = a.handle ? h.mp : nullptr;
        uint64_t* t = a.out ? &ticket : nullptr;
        rc = f == F_DENSE     ? starkhip_multipool_submit(mp, a.slot, a.air, a.cfg, dense, a.n_rows, a.n_cols, a.layout, a.on_device, a.pis, a.n_pis, pow, t)
             : f == F_COLUMNS ? starkhip_multipool_submit_columns(mp, a.slot, a.air, a.cfg, table, a.n_rows, a.n_cols, a.pis, a.n_pis, pow, t)
                              : starkhip_multipool_submit_compact(mp, a.slot, a.air, a.cfg, a.trace, a.pis, a.n_pis, pow, t);
        if (rc == STARKHIP_OK) rc = starkhip_multipool_wait(mp, ticket, &proof, &words, nullptr);
    }
    if (rc == STARKHIP_OK) {
        if (words != 4 + a.n_pis || proof[1] != (uint64_t)a.air || proof[2] != a.n_rows) rc = 1000;
        starkhip_free(proof);
    }
    return rc;
}

static int refusal_table() {
    const starkhip_air_t FIB = STARKHIP_AIR_TEST_FIBONACCI, MUL = STARKHIP_AIR_FP12_MUL, NO_AIR = (starkhip_air_t)999;
    const int SHAPE = STARKHIP_ERR_BAD_SHAPE;
    Handles h = {nullptr, nullptr, nullptr};
    starkhip_pool_config_t pc;
    memset(&pc, 0, sizeof pc);
    pc.big_contexts = 1;
    pc.small_contexts = 2;
    pc.generator_threads = 1;
    pc.trace_threads = 1;
    const int devices[2] = {0, 1};
    CHECK(starkhip_init(0, &h.ctx) == STARKHIP_OK);
    CHECK(starkhip_pool_create(&pc, &h.pool) == STARKHIP_OK);
    CHECK(starkhip_multipool_create(devices, 2, &pc, &h.mp) == STARKHIP_OK);

    // the toy AIR's rows, row-major, column-major and as a column table; an FP12Mul recording
    const size_t fib_rows = (size_t)starkhip_air_default_rows(FIB), fib_cols = (size_t)starkhip_air_columns(FIB), fib_pis = (size_t)starkhip_air_public_inputs(FIB);
    const size_t mul_rows = (size_t)starkhip_air_default_rows(MUL), mul_cols = (size_t)starkhip_air_columns(MUL), mul_pis = (size_t)starkhip_air_public_inputs(MUL);
    CHECK(fib_rows >= 2 && fib_cols >= 2 && fib_pis > 0 && mul_pis > 0 && mul_cols != fib_cols);
    std::vector<uint64_t> rows(fib_rows * fib_cols), colmajor(fib_rows * fib_cols), pis_fib(fib_pis), pis_mul(mul_pis);
    CHECK(starkhip_trace_fibonacci(3, 5, rows.data(), fib_rows, pis_fib.data()) == STARKHIP_OK);
    for (size_t r = 0; r < fib_rows; r++)
        for (size_t c = 0; c < fib_cols; c++) colmajor[c * fib_rows + r] = rows[r * fib_cols + c];
    std::vector<const uint64_t*> table(fib_cols), holed;
    for (size_t c = 0; c < fib_cols; c++) table[c] = &colmajor[c * fib_rows];
    holed = table;
    holed[fib_cols - 1] = nullptr;
    const std::vector<uint32_t> ops = limbs(288, 77);
    void *log = nullptr, *armed = nullptr;
    CHECK(starkhip_trace_log_begin(&log) == STARKHIP_OK);
    CHECK(starkhip_trace_fp12_mul(ops.data(), ops.data() + 144, nullptr, mul_rows, pis_mul.data()) == STARKHIP_OK);
    CHECK(starkhip_trace_log_end(log) == STARKHIP_OK);
    starkhip_config_t cfg_fib, cfg_mul;
    CHECK(starkhip_config_for_air(FIB, &cfg_fib) == STARKHIP_OK && starkhip_config_for_air(MUL, &cfg_mul) == STARKHIP_OK);

    const TraceArgs dense_ok = {FIB, &cfg_fib, rows.data(), fib_rows, fib_cols, 0, 0, pis_fib.data(), fib_pis, true, true, 0};
    const TraceArgs columns_ok = {FIB, &cfg_fib, table.data(), fib_rows, fib_cols, 0, 0, pis_fib.data(), fib_pis, true, true, 0};
    const TraceArgs compact_ok = {MUL, &cfg_mul, log, mul_rows, mul_cols, 0, 0, pis_mul.data(), mul_pis, true, true, 0};
    struct Case { const char* what; Family f; TraceArgs a; int want; };
    std::vector<Case> cases;
    auto add = [&](const char* what, Family f, int want, auto change) {
        TraceArgs a = f == F_DENSE ? dense_ok : f == F_COLUMNS ? columns_ok : compact_ok;
        change(a);
        cases.push_back({what, f, a, want});
    };
    for (Family f : {F_DENSE, F_COLUMNS, F_COMPACT}) {
        add("accepted", f, STARKHIP_OK, [](TraceArgs&) {});
        add("placed by the library", f, STARKHIP_OK, [](TraceArgs& a) { a.slot = -1; });
        add("null handle", f, STARKHIP_ERR_NO_DEVICE, [](TraceArgs& a) { a.handle = false; });
        add("unknown AIR", f, STARKHIP_ERR_BAD_AIR, [&](TraceArgs& a) { a.air = NO_AIR; });
        add("null trace", f, SHAPE, [](TraceArgs& a) { a.trace = nullptr; });
        add("null ticket", f, SHAPE, [](TraceArgs& a) { a.out = false; });
        add("public inputs missing", f, SHAPE, [](TraceArgs& a) { a.pis = nullptr; });
    }
    add("column-major", F_DENSE, STARKHIP_OK, [&](TraceArgs& a) { a.trace = colmajor.data(); a.layout = 1; });
    add("device memory, in a slot", F_DENSE, STARKHIP_OK, [](TraceArgs& a) { a.on_device = 1; });
    add("layout 2", F_DENSE, SHAPE, [](TraceArgs& a) { a.layout = 2; });
    add("layout -1", F_DENSE, SHAPE, [](TraceArgs& a) { a.layout = -1; });
    for (Family f : {F_DENSE, F_COLUMNS}) {
        add("a column too many", f, SHAPE, [](TraceArgs& a) { a.n_cols++; });
        add("a column too few", f, SHAPE, [](TraceArgs& a) { a.n_cols--; });
    }
    add("null column", F_COLUMNS, SHAPE, [&](TraceArgs& a) { a.trace = holed.data(); });
    add("another AIR's recording", F_COMPACT, SHAPE, [&](TraceArgs& a) { a.air = FIB; a.cfg = &cfg_fib; a.pis = pis_fib.data(); a.n_pis = fib_pis; });
    for (const Case& c : cases)
        for (Entry e : {E_PROVE, E_POOL, E_MULTI}) {
            const int got = call_entry(h, e, c.f, c.a);
            if (got != c.want) {
                fprintf(stderr, "tsan_pool: refusal table: %s, family %d, entry %d: %d, want %d\n", c.what, (int)c.f, (int)e, got, c.want);
                return 1;
            }
        }
    // device memory belongs to one device: a multi-device handle wants the slot
    TraceArgs no_slot = dense_ok;
    no_slot.on_device = 1;
    no_slot.slot = -1;
    CHECK(call_entry(h, E_MULTI, F_DENSE, no_slot) == SHAPE);
    // a recording that is still armed on this thread
    std::vector<uint64_t> pis_armed(mul_pis);
    CHECK(starkhip_trace_log_begin(&armed) == STARKHIP_OK);
    CHECK(starkhip_trace_fp12_mul(ops.data(), ops.data() + 144, nullptr, mul_rows, pis_armed.data()) == STARKHIP_OK);
    TraceArgs still_armed = compact_ok;
    still_armed.trace = armed;
    for (Entry e : {E_PROVE, E_POOL, E_MULTI}) CHECK(call_entry(h, e, F_COMPACT, still_armed) == SHAPE);
    // wrong in two ways: no handle before the AIR, the AIR before the trace -- but for an armed recording in the submits and device
    // memory without a slot, which are refused before the AIR is looked at
    for (Family f : {F_DENSE, F_COLUMNS, F_COMPACT})
        for (Entry e : {E_PROVE, E_POOL, E_MULTI}) {
            TraceArgs a = f == F_DENSE ? dense_ok : f == F_COLUMNS ? columns_ok : compact_ok;
            a.air = NO_AIR;
            a.trace = nullptr;
            CHECK(call_entry(h, e, f, a) == STARKHIP_ERR_BAD_AIR);
            a.handle = false;
            CHECK(call_entry(h, e, f, a) == STARKHIP_ERR_NO_DEVICE);
        }
    still_armed.air = NO_AIR;
    CHECK(call_entry(h, E_PROVE, F_COMPACT, still_armed) == STARKHIP_ERR_BAD_AIR);
    CHECK(call_entry(h, E_POOL, F_COMPACT, still_armed) == SHAPE);
    CHECK(call_entry(h, E_MULTI, F_COMPACT, still_armed) == SHAPE);
    no_slot.air = NO_AIR;
    CHECK(call_entry(h, E_MULTI, F_DENSE, no_slot) == SHAPE);
    CHECK(starkhip_trace_log_end(armed) == STARKHIP_OK);
    CHECK(call_entry(h, E_POOL, F_COMPACT, [&] { TraceArgs a = compact_ok; a.trace = armed; return a; }()) == STARKHIP_OK);  // finished: accepted

    starkhip_trace_log_free(armed);
    starkhip_trace_log_free(log);
    starkhip_multipool_destroy(h.mp);
    starkhip_pool_destroy(h.pool);
    starkhip_shutdown(h.ctx);
    printf("refusal table: ok (%zu cases on three entries each)\n", cases.size());
    return 0;
}

// The leaf-hash forms' host-built tables (csrc/poseidon_tables.cpp): the replays of the merged rounds agree with the plain permutation and
// every image has the size tests/golden/hash_table_images.json records -- under the sanitizers, the builders' every index and shift.
static int hash_tables_pass() {
    CHECK(starkhip_selfcheck_hash_tables(50) == 0);
    const size_t golden_bytes[5] = {0, 2592, 2848, 26608, 12736};
    for (int form = 1; form <= 4; form++) {
        std::vector<unsigned char> image(golden_bytes[form]);
        CHECK(starkhip_hash_table_image(form, image.data(), image.size()) == golden_bytes[form]);
    }
    CHECK(starkhip_hash_table_image(0, nullptr, 0) == 0);
    printf("hash tables: ok\n");
    return 0;
}

int main() {
    setenv("STARKHIP_FAKE_DEVICE", "1", 1);
    if (int rc = hash_tables_pass()) return rc;
    if (int rc = refusal_table()) return rc;
    if (int rc = multi_device_pass()) return rc;
    for (unsigned pass = 0; pass < 4; pass++) {
        const unsigned policy = pass < 3 ? pass : 0;
        // the fourth pass: big commitments gathered into lane-form groups (what pools with five or more big contexts do)
        if (pass == 3) setenv("STARKHIP_POOL_BIG_LANE", "1", 1);
        starkhip_pool_config_t cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.big_contexts = 2;
        cfg.small_contexts = 5;
        cfg.generator_threads = 3;
        cfg.trace_threads = 2;
        cfg.commit_policy = policy;
        cfg.stream_priority = 1;
        cfg.warm_up = 1;
        cfg.gather_ms = 5.0f;
        void* pool = nullptr;
        CHECK(starkhip_pool_create(&cfg, &pool) == STARKHIP_OK);
        // witness jobs of three small AIRs and the toy one, submitted from several threads at once
        struct Sub { starkhip_air_t air; std::vector<uint32_t> ops; uint64_t pow; uint64_t ticket; int rc_submit; };
        std::vector<Sub> subs;
        for (int k = 0; k < 4; k++) subs.push_back({STARKHIP_AIR_FP12_MUL, limbs(288, 1 + k), STARKHIP_POW_SEARCH, 0, 0});
        for (int k = 0; k < 3; k++) subs.push_back({STARKHIP_AIR_PAIRING_PRECOMP, limbs(72, 11 + k), STARKHIP_POW_SEARCH, 0, 0});
        for (int k = 0; k < 2; k++) subs.push_back({STARKHIP_AIR_MILLER_LOOP, limbs(96, 21 + k), STARKHIP_POW_SEARCH, 0, 0});
        subs.push_back({STARKHIP_AIR_TEST_FIBONACCI, {3, 0, 5, 0}, STARKHIP_POW_SEARCH, 0, 0});
        subs.push_back({STARKHIP_AIR_FP12_MUL, limbs(288, 31), 0xBAD, 0, 0});    // fails before its commitment
        subs.push_back({STARKHIP_AIR_FP12_MUL, limbs(288, 32), 0xBAD2, 0, 0});   // fails after it
        std::vector<std::thread> th;
        for (size_t i = 0; i < subs.size(); i++)
            th.emplace_back([&, i] {
                subs[i].rc_submit = starkhip_pool_submit_witness(pool, subs[i].air, nullptr, subs[i].ops.data(), subs[i].ops.size(), subs[i].pow, &subs[i].ticket);
            });
        for (auto& t : th) t.join();
        // a FinalExp-class job from rows the caller owns (fake: only the shape is looked at) -- two of them: the second is the "last wave"
        const size_t fe_cols = (size_t)starkhip_air_columns(STARKHIP_AIR_FINAL_EXP), fe_pis = (size_t)starkhip_air_public_inputs(STARKHIP_AIR_FINAL_EXP);
        std::vector<uint64_t> pis(fe_pis, 7), fake_rows(16);
        starkhip_config_t fe_cfg;
        CHECK(starkhip_config_for_air(STARKHIP_AIR_FINAL_EXP, &fe_cfg) == STARKHIP_OK);
        uint64_t fe_t[3];
        for (int k = 0; k < 3; k++)
            CHECK(starkhip_pool_submit(pool, STARKHIP_AIR_FINAL_EXP, &fe_cfg, fake_rows.data(), 8192, fe_cols, 1, 1, pis.data(), pis.size(), STARKHIP_POW_SEARCH, &fe_t[k]) == STARKHIP_OK);
        // wrong shapes are refused at submit
        uint64_t t_bad = 0;
        CHECK(starkhip_pool_submit(pool, STARKHIP_AIR_FINAL_EXP, &fe_cfg, fake_rows.data(), 8192, fe_cols - 1, 1, 1, pis.data(), pis.size(), STARKHIP_POW_SEARCH, &t_bad) == STARKHIP_ERR_BAD_SHAPE);
        CHECK(starkhip_pool_submit_witness(pool, STARKHIP_AIR_FP12_MUL, nullptr, subs[0].ops.data(), 17, STARKHIP_POW_SEARCH, &t_bad) == STARKHIP_ERR_BAD_SHAPE);
        // waits, from two threads
        int failures = 0;
        auto wait_range = [&](size_t a, size_t b) {
            for (size_t i = a; i < b; i++) {
                uint64_t* proof = nullptr;
                size_t words = 0;
                starkhip_ticket_info_t info;
                const int rc = subs[i].rc_submit == STARKHIP_OK ? starkhip_pool_wait(pool, subs[i].ticket, &proof, &words, &info) : subs[i].rc_submit;
                const int want = subs[i].pow == 0xBAD ? STARKHIP_ERR_BAD_SHAPE : subs[i].pow == 0xBAD2 ? STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE : STARKHIP_OK;
                if (rc != want) failures++;
                if (rc == STARKHIP_OK) {
                    const size_t n_pis = (size_t)starkhip_air_public_inputs(subs[i].air);
                    if (words != 4 + n_pis || proof[1] != (uint64_t)subs[i].air || info.t_done < info.t_prove_start) failures++;
                    starkhip_free(proof);
                }
            }
        };
        std::thread w1([&] { wait_range(0, subs.size() / 2); }), w2([&] { wait_range(subs.size() / 2, subs.size()); });
        w1.join();
        w2.join();
        CHECK(failures == 0);
        uint64_t* kept = nullptr;  // one proof stays with the caller beyond the pool's life
        for (int k = 0; k < 3; k++) {
            uint64_t* proof = nullptr;
            size_t words = 0;
            CHECK(starkhip_pool_wait(pool, fe_t[k], &proof, &words, nullptr) == STARKHIP_OK && words == 4 + fe_pis);
            if (k == 0) kept = proof;
            else starkhip_free(proof);
        }
        uint64_t* none = nullptr;
        size_t nw = 0;
        CHECK(starkhip_pool_wait(pool, fe_t[0], &none, &nw, nullptr) == STARKHIP_ERR_BAD_SHAPE);  // a ticket is waited for once
        starkhip_pool_stats_t st;
        CHECK(starkhip_pool_stats(pool, &st) == STARKHIP_OK);
        if (policy != 2) CHECK(st.big_commit_launches == 3 && st.small_commit_requests == 11);  // 10 good small jobs + the one that fails after its commitment
        // shutdown with work still queued: never waited for, still run to the end and freed
        for (int k = 0; k < 6; k++) {
            uint64_t t = 0;
            CHECK(starkhip_pool_submit_witness(pool, STARKHIP_AIR_FP12_MUL, nullptr, subs[0].ops.data(), 288, STARKHIP_POW_SEARCH, &t) == STARKHIP_OK);
        }
        // ... and witness jobs that are still queued for (or in) their RECORDING when the pool is destroyed: the contexts must not
        // leave before the generators have handed them over, and a caller blocked in wait on one of them must get its proof
        uint64_t t_late[3];
        for (int k = 0; k < 3; k++)
            CHECK(starkhip_pool_submit_witness(pool, k == 1 ? STARKHIP_AIR_PAIRING_PRECOMP : STARKHIP_AIR_MILLER_LOOP, nullptr,
                                               subs[k == 1 ? 4 : 7].ops.data(), k == 1 ? 72 : 96, STARKHIP_POW_SEARCH, &t_late[k]) == STARKHIP_OK);
        int late_rc = -100;
        size_t late_words = 0;
        std::thread late([&] {
            uint64_t* proof = nullptr;
            late_rc = starkhip_pool_wait(pool, t_late[2], &proof, &late_words, nullptr);
            if (late_rc == STARKHIP_OK) starkhip_free(proof);
        });
        std::this_thread::sleep_for(std::chrono::milliseconds(20));  // the waiter is inside pool_wait (its job's recording takes longer)
        starkhip_pool_destroy(pool);
        late.join();
        CHECK(late_rc == STARKHIP_OK && late_words == 4 + (size_t)starkhip_air_public_inputs(STARKHIP_AIR_MILLER_LOOP));
        uint64_t bs[5];
        starkhip_proof_blob_stats(bs);
        CHECK(bs[3] > 0);                    // warmed contexts served proofs from the arena
        CHECK(bs[0] == bs[1] && bs[0] <= 1);  // every idle blob went with its context; at most the kept proof's remains
        CHECK(kept[0] == 0xFA4EULL);          // and is still readable
        starkhip_free(kept);
        starkhip_proof_blob_stats(bs);
        CHECK(bs[0] == 0 && bs[2] == 0);
        printf("policy %u: ok (%lu small requests in %lu launches, up to %lu merged)\n", policy, st.small_commit_requests, st.small_commit_launches,
               st.max_merged_commitments);
    }
    return 0;
}
