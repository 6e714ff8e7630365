// Sanitizer harness for a proof pool's verifier (csrc/verify_service.cpp) on the stand-in device of csrc/host_only_stubs.cc
// (STARKHIP_FAKE_DEVICE=1): its four verify launches run their routine on the host, so verdicts are real.  Given a file of proofs
// (tests/test_verify_pool_cpu.py writes oracle proofs of the toy AIR, tampered and malformed ones), it checks:
//   * the pool options ("verify_proofs", "verify_arena_mb") and their errors;
//   * verify jobs submitted and waited for from four threads at once: every verdict equals starkhip_verify's code, and the stand-in's
//     allocation counter does not move once the verifier's arena exists;
//   * "verify_proofs" on the stand-in's proving jobs (their blobs are no proofs: wait must return the verifier's BAD_SHAPE);
//   * a two-device handle's verify batch, both pools receiving work;
//   * destroy with verify work queued.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#include "starkhip.h"

extern "C" unsigned long starkhip_stub_allocations(void);  // host_only_stubs.cc

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "tsan_verify_pool: %s failed at line %d\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

struct Case {
    starkhip_air_t air;
    starkhip_config_t cfg;
    std::vector<uint64_t> proof;
    int want;
};

// per case: int32 air, uint32 config bytes, the config, uint64 words, the words
static bool load(const char* path, std::vector<Case>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    while (true) {
        int32_t air;
        uint32_t cfg_bytes;
        uint64_t words;
        if (fread(&air, 4, 1, f) != 1) break;
        Case c;
        memset(&c.cfg, 0, sizeof c.cfg);
        if (fread(&cfg_bytes, 4, 1, f) != 1 || cfg_bytes != sizeof c.cfg || fread(&c.cfg, cfg_bytes, 1, f) != 1 || fread(&words, 8, 1, f) != 1) {
            fclose(f);
            return false;
        }
        c.proof.resize(words);
        if (words && fread(c.proof.data(), 8, words, f) != words) {
            fclose(f);
            return false;
        }
        memcpy(&c.air, &air, sizeof air);
        c.want = starkhip_verify(c.air, &c.cfg, c.proof.data(), c.proof.size());
        out.push_back(std::move(c));
    }
    fclose(f);
    return !out.empty();
}

static starkhip_pool_config_t pool_config() {
    starkhip_pool_config_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.big_contexts = 1;
    cfg.small_contexts = 2;
    cfg.generator_threads = 2;
    cfg.trace_threads = 1;
    cfg.warm_up = 1;
    cfg.gather_ms = 2.0f;
    return cfg;
}

int main(int argc, char** argv) {
    std::vector<Case> cases;
    CHECK(argc == 2 && load(argv[1], cases));
    int n_ok = 0, n_bad = 0;
    for (const Case& c : cases) (c.want == STARKHIP_OK ? n_ok : n_bad)++;
    CHECK(n_ok > 0 && n_bad > 0);

    // ---- options
    starkhip_pool_config_t pc = pool_config();
    void* pool = nullptr;
    CHECK(starkhip_pool_create(&pc, &pool) == STARKHIP_OK);
    CHECK(starkhip_pool_set_option(pool, "no_such_option", 1) == STARKHIP_ERR_BAD_SHAPE);
    CHECK(starkhip_pool_set_option(pool, "verify_proofs", 2) == STARKHIP_ERR_BAD_SHAPE);
    CHECK(starkhip_pool_set_option(pool, "verify_arena_mb", 0) == STARKHIP_ERR_BAD_SHAPE);
    CHECK(starkhip_pool_set_option(pool, "verify_arena_mb", 8) == STARKHIP_OK);
    starkhip_pool_verify_stats_t vs;
    CHECK(starkhip_pool_verify_stats(pool, &vs) == STARKHIP_OK && vs.arena_bytes == 0);
    CHECK(starkhip_pool_set_option(pool, "verify_proofs", 1) == STARKHIP_OK);  // a warmed pool: the arena now
    CHECK(starkhip_pool_verify_stats(pool, &vs) == STARKHIP_OK && vs.arena_bytes == ((uint64_t)8 << 20));
    CHECK(starkhip_pool_set_option(pool, "verify_arena_mb", 16) == STARKHIP_ERR_BAD_SHAPE);
    CHECK(starkhip_pool_set_option(pool, "verify_proofs", 0) == STARKHIP_OK);
    const unsigned long allocs0 = starkhip_stub_allocations();

    // ---- verify jobs from four threads, each submitting and waiting; twice over, so that batches form while others are waited for
    const size_t n_jobs = 2 * cases.size();
    std::vector<int> got(n_jobs, -1000), sub_rc(n_jobs, -1000);
    std::vector<std::thread> th;
    for (int w = 0; w < 4; w++)
        th.emplace_back([&, w] {
            std::vector<std::pair<size_t, uint64_t>> mine;
            for (size_t i = w; i < n_jobs; i += 4) {
                const Case& c = cases[i % cases.size()];
                uint64_t t = 0;
                sub_rc[i] = starkhip_pool_submit_verify(pool, c.air, &c.cfg, c.proof.data(), c.proof.size(), &t);
                mine.emplace_back(i, t);
                if (mine.size() == 3) {  // wait for the oldest while later ones are queued
                    uint64_t* p = (uint64_t*)1;
                    size_t words = 7;
                    starkhip_ticket_info_t info;
                    got[mine.front().first] = starkhip_pool_wait(pool, mine.front().second, &p, &words, &info);
                    if (p != nullptr || words != 0 || info.phase_ms[0] != 0 || info.t_generate_start != 0 || info.t_done < info.t_submit) got[mine.front().first] = -999;
                    mine.erase(mine.begin());
                }
            }
            for (auto& m : mine) got[m.first] = starkhip_pool_wait(pool, m.second, nullptr, nullptr, nullptr);
        });
    for (auto& t : th) t.join();
    for (size_t i = 0; i < n_jobs; i++) {
        CHECK(sub_rc[i] == STARKHIP_OK);
        if (got[i] != cases[i % cases.size()].want) {
            fprintf(stderr, "tsan_verify_pool: job %zu: %d, starkhip_verify %d\n", i, got[i], cases[i % cases.size()].want);
            return 1;
        }
    }
    CHECK(starkhip_stub_allocations() == allocs0);  // nothing allocated per batch
    // an unknown AIR, a NULL config (starkhip_config_for_air), a NULL proof
    uint64_t t1 = 0, t2 = 0, t3 = 0;
    CHECK(starkhip_pool_submit_verify(pool, (starkhip_air_t)9999, nullptr, cases[0].proof.data(), cases[0].proof.size(), &t1) == STARKHIP_OK);
    CHECK(starkhip_pool_submit_verify(pool, cases[0].air, nullptr, cases[0].proof.data(), cases[0].proof.size(), &t2) == STARKHIP_OK);
    CHECK(starkhip_pool_submit_verify(pool, cases[0].air, &cases[0].cfg, nullptr, 0, &t3) == STARKHIP_OK);
    CHECK(starkhip_pool_submit_verify(pool, cases[0].air, &cases[0].cfg, cases[0].proof.data(), cases[0].proof.size(), nullptr) == STARKHIP_ERR_BAD_SHAPE);
    CHECK(starkhip_pool_wait(pool, t1, nullptr, nullptr, nullptr) == STARKHIP_ERR_BAD_AIR);
    starkhip_config_t dflt;
    CHECK(starkhip_config_for_air(cases[0].air, &dflt) == STARKHIP_OK);
    CHECK(starkhip_pool_wait(pool, t2, nullptr, nullptr, nullptr) == starkhip_verify(cases[0].air, &dflt, cases[0].proof.data(), cases[0].proof.size()));
    CHECK(starkhip_pool_wait(pool, t3, nullptr, nullptr, nullptr) == STARKHIP_ERR_BAD_SHAPE);
    CHECK(starkhip_pool_verify_stats(pool, &vs) == STARKHIP_OK);
    CHECK(vs.verify_jobs == n_jobs + 3 && vs.proofs_checked == 0 && vs.device_batches > 0);
    CHECK(vs.rejected >= 2 * (unsigned long)n_bad + 1);  // the NULL proof too (the unknown AIR never reaches the verifier)

    // ---- "verify_proofs" on proving jobs: the stand-in's blobs are no proofs
    CHECK(starkhip_pool_set_option(pool, "verify_proofs", 1) == STARKHIP_OK);
    const uint32_t fib[4] = {3, 0, 5, 0};
    std::vector<uint64_t> tickets;
    for (int k = 0; k < 6; k++) {
        uint64_t t = 0;
        CHECK(starkhip_pool_submit_witness(pool, STARKHIP_AIR_TEST_FIBONACCI, nullptr, fib, 4, STARKHIP_POW_SEARCH, &t) == STARKHIP_OK);
        tickets.push_back(t);
    }
    for (uint64_t t : tickets) {
        uint64_t* p = (uint64_t*)1;
        size_t words = 7;
        CHECK(starkhip_pool_wait(pool, t, &p, &words, nullptr) == STARKHIP_ERR_BAD_SHAPE && p == nullptr && words == 0);
    }
    CHECK(starkhip_pool_set_option(pool, "verify_proofs", 0) == STARKHIP_OK);
    {  // submitted with the option off: as before
        uint64_t t = 0, *p = nullptr;
        size_t words = 0;
        CHECK(starkhip_pool_submit_witness(pool, STARKHIP_AIR_TEST_FIBONACCI, nullptr, fib, 4, STARKHIP_POW_SEARCH, &t) == STARKHIP_OK);
        CHECK(starkhip_pool_wait(pool, t, &p, &words, nullptr) == STARKHIP_OK && p && words > 0);
        starkhip_free(p);
    }
    CHECK(starkhip_pool_verify_stats(pool, &vs) == STARKHIP_OK && vs.proofs_checked == 6);

    // ---- destroy with verify work queued (never waited for)
    for (size_t i = 0; i < cases.size(); i++) {
        uint64_t t = 0;
        CHECK(starkhip_pool_submit_verify(pool, cases[i].air, &cases[i].cfg, cases[i].proof.data(), cases[i].proof.size(), &t) == STARKHIP_OK);
    }
    starkhip_pool_destroy(pool);
    printf("pool: ok\n");

    // ---- two pretended devices: a verify batch spread over both
    const int devices[2] = {0, 1};
    void* mp = nullptr;
    CHECK(starkhip_multipool_create(devices, 2, &pc, &mp) == STARKHIP_OK);
    CHECK(starkhip_multipool_set_option(mp, "verify_arena_mb", 4) == STARKHIP_OK);
    CHECK(starkhip_multipool_set_option(mp, "bogus", 1) == STARKHIP_ERR_BAD_SHAPE);
    const size_t n = cases.size();
    std::vector<starkhip_air_t> airs(n);
    std::vector<starkhip_config_t> cfgs(n);
    std::vector<const uint64_t*> ptrs(n);
    std::vector<size_t> words(n);
    std::vector<int> res(n, -1000);
    for (size_t i = 0; i < n; i++) {
        airs[i] = cases[i].air;
        cfgs[i] = cases[i].cfg;
        ptrs[i] = cases[i].proof.data();
        words[i] = cases[i].proof.size();
    }
    CHECK(starkhip_multipool_verify_batch(mp, n, airs.data(), cfgs.data(), ptrs.data(), words.data(), res.data()) == STARKHIP_OK);
    for (size_t i = 0; i < n; i++) CHECK(res[i] == cases[i].want);
    for (size_t s = 0; s < 2; s++) {
        CHECK(starkhip_pool_verify_stats(starkhip_multipool_pool(mp, s), &vs) == STARKHIP_OK);
        CHECK(vs.verify_jobs > 0);
    }
    uint64_t t = 0;
    CHECK(starkhip_multipool_submit_verify(mp, 1, cases[0].air, &cases[0].cfg, cases[0].proof.data(), cases[0].proof.size(), &t) == STARKHIP_OK);
    CHECK(starkhip_multipool_ticket_slot(mp, t) == 1);
    CHECK(starkhip_multipool_wait(mp, t, nullptr, nullptr, nullptr) == cases[0].want);
    CHECK(starkhip_multipool_submit_verify(mp, 2, cases[0].air, &cases[0].cfg, cases[0].proof.data(), cases[0].proof.size(), &t) == STARKHIP_ERR_BAD_SHAPE);
    starkhip_multipool_destroy(mp);
    printf("multipool: ok\n");
    return 0;
}
