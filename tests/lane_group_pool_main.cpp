// Sanitizer harness for the grouped lane-form launch of the commitment scheduler (csrc/hash_service.cpp: launch_big_group): a pool of
// eight FinalExp-class contexts against the stand-in device of csrc/host_only_stubs.cc (STARKHIP_FAKE_DEVICE=1), under all three
// commit policies.  Groups of 2, 3 and 4 commitments must go out as ONE grid each, with every member's `done` event recorded on the
// launch stream; a member whose `ready` fails (pow_witness 0xBAD3) fails alone and its group goes out without it.  Built without a GPU
// (`make lane-group-test`: ThreadSanitizer, then AddressSanitizer + UndefinedBehaviorSanitizer); it checks scheduling, threading and
// memory, nothing about proofs.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "starkhip.h"

extern "C" void starkhip_stub_commit_counters(unsigned long out[4]);  // host_only_stubs.cc: launches, lane grids, their members, service-side event records

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "lane_group_pool: %s failed at line %d\n", #cond, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

struct Round {
    unsigned ok = 0, failed = 0, lane = 0, lone = 0;
    unsigned launches12 = 0;  // twelfths of a launch: a member of a group of g accounts for 1 / g of its grid
    unsigned largest_group = 0;
};

// `n` FinalExp-class jobs (job `bad`, if any, with a `ready` that fails), waited for; what their tickets say about the way they went out
static int run_round(void* pool, unsigned n, int bad, bool scheduled, Round* out) {
    const size_t fe_cols = (size_t)starkhip_air_columns(STARKHIP_AIR_FINAL_EXP), fe_pis = (size_t)starkhip_air_public_inputs(STARKHIP_AIR_FINAL_EXP);
    std::vector<uint64_t> pis(fe_pis, 7), fake_rows(16);
    starkhip_config_t fe_cfg;
    CHECK(starkhip_config_for_air(STARKHIP_AIR_FINAL_EXP, &fe_cfg) == STARKHIP_OK);
    std::vector<uint64_t> tickets(n);
    for (unsigned k = 0; k < n; k++)
        CHECK(starkhip_pool_submit(pool, STARKHIP_AIR_FINAL_EXP, &fe_cfg, fake_rows.data(), 8192, fe_cols, 1, 1, pis.data(), pis.size(),
                                   (int)k == bad ? 0xBAD3 : STARKHIP_POW_SEARCH, &tickets[k]) == STARKHIP_OK);
    *out = Round();
    for (unsigned k = 0; k < n; k++) {
        uint64_t* proof = nullptr;
        size_t words = 0;
        starkhip_ticket_info_t info;
        const int rc = starkhip_pool_wait(pool, tickets[k], &proof, &words, &info);
        if ((int)k == bad) {
            CHECK(rc == STARKHIP_ERR_HIP);  // that member, and only that one
            out->failed++;
            continue;
        }
        CHECK(rc == STARKHIP_OK && words == 4 + fe_pis);
        starkhip_free(proof);
        out->ok++;
        if (!scheduled) continue;  // commit policy 2: the context launched its own commitment
        CHECK(info.leaf_hash_group >= 1 && info.leaf_hash_group <= 4);
        if (info.leaf_hash_form == 3) {  // lane form: a member of a group
            out->lane++;
            out->launches12 += 12 / info.leaf_hash_group;
            if (info.leaf_hash_group > out->largest_group) out->largest_group = info.leaf_hash_group;
        } else {  // on its own: the pair form
            CHECK(info.leaf_hash_form == 5 && info.leaf_hash_group == 1);
            out->lone++;
            out->launches12 += 12;
        }
    }
    return 0;
}

int main() {
    setenv("STARKHIP_FAKE_DEVICE", "1", 1);
    setvbuf(stdout, nullptr, _IOLBF, 0);
    for (unsigned policy = 0; policy < 3; policy++) {
        starkhip_pool_config_t cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.big_contexts = 8;
        cfg.small_contexts = 1;
        cfg.generator_threads = 2;
        cfg.trace_threads = 1;
        cfg.commit_policy = policy;
        cfg.warm_up = 1;
        void* pool = nullptr;
        CHECK(starkhip_pool_create(&cfg, &pool) == STARKHIP_OK);
        starkhip_pool_host_info_t hi;
        CHECK(starkhip_pool_host_info(pool, &hi) == STARKHIP_OK && hi.stream_budget == 10 && hi.hw_queues == (unsigned)starkhip_hw_queues_in_effect());
        unsigned long total_grids = 0, total_commitments = 0;
        // groups of 2, 3 and 4; then a group of four with a member whose `ready` fails.  How the jobs fall into groups depends on when
        // their threads run, so every round is held to the invariants, and repeated (a few times at most) until the group meant was seen.
        for (unsigned want = 2; want <= 5; want++) {
            const bool with_bad = want == 5;
            const unsigned n = with_bad ? 4 : want, full = with_bad ? 3 : want;
            bool seen = false;
            for (int attempt = 0; attempt < 8 && !seen; attempt++) {
                unsigned long c0[4], c1[4];
                starkhip_stub_commit_counters(c0);
                Round r;
                if (int rc = run_round(pool, n, (with_bad && policy != 2) ? 1 : -1, policy != 2, &r)) return rc;
                starkhip_stub_commit_counters(c1);
                CHECK(r.ok == n - r.failed && r.failed == ((with_bad && policy != 2) ? 1u : 0u));
                if (policy == 2) {  // no commitment scheduling: every context launches its own, nothing goes through the service
                    CHECK(c1[0] == c0[0] && c1[1] == c0[1] && c1[3] == c0[3]);
                    seen = true;
                    continue;
                }
                CHECK(r.launches12 % 12 == 0);                               // whole groups: every member of a group of g says g
                CHECK(c1[0] - c0[0] == r.launches12 / 12);                  // ONE launch per group (and one per lone commitment)
                CHECK(c1[1] - c0[1] == r.launches12 / 12 - r.lone);         // ... the groups' as lane-form grids
                CHECK(c1[2] - c0[2] == r.lane);                             // ... which hold the members that were ready, and nobody else
                CHECK(c1[3] - c0[3] == r.ok);                               // every member's `done` recorded on its launch stream (once)
                total_grids += r.launches12 / 12;
                total_commitments += n;
                seen = r.largest_group == full;
            }
            CHECK(seen);
        }
        starkhip_pool_stats_t st;
        CHECK(starkhip_pool_stats(pool, &st) == STARKHIP_OK);
        if (policy != 2) CHECK(st.big_commit_grids == total_grids && st.big_commit_launches == total_commitments);
        starkhip_pool_destroy(pool);
        printf("policy %u: ok (%lu commitments in %lu launches)\n", policy, total_commitments, total_grids);
    }
    return 0;
}
