// The proof pool's two picking rules (csrc/pool.h: pick_recording, pick_job) on hand-made queues: what their comments promise, with no
// thread and no device.  Built and run by tests/test_pool_pickers_cpu.py against the library.
#include <stdio.h>

#include <deque>
#include <map>
#include <memory>
#include <vector>

#include "../starky_bls12_381_amd/csrc/pool.h"

using namespace starkhip;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            fprintf(stderr, "pool_pickers: %s failed at line %d\n", #cond, __LINE__); \
            return 1;                                                               \
        }                                                                           \
    } while (0)

static const int FE = STARKHIP_AIR_FINAL_EXP, ML = STARKHIP_AIR_MILLER_LOOP, PP = STARKHIP_AIR_PAIRING_PRECOMP, F12 = STARKHIP_AIR_FP12_MUL;

struct Queue {
    std::vector<std::unique_ptr<Job>> own;
    std::deque<Job*> q;
    Job* add(int air) {
        own.emplace_back(new Job());
        own.back()->air = air;
        own.back()->big = air == FE;
        q.push_back(own.back().get());
        return own.back().get();
    }
    void take(std::deque<Job*>::iterator it) { q.erase(it); }
};

static int recordings() {
    // the ranks the order rests on: recordings that cost nothing (FP12Mul: 16 rows) ahead of all, then by columns
    Job f12, ml, pp;
    f12.air = F12; ml.air = ML; pp.air = PP;
    CHECK(small_rank(&f12) > small_rank(&ml) && small_rank(&ml) > small_rank(&pp) && small_rank(&pp) > 0);

    Queue g;
    Job* p1 = g.add(PP);
    Job* m1 = g.add(ML);
    Job* fe1 = g.add(FE);
    Job* f1 = g.add(F12);
    Job* fe2 = g.add(FE);
    Job* m2 = g.add(ML);
    Job* fe3 = g.add(FE);
    Job* fe4 = g.add(FE);
    // two big contexts and one recording ahead: the first THREE FinalExp-class recordings go first, in arrival order
    const size_t wanted = 2 + 1;
    size_t started = 0;
    for (Job* want : {fe1, fe2, fe3}) {
        auto it = pick_recording(g.q, started, wanted);
        CHECK(it != g.q.end() && *it == want);
        g.take(it);
        started++;
    }
    // then the small AIRs': the 16-row one ahead of all, the others longest first, equal ones in arrival order -- not the fourth big one
    for (Job* want : {f1, m1, m2, p1}) {
        auto it = pick_recording(g.q, started, wanted);
        CHECK(it != g.q.end() && *it == want);
        g.take(it);
    }
    // nothing of the wanted class left: the other one's
    auto it = pick_recording(g.q, started, wanted);
    CHECK(it != g.q.end() && *it == fe4 && g.q.size() == 1);
    // a context has become free (one recording fewer counts as started): big ones are wanted again, before a small one that came earlier
    Queue h;
    Job* hp = h.add(PP);
    Job* hm = h.add(ML);
    Job* hfe = h.add(FE);
    CHECK(*pick_recording(h.q, 2, wanted) == hfe);
    CHECK(*pick_recording(h.q, 3, wanted) == hm);
    h.take(pick_recording(h.q, 2, wanted));
    CHECK(*pick_recording(h.q, 0, wanted) == hm);  // big ones wanted, none queued: the longest small one
    h.take(pick_recording(h.q, 0, wanted));
    CHECK(*pick_recording(h.q, 0, wanted) == hp);
    Queue none;
    CHECK(pick_recording(none.q, 0, wanted) == none.q.end());
    return 0;
}

static int contexts() {
    Queue s;
    Job* p1 = s.add(PP);
    Job* f1 = s.add(F12);
    Job* m1 = s.add(ML);
    Job* p2 = s.add(PP);
    std::map<int, int> idle;
    // a context prefers the AIR it proved last -- the first such job, not the longest proof
    idle[PP] = 1;  // (the asking context counts itself as idle, as in the pool)
    CHECK(*pick_job(s.q, PP, idle, false) == p1);
    idle.clear();
    idle[ML] = 1;
    CHECK(*pick_job(s.q, ML, idle, false) == m1);
    // a fresh context (no AIR yet): the longest proof first -- FP12Mul's rank is the highest
    idle.clear();
    idle[-1] = 1;
    CHECK(*pick_job(s.q, -1, idle, false) == f1);
    // ... but not a job whose AIR an idle context knows
    idle[F12] = 1;
    CHECK(*pick_job(s.q, -1, idle, false) == m1);
    idle[ML] = 2;
    CHECK(*pick_job(s.q, -1, idle, false) == p1);  // equal ranks: arrival order
    idle[PP] = 1;
    CHECK(pick_job(s.q, -1, idle, false) == s.q.end());  // every queued AIR has an idle context of its own: leave them to those
    idle[F12] = 0;  // an entry that counts nobody blocks nothing
    CHECK(*pick_job(s.q, -1, idle, false) == f1);
    // its own AIR wins even when others idle know it too
    CHECK(*pick_job(s.q, PP, idle, false) == p1);
    (void)p2;
    // big contexts take the FIRST eligible job, whatever its rank
    const int ECC = STARKHIP_AIR_ECC_AGGREGATE;
    Queue b;
    Job* e1 = b.add(ECC);
    Job* fe1 = b.add(FE);
    Job* fe2 = b.add(FE);
    std::map<int, int> idle_big;
    idle_big[-1] = 1;
    CHECK(*pick_job(b.q, -1, idle_big, true) == e1);
    CHECK(*pick_job(b.q, FE, idle_big, true) == fe1);
    idle_big[ECC] = 1;
    CHECK(*pick_job(b.q, -1, idle_big, true) == fe1);
    idle_big[FE] = 1;
    CHECK(pick_job(b.q, -1, idle_big, true) == b.q.end());
    (void)fe2;
    Queue none;
    CHECK(pick_job(none.q, FE, idle_big, true) == none.q.end());
    return 0;
}

int main() {
    if (int rc = recordings()) return rc;
    if (int rc = contexts()) return rc;
    printf("pickers: ok\n");
    return 0;
}
