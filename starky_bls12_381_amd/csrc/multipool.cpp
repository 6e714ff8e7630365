// A pool per device behind one handle (starkhip_multipool_*), and what says how a process's CPUs and its jobs are shared out between
// pools: the CPU budget, the cost of a proof and of a verification per AIR, placement by longest processing time first.
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>

#include "pool.h"
#include "prover.h"
#include "scheduler.h"

namespace starkhip {

// CPUs this process may actually use: the cgroup's quota where there is one (a container that sees 256 hardware threads may be
// entitled to 16 of them -- threads beyond the quota are not slower, they are THROTTLED, kernel launches included), else the
// affinity mask.
unsigned cpu_budget() {
    unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) hw = std::max(1, CPU_COUNT(&set));
    double quota = 0, period = 0;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
        char q[64];
        if (fscanf(f, "%63s %lf", q, &period) == 2 && strcmp(q, "max") != 0) quota = atof(q);
        fclose(f);
    } else {
        FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r");
        FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
        if (fq && fp && fscanf(fq, "%lf", &quota) == 1 && fscanf(fp, "%lf", &period) == 1 && quota <= 0) quota = 0;
        if (fq) fclose(fq);
        if (fp) fclose(fp);
    }
    if (quota > 0 && period > 0) hw = std::min(hw, std::max(1u, (unsigned)(quota / period + 0.5)));
    // one process per GPU (torch.distributed.run exports LOCAL_WORLD_SIZE): the node's CPUs are shared by that many pools
    if (const char* lws = getenv("LOCAL_WORLD_SIZE")) {
        const long ranks = atol(lws);
        if (ranks > 1) hw = std::max(1u, hw / (unsigned)ranks);
    }
    return hw;
}

// What one proof of each AIR costs a pool, for placing jobs on the pools of a multi-device handle (longest processing time first):
// milliseconds per proof with the pool FULL of that AIR on one MI355X (tools/air_pool_cost.py, profiles/r06_air_pool_cost.json) -- a job's
// share of its device's time, not its latency.  One signature's six proofs add up to 214 ms, which is what a batch takes per signature
// (4.9 signatures/s).  Rounds 1-5 used the reference's CPU seconds (92 : 12.5 : 4.5 : 0.22, README.md:36-39; ECCAgg a guess of 3): the same
// order, but FP12Mul -- 32 leaves hashed on the host and a 24 ms sponge over 60 285 columns -- weighs more here than its 16 rows suggest.
// The same table as the Python plan (parallel.AIR_COST).
double air_cost(int air) {
    switch (air) {
        case STARKHIP_AIR_FINAL_EXP: return 128.0;
        case STARKHIP_AIR_MILLER_LOOP: return 24.0;
        case STARKHIP_AIR_PAIRING_PRECOMP: return 10.8;
        case STARKHIP_AIR_ECC_AGGREGATE: return 12.6;
        case STARKHIP_AIR_FP12_MUL: return 15.4;
        default: break;
    }
    // A registered AIR: an ESTIMATE, fitted by least squares to the five rows above (largest miss 2.6 ms, FP12Mul's):
    // 4.75 ms + 0.144 ms per 1000 columns (hashing, openings, the transcript) + 38.1 ms per 10^9 (row x constraint) evaluations
    // (the quotient), at the AIR's default rows (1024 when it declared none).
    if (air >= STARKHIP_AIR_CUSTOM_BASE)
        if (const AirInfo* a = air_get(air)) {
            const double rows = a->default_rows ? a->default_rows : 1024;
            return 4.75 + 0.144 * a->cols / 1e3 + 38.1 * rows * a->prog.n_constraints / 1e9;
        }
    return 0.01;
}

// What verifying one proof of each AIR costs, for spreading verify work over the pools of a multi-device handle: the CPU verifier's
// milliseconds per proof, prelude (the Fiat-Shamir replay and the AIR at zeta) plus query rounds (C / 8 permutations per opened trace
// leaf), from the 48 proofs of eight signatures (profiles/r07_verify_device_split.json: FinalExp 55 + 121, MillerLoop 51 + 159, FP12Mul
// 32 + 98, PairingPrecomp 20 + 49).  Those two parts are what the device verifier's host and device sides scale with.  ECCAgg was not
// in that batch: it takes FinalExp's figure (the same 8192 rows, the same query count).
double air_verify_cost(int air) {
    switch (air) {
        case STARKHIP_AIR_FINAL_EXP: return 176.0;
        case STARKHIP_AIR_ECC_AGGREGATE: return 176.0;
        case STARKHIP_AIR_MILLER_LOOP: return 209.8;
        case STARKHIP_AIR_FP12_MUL: return 129.6;
        case STARKHIP_AIR_PAIRING_PRECOMP: return 68.4;
        default: break;
    }
    // A registered AIR: an ESTIMATE, fitted by least squares to the four measured rows above (misses below 0.3 ms): 2.05 ms per 1000
    // columns (the query rounds hash every opened trace leaf) + 0.070 ms per 1000 constraints (the AIR at zeta in the prelude).
    if (air >= STARKHIP_AIR_CUSTOM_BASE)
        if (const AirInfo* a = air_get(air)) return 2.05 * a->cols / 1e3 + 0.070 * a->prog.n_constraints / 1e3;
    return 0.01;
}

// The reference's caller is ONE process that issues its proves from one thread (/root/reference/src/aggregate_proof.rs:304-370,
// :402-414).  For that caller to use a node of GPUs it needs no process group and no collective -- the proofs are independent
//  -- only a pool per device and a rule that says which pool a job goes to.  The rule is the Python plan's
// (signature.plan_batch): longest processing time first -- a job goes to the pool with the least outstanding cost (air_cost), a batch is
// placed in order of decreasing cost, so every device gets whole FinalExp proofs first and the small proofs fill the gaps.
struct MultiPool {
    std::vector<Pool*> pools;
    std::vector<int> devices;
    std::mutex mu;  // placement + enqueue are one step: two submitting threads see each other's jobs
};

static const unsigned TICKET_SLOT_SHIFT = 48;  // ticket of a multi-device handle = (slot + 1) << 48 | the pool's own ticket

int multipool_create(const int* devices, size_t n, const starkhip_pool_config_t& cfg, MultiPool** out) {
    if (!devices || n == 0 || n > 64) return STARKHIP_ERR_BAD_SHAPE;
    std::unique_ptr<MultiPool> mp(new MultiPool());
    // The pools come up side by side (a warmed FinalExp pool allocates 160 GB and builds its plans: seconds per device)
    std::vector<Pool*> made(n, nullptr);
    std::vector<int> rcs(n, STARKHIP_OK);
    std::vector<std::thread> th;
    for (size_t i = 0; i < n; i++)
        th.emplace_back([&, i] {
            starkhip_pool_config_t c = cfg;
            c.device = devices[i];
            try {
                rcs[i] = pool_create(c, &made[i], (unsigned)n);
            } catch (const std::bad_alloc&) {
                rcs[i] = STARKHIP_ERR_OOM;
            } catch (const std::exception&) {
                rcs[i] = STARKHIP_ERR_HIP;
            }
        });
    for (std::thread& t : th) t.join();
    int rc = STARKHIP_OK;
    for (size_t i = 0; i < n; i++)
        if (rcs[i] != STARKHIP_OK && rc == STARKHIP_OK) rc = rcs[i];
    if (rc != STARKHIP_OK) {
        for (Pool* p : made)
            if (p) pool_destroy(p);
        return rc;
    }
    mp->pools = made;
    mp->devices.assign(devices, devices + n);
    // one ordinal given several times: a rehearsal of the multi-device control flow on one card.  Legitimate (the tests do it), but its
    // figures must never pass for N devices: every pool reports how many share its device, and the process says so once.
    bool shared = false;
    for (size_t i = 0; i < n; i++) {
        unsigned same = 0;
        for (size_t k = 0; k < n; k++) same += devices[k] == devices[i];
        pool_set_pools_on_device(made[i], same);
        shared = shared || same > 1;
    }
    static std::atomic<bool> said(false);
    if (shared && !said.exchange(true))
        fprintf(stderr, "starkhip: starkhip_multipool_create was given the same device ordinal more than once -- the pools share that GPU "
                        "(a rehearsal, not a measurement of %zu devices)\n", n);
    *out = mp.release();
    return STARKHIP_OK;
}

void multipool_destroy(MultiPool* mp) {
    if (!mp) return;
    std::vector<std::thread> th;  // every pool runs what it has queued to the end: side by side
    for (Pool* p : mp->pools) th.emplace_back([p] { pool_destroy(p); });
    for (std::thread& t : th) t.join();
    delete mp;
}

size_t multipool_size(const MultiPool* mp) { return mp->pools.size(); }
Pool* multipool_pool(MultiPool* mp, size_t slot) { return slot < mp->pools.size() ? mp->pools[slot] : nullptr; }
int multipool_device(const MultiPool* mp, size_t slot) { return slot < mp->devices.size() ? mp->devices[slot] : -1; }

// the pool a job of `air` goes to (under mp->mu): for a FinalExp-class job the pool with the fewest of them open, then -- and for every
// other job -- the least outstanding cost, then the lowest slot; verify work: the least outstanding verify cost (air_verify_cost), ties
// to the lowest slot
static size_t multipool_pick(MultiPool* mp, int air, bool verify) {
    const AirInfo* a = air_get(air);
    starkhip_config_t cfg;
    bool big = false;
    if (!verify && a && starkhip_config_for_air((starkhip_air_t)air, &cfg) == STARKHIP_OK) {
        unsigned log_n = 0;
        while (((size_t)1 << log_n) < (size_t)a->default_rows) log_n++;
        big = HashService::is_big(log_n, cfg.rate_bits);
    }
    size_t best = 0;
    double best_load = 0;
    unsigned best_big = 0;
    for (size_t i = 0; i < mp->pools.size(); i++) {
        const PoolLoad l = pool_load(mp->pools[i]);
        const double load = verify ? l.verify : l.prove;
        const bool better = i == 0 || (big && l.big_open != best_big ? l.big_open < best_big : load < best_load);
        if (better) {
            best = i;
            best_load = load;
            best_big = l.big_open;
        }
    }
    return best;
}

template <class Submit>
static int multipool_place(MultiPool* mp, int air, int slot, bool verify, uint64_t* ticket, Submit submit) {
    if (!ticket || slot >= (int)mp->pools.size()) return STARKHIP_ERR_BAD_SHAPE;
    std::lock_guard<std::mutex> g(mp->mu);
    const size_t at = slot >= 0 ? (size_t)slot : multipool_pick(mp, air, verify);
    uint64_t inner = 0;
    const int rc = submit(mp->pools[at], &inner);
    if (rc == STARKHIP_OK) *ticket = ((uint64_t)(at + 1) << TICKET_SLOT_SHIFT) | inner;
    return rc;
}

int multipool_submit(MultiPool* mp, int slot, int air, const starkhip_config_t* cfg, const TraceInput& in, const uint64_t* pis, size_t n_pis, uint64_t pow,
                     uint64_t* ticket) {
    if (in.on_device && slot < 0) return STARKHIP_ERR_BAD_SHAPE;  // device memory belongs to one device: the caller says which
    return multipool_place(mp, air, slot, false, ticket, [&](Pool* p, uint64_t* t) { return pool_submit(p, air, cfg, in, pis, n_pis, pow, t); });
}
int multipool_submit_witness(MultiPool* mp, int slot, int air, const starkhip_config_t* cfg, const uint32_t* operands, size_t n_limbs, uint64_t pow,
                             uint64_t* ticket) {
    return multipool_place(mp, air, slot, false, ticket, [&](Pool* p, uint64_t* t) { return pool_submit_witness(p, air, cfg, operands, n_limbs, pow, t); });
}

// Longest processing time first on n_pools idle pools: the jobs by decreasing cost(air) (ties in the caller's order), each to the pool
// with the least cost so far (ties to the lowest slot).  order[k] = the k-th job placed; slots, order: each may be null.
static void plan_longest_first(size_t n, const int* airs, double (*cost)(int), size_t n_pools, int* slots, size_t* order) {
    std::vector<size_t> ord(n);
    for (size_t i = 0; i < n; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return cost(airs[a]) > cost(airs[b]); });
    std::vector<double> load(n_pools, 0.0);
    for (size_t k = 0; k < n; k++) {
        const size_t i = ord[k];
        if (order) order[k] = i;
        if (!slots) continue;
        size_t best = 0;
        for (size_t s = 1; s < n_pools; s++)
            if (load[s] < load[best]) best = s;
        slots[i] = (int)best;
        load[best] += cost(airs[i]);
    }
}
// the plans alone, for tests and for callers that want to see them: placement of a batch of proving jobs, of a verify batch
void plan_lpt(size_t n, const int* airs, size_t n_pools, int* slots) { plan_longest_first(n, airs, air_cost, n_pools, slots, nullptr); }
void plan_verify(size_t n, const int* airs, size_t n_pools, int* slots, size_t* order) { plan_longest_first(n, airs, air_verify_cost, n_pools, slots, order); }

// A whole batch of witness jobs, placed longest first (ties in the caller's order).  All or nothing is not promised: tickets[i] == 0 and
// rcs[i] != OK for a job that was refused; the return value is the first failure.
int multipool_submit_witness_batch(MultiPool* mp, size_t n, const int* airs, const uint32_t* const* operands, const size_t* n_limbs, uint64_t pow,
                                   uint64_t* tickets, int* rcs) {
    if (!airs || !operands || !n_limbs || !tickets) return STARKHIP_ERR_BAD_SHAPE;
    std::vector<size_t> order(n);
    plan_longest_first(n, airs, air_cost, 0, nullptr, order.data());
    int first = STARKHIP_OK;
    for (size_t i : order) {
        tickets[i] = 0;
        const int rc = multipool_submit_witness(mp, -1, airs[i], nullptr, operands[i], n_limbs[i], pow, &tickets[i]);
        if (rcs) rcs[i] = rc;
        if (rc != STARKHIP_OK && first == STARKHIP_OK) first = rc;
    }
    return first;
}

int multipool_ticket_slot(const MultiPool* mp, uint64_t ticket) {
    const uint64_t s = ticket >> TICKET_SLOT_SHIFT;
    return (s >= 1 && s <= mp->pools.size()) ? (int)(s - 1) : -1;
}

int multipool_wait(MultiPool* mp, uint64_t ticket, uint64_t** proof, size_t* words, starkhip_ticket_info_t* info) {
    const int slot = multipool_ticket_slot(mp, ticket);
    if (slot < 0) return STARKHIP_ERR_BAD_SHAPE;
    return pool_wait(mp->pools[(size_t)slot], ticket & (((uint64_t)1 << TICKET_SLOT_SHIFT) - 1), proof, words, info);
}

int multipool_set_option(MultiPool* mp, const char* name, long value) {
    int first = STARKHIP_OK;
    for (Pool* p : mp->pools) {
        const int rc = pool_set_option(p, name, value);
        if (rc != STARKHIP_OK && first == STARKHIP_OK) first = rc;
    }
    return first;
}

int multipool_submit_verify(MultiPool* mp, int slot, int air, const starkhip_config_t* cfg, const uint64_t* proof, size_t words, uint64_t* ticket) {
    return multipool_place(mp, air, slot, true, ticket, [&](Pool* p, uint64_t* t) { return pool_submit_verify(p, air, cfg, proof, words, t); });
}

// starkhip_verify_batch's contract over the handle's devices: every proof a verify job of the pool plan_verify gives it, all submitted
// (longest first) before the first wait
int multipool_verify_batch(MultiPool* mp, size_t n, const int* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs, const size_t* words,
                           int* results) {
    if (n && (!airs || !cfgs || !proofs || !words || !results)) return STARKHIP_ERR_BAD_SHAPE;
    std::vector<int> slots(n);
    std::vector<size_t> order(n);
    plan_verify(n, airs, mp->pools.size(), slots.data(), order.data());
    std::vector<uint64_t> tickets(n, 0);
    int first = STARKHIP_OK;
    for (size_t i : order) {
        const int rc = multipool_submit_verify(mp, slots[i], airs[i], &cfgs[i], proofs[i], words[i], &tickets[i]);
        if (rc != STARKHIP_OK) {
            tickets[i] = 0;
            results[i] = rc;
            if (first == STARKHIP_OK) first = rc;
        }
    }
    for (size_t i = 0; i < n; i++) {
        if (!tickets[i]) continue;
        const int rc = multipool_wait(mp, tickets[i], nullptr, nullptr, nullptr);
        results[i] = rc;
        if ((rc == STARKHIP_ERR_HIP || rc == STARKHIP_ERR_OOM) && first == STARKHIP_OK) first = rc;  // the device work failed: the call did
    }
    return first;
}

}  // namespace starkhip
