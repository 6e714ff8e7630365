// The jobs of a proof pool apart from its threads (pool.h): recording a witness job's trace, and the rules that say which queued job
// goes next.
#include "pool.h"

#include <new>

#include "scheduler.h"
#include "trace_log.h"

namespace starkhip {

int witness_limbs(int air) {
    switch (air) {
        case STARKHIP_AIR_FP12_MUL: return 288;
        case STARKHIP_AIR_FINAL_EXP: return 144;
        case STARKHIP_AIR_MILLER_LOOP: return 96;
        case STARKHIP_AIR_PAIRING_PRECOMP: return 72;
        case STARKHIP_AIR_ECC_AGGREGATE: return 512 * 24 + 512;
        case STARKHIP_AIR_TEST_FIBONACCI: return 4;
        default: return -1;
    }
}

namespace {

// the ONE starkhip_trace_* call of `air` on packed operands (layouts: starkhip_pool_submit_witness in starkhip.h)
int run_generator(int air, const uint32_t* w, size_t n_rows, uint64_t* pis, uint64_t* rows) {
    switch (air) {
        case STARKHIP_AIR_FP12_MUL: return starkhip_trace_fp12_mul(w, w + 144, nullptr, n_rows, pis);
        case STARKHIP_AIR_FINAL_EXP: return starkhip_trace_final_exp(w, nullptr, n_rows, pis);
        case STARKHIP_AIR_MILLER_LOOP: return starkhip_trace_miller_loop(w, w + 12, w + 24, w + 48, w + 72, nullptr, n_rows, pis);
        case STARKHIP_AIR_PAIRING_PRECOMP: return starkhip_trace_pairing_precomp(w, w + 24, w + 48, nullptr, n_rows, pis);
        case STARKHIP_AIR_ECC_AGGREGATE: {
            std::vector<uint8_t> bits(512);
            for (int i = 0; i < 512; i++) bits[i] = (uint8_t)(w[512 * 24 + i] != 0);
            return starkhip_trace_ecc_aggregate(w, bits.data(), nullptr, n_rows, pis);
        }
        case STARKHIP_AIR_TEST_FIBONACCI:
            return starkhip_trace_fibonacci((uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)w[2] | ((uint64_t)w[3] << 32), rows, n_rows, pis);
        default: return STARKHIP_ERR_BAD_AIR;
    }
}

}  // namespace

// the recording itself, on `tt` threads: the job's public inputs and its log (the toy AIR: plain rows)
int record_witness(Job* j, int tt) {
    int rc = STARKHIP_OK;
    try {
        set_thread_trace_threads(tt);
        const AirInfo* a = air_get(j->air);
        j->own_pis.assign(a->pis, 0);
        if (j->air == STARKHIP_AIR_TEST_FIBONACCI) {  // plain rows
            j->own_rows.assign((size_t)a->default_rows * a->cols, 0);
            rc = run_generator(j->air, j->operands.data(), a->default_rows, j->own_pis.data(), j->own_rows.data());
        } else {
            rc = starkhip_trace_log_begin(&j->own_log);
            if (rc == STARKHIP_OK) {
                rc = run_generator(j->air, j->operands.data(), a->default_rows, j->own_pis.data(), nullptr);
                const int rc_end = starkhip_trace_log_end(j->own_log);
                if (rc == STARKHIP_OK) rc = rc_end;
            }
        }
        set_thread_trace_threads(0);
    } catch (const std::bad_alloc&) {
        rc = STARKHIP_ERR_OOM;
    } catch (const std::exception&) {
        rc = STARKHIP_ERR_BAD_SHAPE;
    }
    if (rc != STARKHIP_OK && j->own_log) {
        starkhip_trace_log_free(j->own_log);
        j->own_log = nullptr;
    }
    return rc;
}

// Expected length of a small proof, for ordering only: the permutations per leaf of its commitment; trivial recordings first.
unsigned long small_rank(const Job* j) {
    const AirInfo* a = air_get(j->air);
    if (!a) return 0;
    return (unsigned long)a->cols + (a->default_rows <= 64 ? 1000000ul : 0ul);
}

// Order by need, not by arrival.  FinalExp-class recordings are the long pole of a signature, so the first ones
// go first -- as many as there are contexts to prove them, plus one in reserve -- then the small AIRs' (their
// proofs fill the chip beside the first FinalExp proofs), then the FinalExp traces that will wait for a context
// anyway.  Few recordings run at once, each on many threads (trace_threads_for_call): the FIRST trace of each
// class is ready after tens of milliseconds instead of all of them after hundreds.
// Among the small AIRs' the LONGEST proof first (a small proof is a latency chain of cols / 8 permutations per
// leaf: MillerLoop 12 167, FP12Mul 7 536, PairingPrecomp 3 672), so that the batch does not end on one; recordings
// that cost nothing (FP12Mul: 16 rows) before all others -- their proofs are 2-wave chains that start at once.
std::deque<Job*>::iterator pick_recording(std::deque<Job*>& q_gen, size_t big_recordings_started, size_t big_wanted) {
    auto it = q_gen.end();
    const bool want_big = big_recordings_started < big_wanted;
    for (auto k = q_gen.begin(); k != q_gen.end(); ++k)
        if ((*k)->big == want_big && (it == q_gen.end() || (!want_big && small_rank(*k) > small_rank(*it)))) it = k;
    if (it == q_gen.end())  // none of the wanted class: the best of the other
        for (auto k = q_gen.begin(); k != q_gen.end(); ++k)
            if (it == q_gen.end() || (want_big && small_rank(*k) > small_rank(*it))) it = k;
    return it;
}

// A context keeps the tables, the constraint plan and -- above all -- device buffers sized for the AIRs it has proven
// (growing them means hipFree + hipMalloc, and hipFree waits for every kernel on the device).  So a waiting job goes to
// a context that proved its AIR last if one is idle; a context takes another AIR only when no idle one matches it.
std::deque<Job*>::iterator pick_job(std::deque<Job*>& q, int last_air, const std::map<int, int>& idle, bool big) {
    for (auto k = q.begin(); k != q.end(); ++k)
        if ((*k)->air == last_air) return k;
    auto it = q.end();
    for (auto k = q.begin(); k != q.end(); ++k) {
        auto f = idle.find((*k)->air);
        if (f != idle.end() && f->second != 0) continue;  // somebody idle knows this AIR better
        if (it == q.end() || (!big && small_rank(*k) > small_rank(*it))) it = k;  // the longest proof first
        if (big) break;
    }
    return it;
}

}  // namespace starkhip
