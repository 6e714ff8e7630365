// The commitment scheduler of a proof pool (scheduler.h): the one thread that launches the pooled contexts' trace commitments, and the
// only part of the pool that touches HIP streams and events.
#include "scheduler.h"

#include <pthread.h>

#include <chrono>
#include <map>
#include <tuple>

#include "kernels.h"

namespace starkhip {

HashService::HashService(int device, const Config& config) : cfg(config), device_(device) { th_ = std::thread([this] { run(); }); }

HashService::~HashService() {
    {
        std::lock_guard<std::mutex> g(mu_);
        stop_ = true;
    }
    cv_.notify_all();
    th_.join();
}

void HashService::announce_small() {
    std::lock_guard<std::mutex> g(mu_);
    announced_++;
}
void HashService::abandon_small() {
    {
        std::lock_guard<std::mutex> g(mu_);
        if (announced_ > 0) announced_--;
    }
    cv_.notify_all();
}

void HashService::announce_big() {
    std::lock_guard<std::mutex> g(mu_);
    big_expected_++;
}
void HashService::set_big_queued(int n) {
    {
        std::lock_guard<std::mutex> g(mu_);
        big_queued_ = n;
    }
    cv_.notify_all();
}
void HashService::abandon_big() {
    {
        std::lock_guard<std::mutex> g(mu_);
        if (big_expected_ > 0) big_expected_--;
    }
    cv_.notify_all();
}

HashService::Stats HashService::stats() {
    std::lock_guard<std::mutex> g(mu_);
    return stats_;
}

hipError_t HashService::hash(const gl_t* mat, size_t n_cols, unsigned log_n, unsigned rate_bits, gl_t* digests, hipStream_t st, hipEvent_t ready,
                             hipEvent_t done, bool announced, bool urgent, Timing* timing, LeafPrefix prefix) {
    hipError_t e = hipEventRecord(ready, st);
    Req r;
    r.timing = timing;
    r.prefix = prefix;
    r.mat = mat; r.digests = digests; r.n_cols = n_cols; r.log_n = log_n; r.rate_bits = rate_bits; r.ready = ready; r.done = done;
    r.big = is_big(log_n, rate_bits);
    r.urgent = urgent;
    r.t_arrive = now_s();
    std::unique_lock<std::mutex> lk(mu_);
    if (announced && announced_ > 0) announced_--;
    if (r.big && big_expected_ > 0) big_expected_--;
    if (e != hipSuccess) {
        lk.unlock();
        cv_.notify_all();
        return e;
    }
    (r.big ? big_ : small_).push_back(&r);
    cv_.notify_all();
    // Both hand-overs between the caller's stream and the service's go through the HOST: the caller sleeps until its own work has
    // reached `ready` and says so; the service launches then; the caller sleeps until `done` and goes on enqueueing.  Round 5 used
    // hipStreamWaitEvent both ways -- and a thread of the HIP runtime then polls for as long as a cross-stream dependence is pending:
    // 0.92 of a core during the benchmark, 0.12 of its 0.33 CPU-seconds per proof (tools/experiments/runtime_spin_probe.hip: 65 % of a
    // core with such waits, none without; no runtime setting changed it).  The request has JOINED its window already (groups form while
    // the LDEs still run); what the host round trips cost is a few hundred microseconds of idle stream per commitment.
    lk.unlock();
    const hipError_t er = event_wait_sleeping(ready);
    lk.lock();
    r.ready_state = er == hipSuccess ? 1 : 2;
    if (er != hipSuccess) r.err = er;
    cv_done_.notify_all();
    cv_done_.wait(lk, [&] { return r.state != 0; });
    lk.unlock();
    if (r.state == 2) return r.err;
    return event_wait_sleeping(done);
}

hipError_t HashService::wait_ready(Req* r) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return r->ready_state != 0; });
    return r->ready_state == 1 ? hipSuccess : r->err;
}

void HashService::drain(std::vector<hipEvent_t>& evs) {
    for (hipEvent_t ev : evs) (void)hipEventSynchronize(ev);
    evs.clear();
}

// The stream of the long launches (scheduler.h: the stream budget): the lowest priority class, whose hardware queues no stream of the
// default class shares.  Two of them, so that a group does not wait in stream order for the tail of the one before; an urgent
// commitment (pools with stream_priority 1 only) takes the high-priority stream, made when the first one comes.
hipStream_t HashService::pick_long_stream(bool urgent, hipError_t* err) {
    *err = hipSuccess;
    int least = 0, greatest = 0;
    if (urgent) {
        if (!st_high_ && (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
                          hipStreamCreateWithPriority(&st_high_, hipStreamNonBlocking, greatest) != hipSuccess))
            st_high_ = nullptr;
        if (st_high_) return st_high_;
    }
    for (int k = 0; k < N_LONG_STREAMS; k++) {
        hipStream_t& s = long_st_[(next_long_st_ + k) % N_LONG_STREAMS];
        bool idle = false;
        if (!s) {
            *err = hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (*err == hipSuccess) *err = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least);
            if (*err != hipSuccess) return s = nullptr;
            idle = true;
        } else {
            idle = hipStreamQuery(s) == hipSuccess;
            (void)hipGetLastError();  // hipErrorNotReady from a query is not an error
        }
        if (idle) {
            next_long_st_ = (next_long_st_ + k + 1) % N_LONG_STREAMS;
            return s;
        }
    }
    hipStream_t s = long_st_[next_long_st_];
    next_long_st_ = (next_long_st_ + 1) % N_LONG_STREAMS;
    return s;
}

void HashService::launch_big(Req* r, bool lane, unsigned group) {
    const LeafHashForm form = lane ? FORM_LANE : FORM_PAIR;
    hipError_t e = hipSuccess;
    // lane-form grids launched one by one (STARKHIP_POOL_LANE_GROUPED=0) are a quarter of the chip each: they must overlap, not queue in one stream
    hipStream_t s = lane ? pick_small_stream(&e) : pick_long_stream(r->urgent, &e);
    if (e == hipSuccess) e = wait_ready(r);
    if (r->timing) {
        r->timing->form = leaf_hash_sent(form);
        r->timing->group = group;
        if (e == hipSuccess && r->timing->t0) e = hipEventRecord(r->timing->t0, s);
    }
    // a big commitment on its own: the pair form (is_big() = 32 768 leaves or more: 1 024 waves of it fill the chip)
    if (e == hipSuccess) e = launch_leaf_hash_form(form, r->mat, r->n_cols, r->log_n, r->rate_bits, r->digests, s, r->prefix);
    if (e == hipSuccess && r->timing && r->timing->t1) e = hipEventRecord(r->timing->t1, s);
    if (e == hipSuccess) e = hipEventRecord(r->done, s);
    r->err = e;
    if (e == hipSuccess) track(running_big_, r->done);
}

// A lane-form group as ONE grid (grid.y = commitment) on one long-launch stream.  A member whose `ready` failed fails alone and is left
// out; members of another shape than the first's go out in a grid of their own (FinalExp and ECCAgg commitments join the same groups).
// Returns the number of grids launched.
unsigned HashService::launch_big_group(std::vector<Req*>& group) {
    std::vector<Req*> live;
    for (Req* r : group) {
        r->err = wait_ready(r);
        if (r->err == hipSuccess) live.push_back(r);
    }
    for (Req* r : live)
        if (r->timing) {
            r->timing->form = SENT_LANE;
            r->timing->group = (unsigned)live.size();
        }
    unsigned grids = 0;
    while (!live.empty()) {
        std::vector<Req*> same, rest;
        for (Req* r : live)
            ((r->n_cols == live[0]->n_cols && r->log_n == live[0]->log_n && r->rate_bits == live[0]->rate_bits && same.size() < LEAF_HASH_MAX_BATCH) ? same : rest).push_back(r);
        LeafHashBatch B = {};
        for (size_t i = 0; i < same.size(); i++) {
            B.mat[i] = same[i]->mat;
            B.digests[i] = same[i]->digests;
            B.prefix_count[i] = same[i]->prefix.count;
            B.prefix_cap[i] = same[i]->prefix.cap;
        }
        hipError_t e = hipSuccess;
        hipStream_t s = pick_long_stream(false, &e);
        for (Req* r : same)
            if (e == hipSuccess && r->timing && r->timing->t0) e = hipEventRecord(r->timing->t0, s);
        if (e == hipSuccess) {
            e = launch_leaf_hash_lane_group(B, (unsigned)same.size(), same[0]->n_cols, same[0]->log_n, same[0]->rate_bits, s);
            grids += e == hipSuccess;
        }
        for (Req* r : same) {
            if (e == hipSuccess && r->timing && r->timing->t1) e = hipEventRecord(r->timing->t1, s);
            if (e == hipSuccess) e = hipEventRecord(r->done, s);
            r->err = e;
            if (e == hipSuccess) track(running_big_, r->done);
        }
        live.swap(rest);
    }
    return grids;
}

// Done events of launches that may still be executing.  Only policy 1 (exclusive classes) ever waits for them, so only policy 1
// keeps them; events whose launch has completed are dropped first (a context re-records its event with its next proof: a stale
// entry would make drain() wait for that later proof, and a pool that proves one class only would grow the list for ever).
void HashService::track(std::vector<hipEvent_t>& evs, hipEvent_t done) {
    if (cfg.policy != 1) return;
    size_t keep = 0;
    for (hipEvent_t ev : evs) {
        if (ev == done) continue;
        const bool finished = hipEventQuery(ev) == hipSuccess;
        (void)hipGetLastError();  // hipErrorNotReady is not an error
        if (!finished) evs[keep++] = ev;
    }
    evs.resize(keep);
    evs.push_back(done);
}

// A stream with nothing pending (a merged launch must not wait in stream order behind an earlier window's latency chain); all
// busy: the next one in turn.
hipStream_t HashService::pick_small_stream(hipError_t* err) {
    *err = hipSuccess;
    for (int k = 0; k < N_SMALL_STREAMS; k++) {
        hipStream_t& s = small_st_[(next_small_st_ + k) % N_SMALL_STREAMS];
        if (!s) {
            *err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
            next_small_st_ = (next_small_st_ + k + 1) % N_SMALL_STREAMS;
            return s;
        }
        const bool idle = hipStreamQuery(s) == hipSuccess;
        (void)hipGetLastError();  // hipErrorNotReady from a query is not an error (and must not surface at the next launch)
        if (idle) {
            next_small_st_ = (next_small_st_ + k + 1) % N_SMALL_STREAMS;
            return s;
        }
    }
    hipStream_t s = small_st_[next_small_st_];
    next_small_st_ = (next_small_st_ + 1) % N_SMALL_STREAMS;
    return s;
}

// all pending small commitments, merged by shape: one launch per (columns, rows, rate), each on a stream of its own so that
// different AIRs' windows overlap
void HashService::launch_small(std::vector<Req*>& reqs) {
    std::map<std::tuple<size_t, unsigned, unsigned>, std::vector<Req*>> groups;
    for (Req* r : reqs) groups[std::make_tuple(r->n_cols, r->log_n, r->rate_bits)].push_back(r);
    for (auto& kv : groups) {
        std::vector<Req*>& g = kv.second;
        for (size_t at = 0; at < g.size(); at += LEAF_HASH_MAX_BATCH) {
            const size_t cnt = std::min<size_t>(LEAF_HASH_MAX_BATCH, g.size() - at);
            hipError_t e = hipSuccess;
            hipStream_t s = pick_small_stream(&e);
            LeafHashBatch B = {};
            for (size_t i = 0; i < cnt && e == hipSuccess; i++) {
                B.mat[i] = g[at + i]->mat;
                B.digests[i] = g[at + i]->digests;
                e = wait_ready(g[at + i]);
            }
            const bool row_form = cfg.row_leaves && (((size_t)1 << (g[0]->log_n + g[0]->rate_bits)) <= cfg.row_leaves);
            for (size_t i = 0; i < cnt; i++)
                if (Timing* t = g[at + i]->timing) {
                    t->form = row_form ? SENT_ROW : SENT_MERGED;
                    t->group = (unsigned)cnt;
                    if (e == hipSuccess && t->t0) e = hipEventRecord(t->t0, s);
                }
            if (e == hipSuccess && row_form) {
                // the row form (16 lanes per leaf): shortest chain per leaf at 2.8 x the chip time.  Measured with every small commitment
                // of a pool in it: one signature 0.36 -> 0.38 s, a batch of 8 3.8 -> 3.3 signatures/s; only the tiny ones take it by default
                for (size_t i = 0; i < cnt && e == hipSuccess; i++)
                    e = launch_leaf_hash_form(FORM_ROW, B.mat[i], g[0]->n_cols, g[0]->log_n, g[0]->rate_bits, B.digests[i], s);
            } else if (e == hipSuccess) {
                e = launch_leaf_hash_multi(B, (unsigned)cnt, g[0]->n_cols, g[0]->log_n, g[0]->rate_bits, s);
            }
            for (size_t i = 0; i < cnt; i++) {
                Req* r = g[at + i];
                if (e == hipSuccess && r->timing && r->timing->t1) e = hipEventRecord(r->timing->t1, s);
                if (e == hipSuccess) e = hipEventRecord(r->done, s);
                r->err = e;
                if (e == hipSuccess) track(running_small_, r->done);
            }
            std::lock_guard<std::mutex> lock(mu_);
            stats_.small_launches += row_form ? cnt : 1;
            stats_.max_merged = std::max<unsigned long>(stats_.max_merged, row_form ? 1 : cnt);
        }
    }
}

// Somebody who has STARTED is on the way to the commitment (its upload and LDE are tens of milliseconds): the full bound.  Only jobs that
// have not started could still join -- a recording under way, or every context busy with a proof past its commitment: the soonest of them
// needs a recording's end, an upload and an LDE, so waiting much longer than that for a fuller group costs more than the group gains.
double HashService::big_wait_bound() const { return big_expected_ > 0 ? cfg.big_gather_ms : std::min(cfg.big_gather_ms, cfg.big_queued_wait_ms); }

void HashService::run() {
    pthread_setname_np(pthread_self(), "starkhip-hash");  // thread names: bench.py attributes host CPU time by them
    (void)hipSetDevice(device_);
    // (every stream of the service is made when the first launch needs it: pick_long_stream, pick_small_stream)
    std::unique_lock<std::mutex> lk(mu_);
    while (true) {
        cv_.wait(lk, [&] { return stop_ || !big_.empty() || !small_.empty(); });
        if (stop_ && big_.empty() && small_.empty()) break;
        // small window: ready when every announced small proof has arrived, or the oldest request has waited long enough
        bool small_ready = false;
        if (!small_.empty()) {
            const double waited = (now_s() - small_.front()->t_arrive) * 1e3;
            small_ready = announced_ <= 0 || waited >= cfg.gather_ms || stop_;
        }
        // Lane form (one lane per leaf: 176 issue slots per permutation against the pair form's 205 and the quad form's 272, but 512 waves
        // of 256 registers per commitment -- a quarter of the chip): FOUR side by side run at the issue limit, 344 ms for four against
        // 118 ms each in the pair form.  Launched one by one as they arrive they leave the chip half empty and fall into step behind each
        // other, so they go out in GROUPS: a group waits (bounded) while big proofs that have started have not reached their commitment;
        // a commitment that ends up alone goes out in the pair form.
        bool big_ready = !big_.empty();
        if (cfg.big_lane && !big_.empty()) {
            const double waited = (now_s() - big_.front()->t_arrive) * 1e3;
            // A group goes out full.  Short of four it goes out when nobody else can join soon -- no big proof is on its way to its
            // commitment and none is waiting to start -- or when the oldest request has waited its bound; a lone proof is not held up.
            // (A request joins as soon as its proof has ENQUEUED its LDE: the early launches of a staggered group hash while the late
            // ones' LDEs still run, which measured better than holding the group until every LDE has run -- profiles/r04_ab_experiments.txt.)
            const bool all_here = cfg.big_contexts > 0 && (int)big_.size() >= cfg.big_contexts;  // every context's proof is waiting in this queue
            big_ready = big_.size() >= cfg.lane_group || (big_expected_ <= 0 && big_queued_ <= 0) || all_here || waited >= big_wait_bound() || stop_;
        }
        const bool take_big = big_ready && (!small_ready || !last_was_big_);
        if (take_big) {
            std::vector<Req*> group;
            const size_t want = cfg.big_lane ? cfg.lane_group : 1u;
            while (!big_.empty() && group.size() < want) {  // in arrival order
                group.push_back(big_.front());
                big_.pop_front();
            }
            std::vector<hipEvent_t> wait_for;
            wait_for.swap(running_small_);
            lk.unlock();
            if (cfg.policy == 1) drain(wait_for);  // exclusive classes: the small window has left the chip
            const bool lane = cfg.big_lane && group.size() >= 2;
            unsigned grids = 0;
            if (lane && cfg.lane_grouped) {
                grids = launch_big_group(group);
            } else {
                for (Req* r : group) {
                    launch_big(r, lane, (unsigned)group.size());
                    grids += r->err == hipSuccess;
                }
            }
            lk.lock();
            for (Req* r : group) r->state = r->err == hipSuccess ? 1 : 2;
            stats_.big_launches += group.size();
            stats_.big_grids += grids;
            last_was_big_ = true;
            cv_done_.notify_all();
            continue;
        }
        if (small_ready) {
            std::vector<Req*> reqs(small_.begin(), small_.end());
            small_.clear();
            std::vector<hipEvent_t> wait_for;
            wait_for.swap(running_big_);
            lk.unlock();
            if (cfg.policy == 1) drain(wait_for);
            lk.lock();
            // whatever arrived while the big commitment drained joins the window
            reqs.insert(reqs.end(), small_.begin(), small_.end());
            small_.clear();
            lk.unlock();
            launch_small(reqs);
            lk.lock();
            for (Req* r : reqs) r->state = r->err == hipSuccess ? 1 : 2;
            stats_.small_requests += reqs.size();
            last_was_big_ = false;
            cv_done_.notify_all();
            continue;
        }
        // requests are pending but their window is still gathering: wake up when something arrives or its time is up
        double left_ms = 1e9;
        if (!small_.empty()) left_ms = std::min(left_ms, cfg.gather_ms - (now_s() - small_.front()->t_arrive) * 1e3);
        if (cfg.big_lane && !big_.empty()) left_ms = std::min(left_ms, big_wait_bound() - (now_s() - big_.front()->t_arrive) * 1e3);
        // (system_clock deadline = pthread_cond_timedwait: ThreadSanitizer of gcc 11 does not know pthread_cond_clockwait, which a
        // steady-clock wait_for uses, and then reports the mutex as still held)
        cv_.wait_until(lk, std::chrono::system_clock::now() + std::chrono::microseconds((long)(std::max(0.1, left_ms) * 1e3)));
    }
    lk.unlock();
    for (hipStream_t s : {long_st_[0], long_st_[1], st_high_})
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    for (hipStream_t& s : small_st_)
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
}

}  // namespace starkhip
