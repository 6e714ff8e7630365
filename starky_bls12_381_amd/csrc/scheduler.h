// In-library scheduling of many proofs on one GPU (starkhip_pool_*, include/starkhip.h).
//
// The reference's caller issues its proves one after the other on one thread (/root/reference/src/aggregate_proof.rs:304-370)
// and leaves all parallelism to rayon inside prove().  On a GPU the proofs of one or many signature checks are what fills the
// chip, so the library itself keeps several in flight: a pool of prover contexts with one host thread each, generator threads
// that record traces, and ONE place that decides when a Merkle commitment -- the kernel that owns the chip -- is launched:
//
//  * HashService: every trace commitment of a pooled context goes through it.  The FinalExp-class commitment is a one-shot
//    grid of exactly two 188-register waves per SIMD (kernels_hash.hip): a foreign long-lived wave on a SIMD pushes one of
//    them into a second round and doubles the launch.  The 1024-row AIRs' commitments are the opposite: 128 .. 256 waves of
//    up to 12 167 sequential permutations, 7/8 of the chip idle.  So: commitments of the small class that arrive together are
//    launched as ONE merged grid (leaf_hash_multi_kernel, grid.y = proof); optionally (policy 1) the two classes never
//    overlap -- a big commitment then starts when the small window has drained and vice versa.
//
// The stream budget.  The HIP runtime carries the streams of a process on GPU_MAX_HW_QUEUES hardware queues PER PRIORITY CLASS (HIP's
// default, and what a host that has used HIP before the first pool is left with: 4); streams of one class beyond that share queues, and a
// kernel waits for everything enqueued earlier on ITS QUEUE, whatever the stream (tools/experiments/hw_queue_probe.hip,
// profiles/hwq_probe_4_queues.txt: one 100 ms kernel holds 2 of 11 other default-class streams, four hold all of them, one on a stream of
// another priority class holds none).  A pool of eight big contexts has busy at once, by class:
//    default   8 context streams + its small contexts' streams + one stream per merged small window + the verifier's      (>= 10)
//    lowest    the long launches -- a lane-form group as ONE grid, the lone pair-form commitment: N_LONG_STREAMS = 2
//    highest   nothing, unless the pool was made with stream_priority (then: urgent contexts' streams, one urgent commitment stream)
// The launches that last hundreds of milliseconds are alone in their class: no short kernel of a context can be enqueued behind one.
// The context streams still share the default class's queues among themselves (POOL_STREAM_BUDGET against the value in effect:
// starkhip_hw_queues_status), behind kernels of tens of milliseconds at most.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "gl.h"
#include "kernels.h"  // LeafHashSent

namespace starkhip {

unsigned cpu_budget();  // CPUs this process may really use (cgroup quota, affinity mask; multipool.cpp)
uint64_t thread_cpu_ns();  // trace_tasks.cpp: CPU time of the calling thread
void set_thread_trace_threads(int n);  // capi.cpp: trace_threads() of the calling thread (0 = the process-wide setting)
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
hipError_t event_wait_sleeping(hipEvent_t ev);  // ctx.hip: a few queries, then sleeps of 20 .. 200 microseconds between them
extern std::atomic<uint64_t> g_wait_cpu_ns;     // ctx.hip: CPU time inside the context threads' waits for the device

// Default-class streams a pool can have busy at once (the header comment): a stream per context and a merged small window; the pool of
// eight big contexts and one small one that the benchmark runs: 10.  Capped at the 16 queues the library asks for by itself (24 measured
// slower than 16).  Below it, contexts share hardware queues: starkhip_pool_create says so once on stderr.
inline unsigned pool_stream_budget(unsigned big_contexts, unsigned small_contexts) { return std::min(16u, big_contexts + small_contexts + 1u); }

class HashService {
  public:
    static bool is_big(unsigned log_n, unsigned rate_bits) { return log_n + rate_bits >= 15; }  // >= 2048 waves: fills every SIMD twice
#ifndef STARKHIP_QUEUED_WAIT_MS
#define STARKHIP_QUEUED_WAIT_MS 300.0
#endif
    // What the pool decides once, before the service starts (pool_create); never written afterwards.
    struct Config {
        double gather_ms = 25.0;  // how long a small window waits for announced proofs that have not reached their commitment
        // 0 (default): small commitments that arrive together share a launch, and a big one starts whenever it arrives;
        // 1: in addition the two classes never overlap (a big commitment waits for the small window to drain and vice versa).
        // Measured on one MI355X: a batch of 8 signatures 3.5 against 3.2 signatures/s, one signature 0.42
        // against 0.47 s -- a lone wave on a SIMD runs about twice as fast as one of two, so a FinalExp commitment that starts
        // beside a MillerLoop latency chain loses less than it would by waiting for it.
        int policy = 0;
        bool big_lane = false;    // big commitments in groups, a group of two or more in the lane form (one lane per leaf): pools with five or
                                  // more big contexts; STARKHIP_POOL_BIG_LANE=0 / 1 overrides
        unsigned lane_group = 4;  // STARKHIP_POOL_LANE_GROUP: commitments per lane-form group (four fill the chip: two waves of 256 registers per SIMD)
        bool lane_grouped = true; // a lane-form group is ONE grid on a long-launch stream; STARKHIP_POOL_LANE_GROUPED=0: a launch per commitment, each on a
                                  // default-class stream of its own (what the pool did before; for A/B runs)
        double big_gather_ms = 1000.0;  // lane form: how long a group of big commitments waits at most for proofs that HAVE STARTED to join (a group of three
                                        // wastes a quarter of a 350 ms launch: full groups measured 6.46 against 6.2 - 6.3 proofs/s with a 150 ms bound)
        double big_queued_wait_ms = STARKHIP_QUEUED_WAIT_MS;  // ... and for jobs that have not started (queued, or being recorded) when nobody who has started is on the
                                             // way: a recording plus upload plus LDE -- what the soonest of them needs -- not the full bound (a short batch,
                                             // or the tail of one, would otherwise hold a commitment for several proof lengths)
        int big_contexts = 0;    // the pool's number of big contexts: when all of them wait here, nobody else can come
        size_t row_leaves = 64;  // STARKHIP_POOL_ROW_LEAVES: small commitments of at most this many leaves go out in the row form, one launch each (0: never)
    };
    HashService(int device, const Config& cfg);
    ~HashService();
    HashService(const HashService&) = delete;
    HashService& operator=(const HashService&) = delete;

    // A pooled proof of the small class announces itself when it starts and calls hash() (or abandon()) exactly once: the
    // service holds a small window open while announced proofs have not arrived yet (bounded by `gather_ms`).
    void announce_small();
    void announce_big();   // a FinalExp-class proof has started: its commitment will come (lane-form groups wait for it)
    void abandon_big();
    void abandon_small();
    void set_big_queued(int n);  // the pool's count of big jobs that have not started yet (queued, or their trace being recorded)
    // Leaf digests of the coset-major LDE `mat` (kernels_hash.hip: launch_leaf_hash_form) into `digests`, ordered after everything
    // enqueued on `st` so far; when this returns, `st` has been made to wait for the launch (the caller goes on enqueueing).
    // `ready` / `done` are events owned by the caller's context.
    // `timing` (optional): two timing-enabled events of the caller's, recorded on the LAUNCH stream right before and after the kernel
    // that hashes this commitment (its own duration, not the wait for its group), and how it went out: form = a LeafHashSent
    // (kernels.h); group = commitments launched side by side with it.
    struct Timing {
        hipEvent_t t0 = nullptr, t1 = nullptr;
        int form = SENT_QUAD;
        unsigned group = 1;
    };
    // `prefix`: the caller's saved state past an identity prefix (kernels.h: LeafPrefix) for the lane and pair forms; a group may mix
    // members with and without one.
    hipError_t hash(const gl_t* mat, size_t n_cols, unsigned log_n, unsigned rate_bits, gl_t* digests, hipStream_t st, hipEvent_t ready,
                    hipEvent_t done, bool announced, bool urgent = false, Timing* timing = nullptr, LeafPrefix prefix = LeafPrefix());

    const Config cfg;

    struct Stats {
        unsigned long big_launches = 0, small_launches = 0, small_requests = 0, max_merged = 0;
        unsigned long big_grids = 0;  // kernel launches behind big_launches (commitments): a lane-form group is one
    };
    Stats stats();

  private:
    struct Req {
        const gl_t* mat;
        gl_t* digests;
        size_t n_cols;
        unsigned log_n, rate_bits;
        hipEvent_t ready, done;
        bool big, urgent = false;
        int state = 0;  // 0 queued, 1 launched, 2 failed
        int ready_state = 0;  // 0: the work that produces `mat` is still running (`ready` not reached), 1: it has run, 2: it failed (under mu_)
        hipError_t err = hipSuccess;
        double t_arrive = 0;
        Timing* timing = nullptr;
        LeafPrefix prefix;
    };
    void run();
    double big_wait_bound() const;  // under mu_: how long the oldest queued big commitment waits at most for its group to fill
    hipError_t wait_ready(Req* r);  // the service thread, before it launches r's kernel: sleeps until r's caller has seen `ready`
    void launch_big(Req* r, bool lane, unsigned group);
    unsigned launch_big_group(std::vector<Req*>& group);
    void launch_small(std::vector<Req*>& reqs);
    void drain(std::vector<hipEvent_t>& evs);
    void track(std::vector<hipEvent_t>& evs, hipEvent_t done);

    int device_;
    // big commitments: the long-launch streams (lowest priority class) / urgent (highest class; made for the first urgent commitment)
    static const int N_LONG_STREAMS = 2;
    hipStream_t long_st_[N_LONG_STREAMS] = {}, st_high_ = nullptr;
    unsigned next_long_st_ = 0;
    hipStream_t pick_long_stream(bool urgent, hipError_t* err);
    // merged launches run side by side: each goes to a stream that is idle, so a window never queues behind an earlier one
    static const int N_SMALL_STREAMS = 12;
    hipStream_t small_st_[N_SMALL_STREAMS] = {};
    unsigned next_small_st_ = 0;
    hipStream_t pick_small_stream(hipError_t* err);
    std::mutex mu_;  // guards the queues, counters, flags and stats_ below
    std::condition_variable cv_, cv_done_;
    std::deque<Req*> big_, small_;
    int announced_ = 0;     // small proofs that have started and not yet asked for their commitment
    int big_expected_ = 0;  // big proofs that have started and not yet reached their commitment
    int big_queued_ = 0;    // big jobs of the pool that have not started
    bool stop_ = false, last_was_big_ = false;
    Stats stats_;
    std::vector<hipEvent_t> running_big_, running_small_;  // done events of launches that may still be executing (the service thread's own)
    std::thread th_;
};

}  // namespace starkhip
