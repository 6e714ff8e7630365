// The device verifier inside a proof pool (starkhip_pool_set_option "verify_proofs", starkhip_pool_submit_verify).
//
// starkhip_verify_batch allocates its buffers, creates a stream and page-locked staging on every call, and hipFree waits for the whole
// device: beside a running pool every call would stall the pool's kernels.  The service pays for all of that once, when it starts:
//  * one non-blocking stream at normal priority, and a device arena split in two halves, so that one batch is packed and staged on
//    the host while the other's copies and kernels run; a batch's descriptors, results and proof regions are all carved out of its half;
//  * page-locked result words per half, and two 32 MB page-locked staging halves for proofs in pageable memory.
// Afterwards it allocates nothing and never synchronises the device: it waits on its own events, sleeping.
//
// Per proof, verify_prelude runs on a few host threads of the pool (at the generator threads' nice value: the threads that feed the GPU
// come first).  A proof that fails its prelude is finished at once.  The others are packed into a free half, in the order their
// preludes finish; a half goes out when it is full, or when nothing else is ready and the oldest proof in it has waited `gather_ms`.
// A proof larger than a half is verified alone in the whole arena (both halves idle), one larger than the arena in buffers of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "starkhip.h"
#include "verify_chunk.h"

namespace starkhip {

class VerifyService {
  public:
    // done(tag, code, t_prelude): the verdict of a submitted proof (starkhip_verify's code, or HIP / OOM if the device work failed) and
    // when its prelude started (steady clock, seconds).  Called on a service thread, with no lock of the service held.
    using Done = std::function<void(void* tag, int code, double t_prelude)>;
    struct Stats {
        unsigned long proofs = 0, rejected = 0, batches = 0;
        double upload_ms = 0, device_ms = 0, prelude_ms = 0, prelude_cpu_s = 0;
        uint64_t arena_bytes = 0;
    };

    VerifyService(int device, size_t arena_bytes, double gather_ms, unsigned prelude_threads, int nice, Done done);
    ~VerifyService();  // runs what was submitted to the end, then frees everything
    VerifyService(const VerifyService&) = delete;
    VerifyService& operator=(const VerifyService&) = delete;

    int start();  // the one-time setup: STARKHIP_OK, STARKHIP_ERR_OOM or STARKHIP_ERR_HIP (then the service must not be used)
    // `proof` stays the caller's until done() has been called for `tag`
    void submit(int air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words, void* tag);
    Stats stats();

  private:
    struct Req;
    struct Half;
    void prelude_loop();
    void batch_loop();
    void complete_loop();
    int launch(Half& h, std::vector<Req*>& reqs, bool whole);
    int run_alone(Req* r);  // a proof larger than the arena: buffers of its own
    void finish(Req* r, int code);

    int device_;
    size_t arena_bytes_;
    double gather_ms_;
    unsigned n_prelude_;
    int nice_;
    Done done_;

    hipStream_t st_ = nullptr;
    void* arena_ = nullptr;
    uint32_t* results_ = nullptr;  // page-locked, RESULT_WORDS per half
    VerifyStaging staging_;  // used by the batch thread only
    Half* halves_[2] = {nullptr, nullptr};
    bool started_ = false;

    std::mutex mu_;
    std::condition_variable cv_pre_, cv_batch_, cv_done_;
    std::deque<Req*> q_pre_, ready_;
    std::deque<Half*> inflight_;
    unsigned pre_running_ = 0;
    bool stop_ = false, batch_done_ = false;
    Stats stats_;
    std::vector<std::thread> threads_;
};

}  // namespace starkhip
