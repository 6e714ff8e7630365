// VerifyService (verify_service.h): a proof pool's device verifier.
#include "verify_service.h"

#include <pthread.h>
#include <string.h>
#include <sys/resource.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <new>

#include "blob_arena.h"
#include "scheduler.h"
#include "verify_chunk.h"

namespace starkhip {

namespace {
double steady_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
const size_t RESULT_WORDS = (size_t)1 << 19;  // page-locked result words per half (a status per query, a range flag per proof)
int hip_code(hipError_t e) {
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? STARKHIP_ERR_OOM : STARKHIP_ERR_HIP;
}
}  // namespace

struct VerifyService::Req {
    int air = 0;
    starkhip_config_t cfg;
    const uint64_t* proof = nullptr;
    size_t words = 0;
    void* tag = nullptr;
    VerifyItem it;
    size_t bytes = 0;          // device bytes in a chunk
    double t_prelude = 0, t_ready = 0;
};

struct VerifyService::Half {
    unsigned index = 0;
    void* base = nullptr;
    size_t cap = 0;
    uint32_t* results = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // before the upload, before the kernels, after the read-back
    bool busy = false, whole = false;
    VerifyChunk ch;
    std::vector<Req*> reqs;
};

VerifyService::VerifyService(int device, size_t arena_bytes, double gather_ms, unsigned prelude_threads, int nice, Done done)
    : device_(device), arena_bytes_(arena_bytes), gather_ms_(gather_ms), n_prelude_(std::max(1u, prelude_threads)), nice_(nice), done_(done) {}

int VerifyService::start() {
    int prev = -1;
    (void)hipGetDevice(&prev);
    hipError_t e = hipSetDevice(device_);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st_, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&arena_, arena_bytes_);
    if (e == hipSuccess) e = hipHostMalloc((void**)&results_, 2 * RESULT_WORDS * 4, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc(&staging_.mem, 2 * VERIFY_STAGING_HALF, hipHostMallocDefault);
    staging_.lazy = false;
    for (hipEvent_t& ev : staging_.sev)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    for (unsigned i = 0; i < 2; i++) {
        halves_[i] = new Half();
        halves_[i]->index = i;
        halves_[i]->base = (char*)arena_ + i * (arena_bytes_ / 2);
        halves_[i]->cap = arena_bytes_ / 2;
        halves_[i]->results = results_ + i * RESULT_WORDS;
        for (hipEvent_t& ev : halves_[i]->ev)
            if (e == hipSuccess) e = hipEventCreate(&ev);
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) return hip_code(e);
    stats_.arena_bytes = arena_bytes_;
    started_ = true;
    for (unsigned i = 0; i < n_prelude_; i++) threads_.emplace_back([this] { prelude_loop(); });
    threads_.emplace_back([this] { batch_loop(); });
    threads_.emplace_back([this] { complete_loop(); });
    return STARKHIP_OK;
}

VerifyService::~VerifyService() {
    {
        std::lock_guard<std::mutex> g(mu_);
        stop_ = true;
    }
    cv_pre_.notify_all();
    cv_batch_.notify_all();
    cv_done_.notify_all();
    for (std::thread& t : threads_) t.join();
    if (st_) (void)hipStreamSynchronize(st_);
    for (Half* h : halves_) {
        if (!h) continue;
        for (hipEvent_t ev : h->ev)
            if (ev) (void)hipEventDestroy(ev);
        delete h;
    }
    for (hipEvent_t ev : staging_.sev)
        if (ev) (void)hipEventDestroy(ev);
    if (arena_) (void)hipFree(arena_);
    if (results_) (void)hipHostFree(results_);
    if (staging_.mem) (void)hipHostFree(staging_.mem);
    if (st_) (void)hipStreamDestroy(st_);
}

void VerifyService::submit(int air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words, void* tag) {
    Req* r = new (std::nothrow) Req();
    if (!r) {
        done_(tag, STARKHIP_ERR_OOM, steady_s());
        return;
    }
    r->air = air;
    r->cfg = cfg;
    r->proof = proof;
    r->words = words;
    r->tag = tag;
    {
        std::lock_guard<std::mutex> g(mu_);
        q_pre_.push_back(r);
    }
    cv_pre_.notify_one();
}

VerifyService::Stats VerifyService::stats() {
    std::lock_guard<std::mutex> g(mu_);
    return stats_;
}

void VerifyService::finish(Req* r, int code) {
    {
        std::lock_guard<std::mutex> g(mu_);
        stats_.proofs++;
        if (code != STARKHIP_OK) stats_.rejected++;
    }
    done_(r->tag, code, r->t_prelude);
    delete r;
}

void VerifyService::prelude_loop() {
    pthread_setname_np(pthread_self(), "starkhip-vpre");
    if (nice_ > 0) (void)setpriority(PRIO_PROCESS, (id_t)syscall(SYS_gettid), nice_);  // as the generator threads: feeding the GPU comes first
    while (true) {
        Req* r;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_pre_.wait(lk, [&] { return stop_ || !q_pre_.empty(); });
            if (q_pre_.empty()) return;
            r = q_pre_.front();
            q_pre_.pop_front();
            pre_running_++;
        }
        const uint64_t cpu0 = thread_cpu_ns();
        r->t_prelude = steady_s();
        try {
            verify_prelude_item(r->air, r->cfg, r->proof, r->words, &r->it);
        } catch (const std::bad_alloc&) {
            r->it.queries = false;
            r->it.code = STARKHIP_ERR_OOM;
        }
        const double t1 = steady_s();
        bool queued = false;
        {
            std::lock_guard<std::mutex> g(mu_);
            stats_.prelude_ms += (t1 - r->t_prelude) * 1e3;
            stats_.prelude_cpu_s += (double)(thread_cpu_ns() - cpu0) * 1e-9;
            pre_running_--;
            if (r->it.queries) {
                r->bytes = verify_device_bytes(r->it.pre.pl);
                r->t_ready = t1;
                ready_.push_back(r);
                queued = true;
            }
        }
        cv_batch_.notify_all();  // a proof is ready, or one fewer prelude is under way
        if (!queued) finish(r, r->it.code);  // failed its prelude: not uploaded
    }
}

void VerifyService::batch_loop() {
    pthread_setname_np(pthread_self(), "starkhip-verify");
    (void)hipSetDevice(device_);
    std::unique_lock<std::mutex> lk(mu_);
    while (true) {
        cv_batch_.wait(lk, [&] { return !ready_.empty() || (stop_ && q_pre_.empty() && pre_running_ == 0); });
        if (ready_.empty()) break;
        Req* head = ready_.front();
        const size_t half_cap = arena_bytes_ / 2;
        if (head->bytes + VERIFY_CARVE_SLACK > arena_bytes_ || head->it.pre.pl.n_queries + 1 > 2 * RESULT_WORDS) {
            ready_.pop_front();
            lk.unlock();
            const int code = run_alone(head);
            finish(head, code);
            lk.lock();
            continue;
        }
        const bool whole = head->bytes + VERIFY_CARVE_SLACK > half_cap || head->it.pre.pl.n_queries + 1 > RESULT_WORDS;
        Half* h = nullptr;
        if (whole) {
            if (!halves_[0]->busy && !halves_[1]->busy) h = halves_[0];
        } else {
            for (Half* c : halves_)
                if (!c->busy) {
                    h = c;
                    break;
                }
        }
        if (!h) {  // the completion thread frees a half and says so
            cv_batch_.wait(lk);
            continue;
        }
        // what of the ready proofs fits this half, in the order their preludes finished
        const size_t cap = whole ? arena_bytes_ : half_cap, res_cap = whole ? 2 * RESULT_WORDS : RESULT_WORDS;
        size_t n = 0, bytes = VERIFY_CARVE_SLACK, res = 0;
        bool full = false;
        for (Req* r : ready_) {
            const size_t rr = r->it.pre.pl.n_queries + 1;
            if (n > 0 && (whole || bytes + r->bytes > cap || res + rr > res_cap)) {
                full = true;
                break;
            }
            bytes += r->bytes;
            res += rr;
            n++;
        }
        const bool more_coming = !q_pre_.empty() || pre_running_ > 0;
        const double waited_ms = (steady_s() - head->t_ready) * 1e3;
        if (!full && more_coming && !stop_ && waited_ms < gather_ms_) {  // gather: wake up when something arrives or the window closes
            const double left_ms = std::max(0.1, gather_ms_ - waited_ms);
            cv_batch_.wait_until(lk, std::chrono::system_clock::now() + std::chrono::microseconds((long)(left_ms * 1e3)));
            continue;
        }
        std::vector<Req*> reqs(ready_.begin(), ready_.begin() + (long)n);
        ready_.erase(ready_.begin(), ready_.begin() + (long)n);
        h->busy = true;
        h->whole = whole;
        if (whole) halves_[1]->busy = true;
        lk.unlock();
        const int code = launch(*h, reqs, whole);
        lk.lock();
        if (code == STARKHIP_OK) {
            inflight_.push_back(h);
            stats_.batches++;
            cv_done_.notify_all();
            continue;
        }
        h->busy = false;
        if (whole) halves_[1]->busy = false;
        h->reqs.clear();
        lk.unlock();
        for (Req* r : reqs) finish(r, code);
        lk.lock();
    }
    batch_done_ = true;
    lk.unlock();
    cv_done_.notify_all();
}

// one batch into half `h` (whole: the whole arena): descriptors and proof regions up, the kernel chain, the result words back
int VerifyService::launch(Half& h, std::vector<Req*>& reqs, bool whole) {
    h.ch = VerifyChunk();
    h.reqs = reqs;
    for (size_t k = 0; k < reqs.size(); k++) verify_chunk_add(h.ch, k, reqs[k]->it.pre);
    verify_chunk_seal(h.ch);
    VerifyDevBufs b;
    if (!verify_bufs_carve(h.ch, h.base, whole ? arena_bytes_ : h.cap, &b)) return STARKHIP_ERR_OOM;
    hipError_t e = hipEventRecord(h.ev[0], st_);
    if (e == hipSuccess) e = verify_chunk_upload_descriptors(h.ch, b, st_);
    for (size_t k = 0; k < reqs.size() && e == hipSuccess; k++) {
        VerifyPiece pc[2];
        verify_pieces(h.ch, k, reqs[k]->proof, reqs[k]->it.pre.pl, pc);
        const bool pinned = blob_is_pinned(reqs[k]->proof, reqs[k]->words * 8);
        for (const VerifyPiece& p : pc)
            if (e == hipSuccess) e = staging_.copy(b.words + p.dst, p.src, p.words, pinned, st_);
    }
    if (e == hipSuccess) e = hipEventRecord(h.ev[1], st_);
    if (e == hipSuccess) e = verify_chunk_launch(h.ch, b, st_);
    const size_t nq = h.ch.query_proof.size(), np = h.ch.proofs.size();
    if (e == hipSuccess && nq) e = hipMemcpyAsync(h.results, b.status, nq * 4, hipMemcpyDeviceToHost, st_);
    if (e == hipSuccess) e = hipMemcpyAsync(h.results + nq, b.bad, np * 4, hipMemcpyDeviceToHost, st_);
    if (e == hipSuccess) e = hipEventRecord(h.ev[2], st_);
    if (e != hipSuccess) {
        const int code = hip_code(e);
        (void)hipStreamSynchronize(st_);  // the service's own stream: nothing may still read the callers' proofs
        return code;
    }
    return STARKHIP_OK;
}

// a proof larger than the whole arena: alone, in buffers of its own (the only allocation after setup; "verify_arena_mb" too small
// for the proofs it is given)
int VerifyService::run_alone(Req* r) {
    VerifyChunk ch;
    verify_chunk_add(ch, 0, r->it.pre);
    verify_chunk_seal(ch);
    const size_t bytes = ch.bytes + VERIFY_CARVE_SLACK;
    void* mem = nullptr;
    hipError_t e = hipMalloc(&mem, bytes);
    if (e != hipSuccess) return hip_code(e);
    VerifyDevBufs b;
    verify_bufs_carve(ch, mem, bytes, &b);
    e = verify_chunk_upload_descriptors(ch, b, st_);
    VerifyPiece pc[2];
    verify_pieces(ch, 0, r->proof, r->it.pre.pl, pc);
    const bool pinned = blob_is_pinned(r->proof, r->words * 8);
    for (const VerifyPiece& p : pc)
        if (e == hipSuccess) e = staging_.copy(b.words + p.dst, p.src, p.words, pinned, st_);
    if (e == hipSuccess) e = verify_chunk_launch(ch, b, st_);
    std::vector<uint32_t> status(ch.query_proof.size()), bad(1);
    if (e == hipSuccess) e = hipMemcpyAsync(status.data(), b.status, status.size() * 4, hipMemcpyDeviceToHost, st_);
    if (e == hipSuccess) e = hipMemcpyAsync(bad.data(), b.bad, 4, hipMemcpyDeviceToHost, st_);
    const hipError_t es = hipStreamSynchronize(st_);
    if (e == hipSuccess) e = es;
    (void)hipFree(mem);
    if (e != hipSuccess) return hip_code(e);
    const size_t nq = r->it.pre.pl.n_queries;
    int code = STARKHIP_OK;
    verify_chunk_codes(ch, status.data(), bad.data(), &nq, &code);
    std::lock_guard<std::mutex> g(mu_);
    stats_.batches++;
    return code;
}

void VerifyService::complete_loop() {
    pthread_setname_np(pthread_self(), "starkhip-vdone");
    (void)hipSetDevice(device_);
    while (true) {
        Half* h;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_done_.wait(lk, [&] { return !inflight_.empty() || batch_done_; });
            if (inflight_.empty()) return;
            h = inflight_.front();
        }
        hipError_t e = event_wait_sleeping(h->ev[2]);
        float up = 0, dev = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&up, h->ev[0], h->ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&dev, h->ev[1], h->ev[2]);
        std::vector<int> codes(h->reqs.size(), e == hipSuccess ? STARKHIP_OK : hip_code(e));
        if (e == hipSuccess) {
            std::vector<size_t> nq(h->reqs.size());
            for (size_t k = 0; k < nq.size(); k++) nq[k] = h->reqs[k]->it.pre.pl.n_queries;
            verify_chunk_codes(h->ch, h->results, h->results + h->ch.query_proof.size(), nq.data(), codes.data());
        }
        std::vector<Req*> reqs;
        reqs.swap(h->reqs);
        {
            std::lock_guard<std::mutex> g(mu_);
            inflight_.pop_front();
            stats_.upload_ms += up;
            stats_.device_ms += dev;
            h->busy = false;
            if (h->whole) halves_[1]->busy = false;
            h->whole = false;
        }
        cv_batch_.notify_all();
        for (size_t k = 0; k < reqs.size(); k++) finish(reqs[k], codes[k]);
    }
}

}  // namespace starkhip
