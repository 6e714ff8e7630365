// Stand-ins for the GPU entry points, linked ONLY into the sanitizer builds of the host code (make asan / tsan-test).  Not part of
// libstarkhip.so.  By default every device path answers "no device", as the real library does on a box without a GPU.
// With STARKHIP_FAKE_DEVICE=1 in the environment the stand-ins PRETEND instead: contexts can be created, prove() sleeps a few
// milliseconds, asks the pool's commitment scheduler for its "commitment" (so HashService runs its real gather / merge / launch
// logic against no-op HIP calls) and returns a blob that ends in the public inputs.  That lets ThreadSanitizer and
// AddressSanitizer run the proof pool's threads -- generators, context workers, the commitment scheduler, shutdown -- on a CPU
// (tests/tsan_pool_main.cpp); it proves nothing about proofs.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <set>
#include <thread>

#include "blob_arena.h"
#include "kernels.h"
#include "prover.h"
#include "scheduler.h"
#include "verifier.h"
#include "verify_chunk.h"
#include "verify_query.h"

namespace starkhip {
std::atomic<uint64_t> g_wait_cpu_ns(0);

static bool fake_device() {
    const char* e = getenv("STARKHIP_FAKE_DEVICE");
    return e && *e == '1';
}

struct Ctx {
    int device = 0;
    HashService* hs = nullptr;
    bool hash_requested = false, urgent = false, check_trace = false;
    std::atomic<uint64_t> traces_checked{0};
    float timings[STARKHIP_N_PHASES] = {0}, ktimings[3] = {0}, htimings[2] = {0};
    double verify_timings[4] = {0};
    std::set<int> blob_airs;
    HashService::Timing hash_timing;  // how the scheduler sent the last "commitment" out (no timing events: form and group only)
    char done_tag = 0;                // its address is this context's `done` event: the scheduler's records of it are counted
};
// a `ready` event whose wait fails (pow_witness 0xBAD3: the work before a commitment failed on the device)
static char g_failing_ready_tag = 0;
static hipEvent_t failing_ready() { return (hipEvent_t)&g_failing_ready_tag; }
int ctx_create(int device, Ctx** out, int) {
    if (!fake_device() || device < 0 || device >= 8) {  // the pretended node has eight devices
        *out = nullptr;
        return STARKHIP_ERR_NO_DEVICE;
    }
    *out = new Ctx();
    (*out)->device = device;
    return STARKHIP_OK;
}
void ctx_destroy(Ctx* c) {
    if (c) blob_arena_drop(c);
    delete c;
}
size_t ctx_device_bytes(Ctx*) { return 0; }
size_t ctx_pinned_bytes(Ctx*) { return 0; }
const float* ctx_timings(Ctx* c) { return c->timings; }
long ctx_verify_chunk_mb(Ctx*) { return 1024; }
double* ctx_verify_timings(Ctx* c) { return c->verify_timings; }
int ctx_device(Ctx* c) { return c->device; }
const float* ctx_kernel_timings(Ctx* c) { return c->ktimings; }
const float* ctx_host_timings(Ctx* c) { return c->htimings; }
void ctx_commit_info(Ctx* c, int* form, unsigned* group) { *form = c->hash_timing.form; *group = c->hash_timing.group; }
int ctx_set_option(Ctx*, const char*, long) { return STARKHIP_ERR_NO_DEVICE; }
void ctx_attach_hash_service(Ctx* c, HashService* hs) { c->hs = hs; }
bool ctx_has_hash_service(Ctx* c) { return c->hs != nullptr; }
void ctx_hash_request_reset(Ctx* c) { c->hash_requested = false; }
bool ctx_hash_requested(Ctx* c) { return c->hash_requested; }
int ctx_set_urgent(Ctx* c, bool urgent) { c->urgent = urgent; return STARKHIP_OK; }
void ctx_set_check_trace(Ctx* c, bool on, size_t) { c->check_trace = on; }  // the pretended check finds every trace satisfying
void ctx_set_fill_lookups(Ctx*, bool) {}  // the pretended proof fills nothing
void ctx_set_fill_frequencies(Ctx*, bool) {}
void ctx_set_hasher(Ctx*, int) {}
void ctx_check_stats(Ctx* c, uint64_t out[2]) { out[0] = c->traces_checked.load(); out[1] = 0; }
int ctx_reserve(Ctx* c, const AirInfo& air, const starkhip_config_t&, size_t, unsigned proof_blobs, bool) {
    if (proof_blobs && !c->blob_airs.count(air.id)) {  // the fake proofs are tiny; what is exercised is the arena's bookkeeping
        if (blob_arena_add(c, 64 + air.prog.n_pis * 8, proof_blobs) != 0) return STARKHIP_ERR_OOM;
        c->blob_airs.insert(air.id);
    }
    return STARKHIP_OK;
}

int prove(Ctx* c, const AirInfo& air, const starkhip_config_t& cfg, const TraceInput& in, const uint64_t* pis, size_t n_pis, uint64_t pow_witness,
          uint64_t** proof_out, size_t* proof_words) {
    if (!fake_device()) return STARKHIP_ERR_NO_DEVICE;
    if (n_pis != air.prog.n_pis) return STARKHIP_ERR_BAD_SHAPE;              // before the "commitment", like the real one
    if (pow_witness == 0xBAD) return STARKHIP_ERR_BAD_SHAPE;                  // a job that fails before its commitment (tests)
    const size_t n_rows = in.n_rows;
    std::this_thread::sleep_for(std::chrono::milliseconds(air.cols > 50000 ? 3 : 1));  // "upload + LDE"
    if (c->check_trace) c->traces_checked++;
    unsigned log_n = 0;
    while (((size_t)1 << log_n) < n_rows) log_n++;
    if (c->hs) {
        c->hash_requested = true;
        static gl_t dummy[8];
        c->hash_timing = HashService::Timing();
        if (c->hs->hash(dummy, air.cols, log_n, cfg.rate_bits, dummy, nullptr, pow_witness == 0xBAD3 ? failing_ready() : nullptr, (hipEvent_t)&c->done_tag,
                        !HashService::is_big(log_n, cfg.rate_bits), c->urgent, &c->hash_timing) != hipSuccess)
            return STARKHIP_ERR_HIP;
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(2));  // "the rest of the proof"
    if (pow_witness == 0xBAD2) return STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE;     // a job that fails after its commitment
    uint64_t* out = blob_alloc((4 + n_pis) * 8);
    if (!out) return STARKHIP_ERR_OOM;
    out[0] = 0xFA4EULL; out[1] = (uint64_t)air.id; out[2] = n_rows; out[3] = (uint64_t)c->urgent | ((uint64_t)c->device << 8);
    if (n_pis) memcpy(out + 4, pis, n_pis * 8);
    *proof_out = out;
    *proof_words = 4 + n_pis;
    c->timings[STARKHIP_N_PHASES - 1] = 3.0f;
    return STARKHIP_OK;
}
// the halves of prove() a system runs (system.cpp): no pretended system proofs
int prove_first_half(Ctx*, const AirInfo&, const starkhip_config_t&, const TraceInput&, const uint64_t*, size_t, uint64_t, const CtlTable*, ProveJob** job, uint64_t**, size_t*) {
    *job = nullptr;
    return STARKHIP_ERR_NO_DEVICE;
}
int prove_trace_cap(ProveJob*, const uint64_t**, size_t*) { return STARKHIP_ERR_NO_DEVICE; }
int prove_job_hasher(ProveJob*) { return 0; }
int prove_ctl_polys(ProveJob*, const uint64_t*, uint64_t*, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int prove_second_half(ProveJob*, const Challenger*, uint64_t**, size_t*) { return STARKHIP_ERR_NO_DEVICE; }
void prove_job_free(ProveJob*) {}
int ctl_polys(Ctx*, const CtlTable&, const TraceInput&, const uint64_t*, uint64_t*, uint64_t*, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int lde_batch(Ctx*, const uint64_t*, size_t, unsigned, unsigned, uint64_t*, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int ntt_long(Ctx*, uint64_t*, size_t, unsigned, int) { return STARKHIP_ERR_NO_DEVICE; }
int merkle_cap(Ctx*, const uint64_t*, size_t, unsigned, unsigned, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int permute_batch(Ctx*, uint64_t*, size_t) { return STARKHIP_ERR_NO_DEVICE; }
int permute_batch_form(Ctx*, int, int, uint64_t*, size_t) { return STARKHIP_ERR_NO_DEVICE; }
int keccak_permute_batch(Ctx*, uint64_t*, size_t) { return STARKHIP_ERR_NO_DEVICE; }
int merkle_tree_hasher(Ctx*, int, const uint64_t*, size_t, unsigned, unsigned, uint64_t*, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int hash_rows_hasher(Ctx*, int, const uint64_t*, size_t, size_t, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int leaf_hash_lane_group(Ctx*, const uint64_t*, size_t, size_t, unsigned, unsigned, int, int, unsigned, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int leaf_prefix_table(Ctx*, unsigned, unsigned, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int expand_log(Ctx*, const TraceLog*, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int check_trace(Ctx*, const AirInfo&, const TraceInput&, const uint64_t*, uint64_t*, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int check_trace_report(Ctx*, const AirInfo&, const TraceInput&, const uint64_t*, uint32_t*, uint64_t*, uint64_t*, size_t, starkhip_check_report_t*) {
    return STARKHIP_ERR_NO_DEVICE;
}
int check_trace_free_cells(Ctx*, const AirInfo&, const TraceInput&, const uint64_t*, uint64_t, uint32_t*, uint64_t*, starkhip_free_cells_t*) {
    return STARKHIP_ERR_NO_DEVICE;
}
int check_trace_free_cell_classes(Ctx*, const AirInfo&, const TraceInput&, const uint64_t*, uint64_t, uint32_t*, uint64_t*, uint32_t*,
                                  starkhip_free_cell_classes_t*) {
    return STARKHIP_ERR_NO_DEVICE;
}
int check_trace_permutations(Ctx*, const AirInfo&, const TraceInput&, uint64_t, uint32_t*, uint64_t*, uint64_t*, size_t, starkhip_perm_check_t*) {
    return STARKHIP_ERR_NO_DEVICE;
}
void perm_check_timings(Ctx*, float ms[4]) { ms[0] = ms[1] = ms[2] = ms[3] = 0; }
int lookup_columns(Ctx*, const TraceInput&, uint64_t*, const starkhip_lookup_t*, size_t, uint32_t*, uint64_t*, uint64_t*, size_t, starkhip_lookup_report_t*) {
    return STARKHIP_ERR_NO_DEVICE;
}
void lookup_timings(Ctx*, float ms[4]) { ms[0] = ms[1] = ms[2] = ms[3] = 0; }
int logup_frequencies(Ctx*, const AirInfo&, const TraceInput&, uint64_t*, uint32_t*, uint32_t*, uint64_t*, uint64_t*, size_t, starkhip_logup_report_t*) {
    return STARKHIP_ERR_NO_DEVICE;
}
void logup_frequency_timings(Ctx*, float ms[5]) { ms[0] = ms[1] = ms[2] = ms[3] = ms[4] = 0; }
int lde_bench(Ctx*, size_t, unsigned, unsigned, unsigned, unsigned, const uint64_t*, float*, float*) { return STARKHIP_ERR_NO_DEVICE; }
int field_ops(Ctx*, int, const uint64_t*, const uint64_t*, uint64_t*, size_t) { return STARKHIP_ERR_NO_DEVICE; }
int permutation_zs(Ctx*, const AirInfo&, const TraceInput&, const uint64_t*, uint64_t*, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int logup_polys(Ctx*, const AirInfo&, const TraceInput&, const uint64_t*, uint64_t*, uint64_t*, uint64_t*) { return STARKHIP_ERR_NO_DEVICE; }
int host_alloc(Ctx*, size_t, void**) { return STARKHIP_ERR_NO_DEVICE; }
void host_free(void*) {}

// ctx.hip's sleeping wait: the fake device is always done -- except with the work that the failing `ready` stands for
hipError_t event_wait_sleeping(hipEvent_t ev) { return ev == failing_ready() ? hipErrorUnknown : hipSuccess; }

// the two launches the commitment scheduler makes
static std::atomic<unsigned long> g_fake_launches(0), g_fake_merged(0), g_fake_lane_grids(0), g_fake_lane_members(0), g_service_records(0);
hipError_t launch_leaf_hash_form(LeafHashForm, const gl_t*, size_t, unsigned, unsigned, gl_t*, hipStream_t, LeafPrefix) { g_fake_launches++; return hipSuccess; }
hipError_t launch_leaf_hash_multi(const LeafHashBatch&, unsigned count, size_t, unsigned, unsigned, hipStream_t) {
    g_fake_launches++;
    g_fake_merged += count;
    return hipSuccess;
}
hipError_t launch_leaf_hash_lane_group(const LeafHashBatch& B, unsigned count, size_t, unsigned, unsigned, hipStream_t) {
    if (count == 0 || count > LEAF_HASH_MAX_BATCH) return hipErrorInvalidValue;
    for (unsigned i = 0; i < count; i++)
        if (!B.mat[i] || !B.digests[i]) return hipErrorInvalidValue;
    g_fake_launches++;
    g_fake_lane_grids++;
    g_fake_lane_members += count;
    return hipSuccess;
}
// the Keccak hasher's launches (kernels_keccak.hip): no host code calls them -- a pretended proof hashes nothing -- and the device
// verifier's Keccak leaves go through launch_verify_leaf_digests below, on the host
hipError_t launch_leaf_hash_keccak(const gl_t*, size_t, unsigned, unsigned, gl_t*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_leaf_hash_rows_keccak(const gl_t*, size_t, size_t, gl_t*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_merkle_levels_keccak(gl_t*, unsigned, unsigned, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_permute_batch_keccak(gl_t*, size_t, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_pow_grind_keccak(const gl_t*, int, unsigned, uint64_t, uint64_t, unsigned long long*, hipStream_t) { return hipErrorNoDevice; }
hipError_t launch_verify_leaf_digests_keccak(const gl_t* words, const VQLeaf* leaves, size_t n, gl_t* digests, hipStream_t) {
    if (!fake_device()) return hipErrorNoDevice;
    verify_host_leaf_digests(words, leaves, n, digests);
    return hipSuccess;
}
// the device verifier's launches (verifier_device.cpp, verify_service.cpp): with the pretended device, their routine on the host --
// the same code as starkhip_verify_batch_replay's (verify_query.h, the host permutation) on the "device" buffers, which are host memory
// here, so that a CPU build of the pool gives real verdicts; without it, no device
hipError_t launch_ext_powers(gl2_t* out, gl2_t alpha, size_t n, hipStream_t) {
    if (!fake_device()) return hipErrorNoDevice;
    verify_host_ext_powers(out, alpha, n);
    return hipSuccess;
}
hipError_t launch_verify_leaf_digests(const gl_t* words, const VQLeaf* leaves, size_t n, gl_t* digests, unsigned, hipStream_t) {
    if (!fake_device()) return hipErrorNoDevice;
    verify_host_leaf_digests(words, leaves, n, digests);
    return hipSuccess;
}
hipError_t launch_verify_range(const gl_t* words, const VQProof* proofs, size_t n, uint32_t* bad, hipStream_t) {
    if (!fake_device()) return hipErrorNoDevice;
    verify_host_range(words, proofs, n, bad);
    return hipSuccess;
}
hipError_t launch_verify_combine(const gl_t* words, const VQProof* proofs, const uint32_t* qp, size_t nq, const gl2_t* apow, gl2_t* sums, hipStream_t) {
    if (!fake_device()) return hipErrorNoDevice;
    verify_host_combine(words, proofs, qp, nq, apow, sums);
    return hipSuccess;
}
hipError_t launch_verify_queries(const gl_t* words, const VQProof* proofs, const uint32_t* qp, const uint64_t* xi, size_t nq, const gl_t* dig,
                                 const gl2_t* sums, uint32_t* status, hipStream_t) {
    if (!fake_device()) return hipErrorNoDevice;
    verify_host_queries(words, proofs, qp, xi, nq, dig, sums, status);
    return hipSuccess;
}
}  // namespace starkhip

// ---- no-op HIP runtime: only what hash_service.cpp calls (the sanitizer builds do not link libamdhip64).  Copies and fills are real (the
// "device" is host memory and every stream is synchronous); every allocation -- device, page-locked, stream -- is counted
// (starkhip_stub_allocations: the pool's verifier must not allocate after its setup)
static std::atomic<unsigned long> g_stub_allocs(0);
extern "C" unsigned long starkhip_stub_allocations(void) { return g_stub_allocs.load(); }
// what the commitment scheduler has launched and recorded so far: [0] leaf-hash launches of every kind, [1] lane-form group grids, [2] the
// commitments in them, [3] events recorded on the scheduler's own streams (the members' `done`; the fake proofs have no timing events)
extern "C" void starkhip_stub_commit_counters(unsigned long out[4]) {
    out[0] = starkhip::g_fake_launches.load(); out[1] = starkhip::g_fake_lane_grids.load(); out[2] = starkhip::g_fake_lane_members.load();
    out[3] = starkhip::g_service_records.load();
}
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { g_stub_allocs++; *s = (hipStream_t)malloc(1); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { g_stub_allocs++; *s = (hipStream_t)malloc(1); return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) { *least = 1; *greatest = -1; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free((void*)s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t s) { if (s) starkhip::g_service_records++; return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { g_stub_allocs++; *p = malloc(bytes ? bytes : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
// ... and what the device verifier's host side calls
hipError_t hipMalloc(void** p, size_t bytes) { g_stub_allocs++; *p = malloc(bytes ? bytes : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { if (n) memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { if (n) memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { if (n) memset(d, v, n); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { g_stub_allocs++; *e = (hipEvent_t)malloc(1); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { g_stub_allocs++; *e = (hipEvent_t)malloc(1); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free((void*)e); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0; return hipSuccess; }
}
