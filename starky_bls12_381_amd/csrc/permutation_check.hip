// starkhip_check_trace_permutations on the context's device: one pair under one seed as its sorted items (sorted_items_run, ctx.hip: keys
// and the stable sort of kernels_multiset.hip), then the classification and the masks' popcounts of kernels_multiset.hip over them --
// under the host half of permutation_check.h.  The pair columns are gathered where permutation_zs() and prove() keep them (perm.cols, by
// perm_columns()); c->mset holds one pair's buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ctx.h"
#include "kernels_multiset.h"
#include "permutation.h"
#include "permutation_check.h"

namespace starkhip {

namespace {
struct DevicePermSteps : PermCheckSteps {
    Ctx* c;
    size_t n, W;
    std::vector<uint32_t> pair_at;  // where each pair starts in mset.desc
    DevicePermSteps(Ctx* c_, size_t n_) : c(c_), n(n_), W((n_ + 63) / 64) {}
    unsigned long long* d_masks() const { return c->mset.masks.as<unsigned long long>(); }  // [2][W], then the three counters
    int run(size_t q, gl_t seed, uint64_t counts[3]) override {
        hipStream_t st = c->st;
        Ctx::MultisetBufs& mb = c->mset;
        const gl_t* keys = nullptr;
        const uint32_t* idx = nullptr;
        const uint32_t* pair = mb.desc.as<uint32_t>() + pair_at[q];
        const gl_t* cols = c->perm.cols.as<gl_t>();
        HIPCHK(hipMemsetAsync(d_masks(), 0, (2 * W + 3) * 8, st));
        HIPCHK(hipEventRecord(c->kev[2], st));
        if (int rc = sorted_items_run(c, pair, cols, n, n, seed, &keys, &idx)) return rc;
        HIPCHK(hipEventRecord(c->kev[3], st));
        HIPCHK(launch_multiset_classify(pair, cols, n, n, keys, idx, d_masks(), d_masks() + 2 * W, st));
        HIPCHK(launch_multiset_count(d_masks(), n, d_masks() + 2 * W, st));
        HIPCHK(hipEventRecord(c->kev[4], st));
        unsigned long long res[3] = {0, 0, 0};
        HIPCHK(read_back(c, res, d_masks() + 2 * W, sizeof res, st));
        HIPCHK(stream_wait(c));
        float sort_ms = 0, classify_ms = 0;
        HIPCHK(hipEventElapsedTime(&sort_ms, c->kev[2], c->kev[3]));
        HIPCHK(hipEventElapsedTime(&classify_ms, c->kev[3], c->kev[4]));
        mb.ms[1] += sort_ms;
        mb.ms[2] += classify_ms;
        for (int i = 0; i < 3; i++) counts[i] = res[i];
        return STARKHIP_OK;
    }
    int masks(uint64_t* out) override {
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(hipMemcpyAsync(out, d_masks(), 2 * W * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(stream_wait(c));
        c->mset.ms[3] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return STARKHIP_OK;
    }
};
}  // namespace

int check_trace_permutations(Ctx* c, const AirInfo& air, const TraceInput& in, uint64_t seed, uint32_t* per_pair, uint64_t* masks, uint64_t* list,
                             size_t cap, starkhip_perm_check_t* out) {
    const AirProgram& P = air.prog;
    const size_t n = in.n_rows, C = P.n_cols;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const std::vector<uint32_t> cols = perm_columns(P);
    DevicePermSteps steps(c, n);
    std::vector<uint32_t> desc;  // per pair: n_entries, then n_entries x (lhs, rhs) as indices into `cols`
    for (const auto& pr : P.perm_pairs) {
        steps.pair_at.push_back((uint32_t)desc.size());
        desc.push_back((uint32_t)pr.size());
        for (uint64_t e : pr)
            for (uint32_t col : {(uint32_t)e, (uint32_t)(e >> 32)}) desc.push_back((uint32_t)(std::lower_bound(cols.begin(), cols.end(), col) - cols.begin()));
    }
    Ctx::MultisetBufs& mb = c->mset;
    if (!in.callers_columns()) HIPCHK(c->values.ensure(C * n * 8));
    if (in.park_words(C)) HIPCHK(c->lde.ensure(in.park_words(C) * 8));  // the staging of row-major host rows
    HIPCHK(c->perm.cols.ensure(cols.size() * n * 8));
    HIPCHK(mb.desc.ensure(desc.size() * 4));
    if (int rc = sorted_items_reserve(c, 2 * n)) return rc;
    HIPCHK(mb.masks.ensure((2 * steps.W + 3) * 8));
    std::fill(mb.ms, mb.ms + 4, 0.f);
    HIPCHK(hipEventRecord(c->kev[0], st));
    const gl_t* d_values = nullptr;
    if (int rc = upload_dense(c, in, c->values.as<gl_t>(), &d_values)) return rc;
    for (size_t k = 0; k < cols.size(); k++)
        HIPCHK(hipMemcpyAsync(c->perm.cols.as<gl_t>() + k * n, d_values + (size_t)cols[k] * n, n * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(mb.desc.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->kev[1], st));
    HIPCHK(stream_wait(c));  // (`desc` may go out of scope on any return below)
    HIPCHK(hipEventElapsedTime(&mb.ms[0], c->kev[0], c->kev[1]));
    return perm_check_run(P, n, steps, seed, per_pair, masks, list, cap, out);
}

void perm_check_timings(Ctx* c, float ms[4]) { std::copy(c->mset.ms, c->mset.ms + 4, ms); }

}  // namespace starkhip
