// starkhip_lookup_columns on the context's device: one lookup as its sorted items (sorted_items_run, ctx.hip: keys and the stable sort of
// kernels_multiset.hip) and the steps of kernels_lookup.hip over them -- mark, the scan of the tile counts, the two placements -- under
// the host half of lookup_columns.h.  A
// column-major device trace is read and written where it lies; a row-major one is read through a gather of the two columns and written
// in place with stride n_cols; of a host trace the two columns go up and, for a lookup that holds, the two output columns come back.
// The placements are launched only after the lookup's missing count has come back as zero: a failed lookup writes nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ctx.h"
#include "kernels_lookup.h"
#include "lookup_columns.h"

namespace starkhip {

namespace {
struct DeviceLookupSteps : LookupSteps {
    Ctx* c;
    const TraceInput& in;
    uint64_t* words;  // the trace `in` views, writable
    size_t n, W, n_lookups = 0;
    std::vector<uint64_t> host;  // a host trace: [4][n] as Ctx::LookupBufs::cols
    DeviceLookupSteps(Ctx* c_, const TraceInput& in_, uint64_t* words_)
        : c(c_), in(in_), words(words_), n(in_.n_rows), W((in_.n_rows + 63) / 64), host(in_.on_device ? 0 : 4 * in_.n_rows) {}
    unsigned long long* d_mask() const { return c->lookup.mask.as<unsigned long long>(); }  // [W], then the missing count
    int run(size_t q, const starkhip_lookup_t& lk, uint64_t* missing) override {
        hipStream_t st = c->st;
        Ctx::LookupBufs& lb = c->lookup;
        const size_t items = 2 * n, C = in.n_cols;
        const bool in_place = in.callers_columns();
        const gl_t* keys = nullptr;
        const uint32_t* idx = nullptr;
        gl_t* staged = lb.cols.as<gl_t>();
        uint8_t* flags = lb.flags.as<uint8_t>();
        uint32_t* sums = lb.sums.as<uint32_t>();
        uint32_t* slot = lb.slot.as<uint32_t>();
        HIPCHK(hipEventRecord(c->kev[0], st));
        if (!in.on_device) {
            for (size_t r = 0; r < n; r++) {
                host[r] = in.words[in.at(r, lk.input)];
                host[n + r] = in.words[in.at(r, lk.table)];
            }
            HIPCHK(hipMemcpyAsync(staged, host.data(), items * 8, hipMemcpyHostToDevice, st));
        } else if (!in_place) HIPCHK(launch_lookup_gather(in.words, C, n, lk.input, lk.table, staged, st));
        HIPCHK(hipMemsetAsync(d_mask(), 0, (W + 1) * 8, st));
        HIPCHK(hipMemsetAsync(slot, 0xFF, n * 4, st));
        HIPCHK(hipEventRecord(c->kev[1], st));
        const uint32_t* desc = lb.desc.as<uint32_t>() + 3 * (in_place ? q : (size_t)n_lookups);
        if (int rc = sorted_items_run(c, desc, in_place ? in.words : staged, n, n, 0, &keys, &idx)) return rc;
        HIPCHK(hipEventRecord(c->kev[2], st));
        HIPCHK(launch_lookup_mark(keys, idx, n, flags, sums, d_mask(), d_mask() + W, st));
        HIPCHK(launch_lookup_scan(sums, n, st));
        HIPCHK(hipEventRecord(c->kev[3], st));
        unsigned long long res = 0;
        HIPCHK(read_back(c, &res, d_mask() + W, sizeof res, st));
        HIPCHK(stream_wait(c));
        for (int i = 0; i < 3; i++) {  // upload or gather, keys and sort, mark and scan
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, c->kev[i], c->kev[i + 1]));
            lb.ms[i] += ms;
        }
        *missing = res;
        if (res) return STARKHIP_OK;
        // where element r of each output column lies
        gl_t *pi = staged + 2 * n, *pt = staged + 3 * n;
        size_t stride = 1;
        if (in_place) pi = words + (size_t)lk.permuted_input * n, pt = words + (size_t)lk.permuted_table * n;
        else if (in.on_device) pi = words + lk.permuted_input, pt = words + lk.permuted_table, stride = C;
        HIPCHK(hipEventRecord(c->kev[4], st));
        HIPCHK(launch_lookup_place_inputs(keys, flags, sums, n, pi, pt, stride, slot, st));
        HIPCHK(launch_lookup_place_table(keys, flags, sums, n, pt, stride, slot, st));
        HIPCHK(hipEventRecord(c->kev[5], st));
        const auto t1 = std::chrono::steady_clock::now();
        if (!in.on_device) HIPCHK(hipMemcpyAsync(host.data() + 2 * n, pi, items * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(stream_wait(c));
        if (!in.on_device) {
            for (size_t r = 0; r < n; r++) {
                words[in.at(r, lk.permuted_input)] = host[2 * n + r];
                words[in.at(r, lk.permuted_table)] = host[3 * n + r];
            }
            lb.ms[3] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
        }
        float place_ms = 0;
        HIPCHK(hipEventElapsedTime(&place_ms, c->kev[4], c->kev[5]));
        lb.ms[2] += place_ms;
        return STARKHIP_OK;
    }
    int mask(uint64_t* out) override {
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(hipMemcpyAsync(out, d_mask(), W * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(stream_wait(c));
        c->lookup.ms[3] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return STARKHIP_OK;
    }
};
}  // namespace

int lookup_columns(Ctx* c, const TraceInput& in, uint64_t* words, const starkhip_lookup_t* lookups, size_t n_lookups, uint32_t* per_lookup,
                   uint64_t* masks, uint64_t* list, size_t cap, starkhip_lookup_report_t* out) {
    const size_t n = in.n_rows, items = 2 * n;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->st;
    DeviceLookupSteps steps(c, in, words);
    steps.n_lookups = n_lookups;
    std::vector<uint32_t> desc;  // per lookup: one entry (input, table) as columns of the trace; last: the same over the staged columns
    for (size_t q = 0; q < n_lookups; q++) desc.insert(desc.end(), {1u, lookups[q].input, lookups[q].table});
    desc.insert(desc.end(), {1u, 0u, 1u});
    Ctx::LookupBufs& lb = c->lookup;
    if (int rc = sorted_items_reserve(c, items)) return rc;
    HIPCHK(lb.desc.ensure(desc.size() * 4));
    if (!in.callers_columns()) HIPCHK(lb.cols.ensure(4 * n * 8));
    HIPCHK(lb.flags.ensure(items));
    HIPCHK(lb.sums.ensure(lookup_sum_words(items) * 4));
    HIPCHK(lb.slot.ensure(n * 4));
    HIPCHK(lb.mask.ensure((steps.W + 1) * 8));
    std::fill(lb.ms, lb.ms + 4, 0.f);
    HIPCHK(hipMemcpyAsync(lb.desc.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(stream_wait(c));  // (`desc` may go out of scope on any return below)
    return lookup_run(n, lookups, n_lookups, steps, per_lookup, masks, list, cap, out);
}

void lookup_timings(Ctx* c, float ms[4]) { std::copy(c->lookup.ms, c->lookup.ms + 4, ms); }

}  // namespace starkhip
