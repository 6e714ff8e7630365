// starkhip_lookup_columns and the fill of prove() ("fill_lookups") on the context's device: the lookups of a trace in batches of G
// (lookup_batch_size), each batch as its sorted items (sorted_items_run, ctx.hip: keys and the stable sort of kernels_multiset.hip, one
// set per lookup) and the steps of kernels_lookup.hip over them -- mark, the scan of the tile counts, the two placements -- one set of
// launches with grid.y = lookup, under the host half of lookup_columns.h.  A column-major device trace is read and written where it
// lies; a row-major one is read through a gather of the batch's columns and written in place with stride n_cols; of a host trace the
// batch's staged columns go up in one copy and, for a lookup that holds, its two output columns come back.
// The placements follow mark and scan on the stream without a wait in between.  In the caller's trace they are gated on the device by
// the lookup's own missing count: a failed lookup writes nothing.  In prove() the trace is the prover's own copy, the placements are
// not gated, and a failed lookup ends the proof.  Either way the host waits once per batch, for its missing counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ctx.h"
#include "kernels_lookup.h"
#include "kernels_multiset.h"
#include "lookup_columns.h"

namespace starkhip {

namespace {
// Ctx::LookupBufs::desc for L lookups in batches of at most G, 32-bit words:
//   keys_trace  [L][3]  {1, input, table}: a lookup's items as columns of the trace (a batch's descriptors lie back to back)
//   keys_staged [G][3]  {1, 4 g, 4 g + 1}: ... as columns of the staging [G][4][n]
//   out_trace   [L][2]  {permuted_input, permuted_table}
//   out_staged  [G][2]  {4 g + 2, 4 g + 3}
struct LookupDesc {
    size_t L, G;
    size_t keys_trace(size_t q) const { return 3 * q; }
    size_t keys_staged() const { return 3 * L; }
    size_t out_trace(size_t q) const { return 3 * (L + G) + 2 * q; }
    size_t out_staged() const { return 3 * (L + G) + 2 * L; }
    size_t words() const { return 5 * (L + G); }
    std::vector<uint32_t> build(const starkhip_lookup_t* lookups) const {
        std::vector<uint32_t> d;
        for (size_t q = 0; q < L; q++) d.insert(d.end(), {1u, lookups[q].input, lookups[q].table});
        for (uint32_t g = 0; g < G; g++) d.insert(d.end(), {1u, 4 * g, 4 * g + 1});
        for (size_t q = 0; q < L; q++) d.insert(d.end(), {lookups[q].permuted_input, lookups[q].permuted_table});
        for (uint32_t g = 0; g < G; g++) d.insert(d.end(), {4 * g + 2, 4 * g + 3});
        return d;
    }
};

struct DeviceLookupSteps : LookupSteps {
    Ctx* c;
    const TraceInput& in;
    uint64_t* words;  // the trace `in` views, writable
    LookupDesc D;
    bool own;         // the trace is the prover's own copy: the placements are not gated
    size_t n, W, last_g = 0;
    std::vector<uint64_t> host;  // a host trace: [G][4][n] as Ctx::LookupBufs::cols
    DeviceLookupSteps(Ctx* c_, const TraceInput& in_, uint64_t* words_, LookupDesc D_, bool own_)
        : c(c_), in(in_), words(words_), D(D_), own(own_), n(in_.n_rows), W((in_.n_rows + 63) / 64), host(in_.on_device ? 0 : D_.G * 4 * in_.n_rows) {}
    unsigned long long* d_mask() const { return c->lookup.mask.as<unsigned long long>(); }  // a batch of g: [g][W], then the g missing counts
    int run(size_t q0, const starkhip_lookup_t* lks, size_t g, uint64_t* missing) override {
        if (!g || g > D.G || q0 + g > D.L) return STARKHIP_ERR_BAD_SHAPE;
        hipStream_t st = c->st;
        Ctx::LookupBufs& lb = c->lookup;
        const size_t C = in.n_cols;
        const bool in_place = in.callers_columns();
        const gl_t* keys = nullptr;
        const uint32_t* idx = nullptr;
        gl_t* staged = lb.cols.as<gl_t>();
        const uint32_t* desc = lb.desc.as<uint32_t>();
        uint8_t* flags = lb.flags.as<uint8_t>();
        uint32_t* sums = lb.sums.as<uint32_t>();
        uint32_t* slot = lb.slot.as<uint32_t>();
        unsigned long long* counts = d_mask() + g * W;
        last_g = g;
        HIPCHK(hipEventRecord(c->kev[0], st));
        if (!in.on_device) {
            for (size_t i = 0; i < g; i++) {
                const uint32_t col[4] = {lks[i].input, lks[i].table, lks[i].permuted_input, lks[i].permuted_table};
                for (size_t k = 0; k < 4; k++)
                    for (size_t r = 0; r < n; r++) host[(4 * i + k) * n + r] = in.words[in.at(r, col[k])];
            }
            HIPCHK(hipMemcpyAsync(staged, host.data(), g * 4 * n * 8, hipMemcpyHostToDevice, st));
        } else if (!in_place) HIPCHK(launch_lookup_gather(in.words, C, n, desc + D.keys_trace(q0), g, staged, st));
        HIPCHK(hipMemsetAsync(d_mask(), 0, g * (W + 1) * 8, st));
        HIPCHK(hipMemsetAsync(slot, 0xFF, g * n * 4, st));
        HIPCHK(hipEventRecord(c->kev[1], st));
        if (int rc = sorted_items_run(c, desc + (in_place ? D.keys_trace(q0) : D.keys_staged()), in_place ? in.words : staged, n, n, 0, &keys, &idx, g, 3)) return rc;
        HIPCHK(hipEventRecord(c->kev[2], st));
        HIPCHK(launch_lookup_mark(keys, idx, n, g, flags, sums, d_mask(), counts, st));
        HIPCHK(launch_lookup_scan(sums, n, g, st));
        // where element r of column col lies
        LookupOut out = {staged, n, 1};
        const uint32_t* out_cols = desc + D.out_staged();
        if (in.on_device) {
            out = in_place ? LookupOut{words, n, 1} : LookupOut{words, 1, C};
            out_cols = desc + D.out_trace(q0);
        }
        HIPCHK(launch_lookup_place(keys, flags, sums, n, g, out, out_cols, own ? nullptr : counts, slot, st));
        HIPCHK(hipEventRecord(c->kev[3], st));
        std::vector<unsigned long long> res(g, 0);
        HIPCHK(read_back(c, res.data(), counts, g * sizeof(unsigned long long), st));
        HIPCHK(stream_wait(c));  // the one wait of the batch for its counts
        for (int i = 0; i < 3; i++) {  // upload or gather, keys and sort, mark and scan and placements
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, c->kev[i], c->kev[i + 1]));
            lb.ms[i] += ms;
        }
        std::copy(res.begin(), res.end(), missing);
        if (in.on_device) return STARKHIP_OK;
        const auto t1 = std::chrono::steady_clock::now();
        bool any = false;
        for (size_t i = 0; i < g; i++) {
            if (res[i]) continue;
            HIPCHK(hipMemcpyAsync(host.data() + (4 * i + 2) * n, staged + (4 * i + 2) * n, 2 * n * 8, hipMemcpyDeviceToHost, st));
            any = true;
        }
        if (any) HIPCHK(stream_wait(c));
        for (size_t i = 0; i < g; i++) {
            if (res[i]) continue;
            for (size_t r = 0; r < n; r++) {
                words[in.at(r, lks[i].permuted_input)] = host[(4 * i + 2) * n + r];
                words[in.at(r, lks[i].permuted_table)] = host[(4 * i + 3) * n + r];
            }
        }
        lb.ms[3] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
        return STARKHIP_OK;
    }
    int mask(size_t i, uint64_t* out) override {
        if (i >= last_g) return STARKHIP_ERR_BAD_SHAPE;
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(hipMemcpyAsync(out, d_mask() + i * W, W * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(stream_wait(c));
        c->lookup.ms[3] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return STARKHIP_OK;
    }
};
}  // namespace

std::vector<LookupWant> lookup_work_buffers(Ctx* c, size_t n_rows, size_t n_lookups, bool staged) {
    const size_t G = lookup_batch_size(n_rows, n_lookups, (size_t)c->opt_lookup_batch), items = 2 * n_rows, W = (n_rows + 63) / 64;
    Ctx::LookupBufs& lb = c->lookup;
    return {{&c->mset.keys, 2 * G * items * 8},
            {&c->mset.idx, 2 * G * items * 4},
            {&c->mset.table, G * (multiset_table_words(items) + multiset_scan_chunks(items)) * 4},
            {&lb.desc, LookupDesc{n_lookups, G}.words() * 4},
            {&lb.cols, staged ? G * 4 * n_rows * 8 : 0},
            {&lb.flags, G * items},
            {&lb.sums, G * lookup_sum_words(items) * 4},
            {&lb.slot, G * n_rows * 4},
            {&lb.mask, G * (W + 1) * 8}};
}

// room for the batches of a fill and the descriptors of `lookups` on the device; *D says where they lie
static int lookup_prepare(Ctx* c, size_t n, bool staged, const starkhip_lookup_t* lookups, size_t n_lookups, int desc_air, LookupDesc* D) {
    Ctx::LookupBufs& lb = c->lookup;
    *D = LookupDesc{n_lookups, lookup_batch_size(n, n_lookups, (size_t)c->opt_lookup_batch)};
    const void* desc_was = lb.desc.p;
    for (const LookupWant& w : lookup_work_buffers(c, n, n_lookups, staged)) HIPCHK(w.b->ensure(w.bytes));
    std::fill(lb.ms, lb.ms + 4, 0.f);
    if (desc_air >= 0 && lb.desc_air == desc_air && lb.desc_G == D->G && lb.desc.p == desc_was) return STARKHIP_OK;  // a registered AIR's list never changes
    lb.desc_air = -1;
    const std::vector<uint32_t> desc = D->build(lookups);
    HIPCHK(hipMemcpyAsync(lb.desc.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(stream_wait(c));  // (`desc` goes out of scope)
    lb.desc_air = desc_air;
    lb.desc_G = D->G;
    return STARKHIP_OK;
}

int lookup_columns(Ctx* c, const TraceInput& in, uint64_t* words, const starkhip_lookup_t* lookups, size_t n_lookups, uint32_t* per_lookup,
                   uint64_t* masks, uint64_t* list, size_t cap, starkhip_lookup_report_t* out) {
    HIPCHK(hipSetDevice(c->device));
    LookupDesc D;
    if (int rc = lookup_prepare(c, in.n_rows, !in.callers_columns(), lookups, n_lookups, -1, &D)) return rc;
    DeviceLookupSteps steps(c, in, words, D, false);
    return lookup_run(in.n_rows, lookups, n_lookups, D.G, steps, per_lookup, masks, list, cap, out);
}

int lookup_fill_in_prove(Ctx* c, const AirInfo& air, gl_t* d_trace, size_t n_rows, uint64_t** blob, size_t* words) {
    const std::vector<starkhip_lookup_t>& lks = air.lookups;
    const TraceInput in = TraceInput::dense(d_trace, n_rows, air.prog.n_cols, 1, 1);
    LookupDesc D;
    if (int rc = lookup_prepare(c, n_rows, false, lks.data(), lks.size(), air.id, &D)) return rc;
    DeviceLookupSteps steps(c, in, d_trace, D, true);
    const size_t cap = (size_t)c->opt_check_trace_list;
    std::vector<uint64_t> list(2 * std::max<size_t>(1, cap));
    starkhip_lookup_report_t rep = {0, 0, 0, 0};
    if (int rc = lookup_run(n_rows, lks.data(), lks.size(), D.G, steps, nullptr, nullptr, list.data(), cap, &rep)) return rc;
    if (!rep.lookups_failed) return STARKHIP_OK;
    c->traces_checked++;
    c->traces_rejected++;
    *blob = lookup_blob_make(air.id, n_rows, rep, list.data(), words);
    return *blob ? STARKHIP_ERR_TRACE : STARKHIP_ERR_OOM;
}

void lookup_timings(Ctx* c, float ms[4]) { std::copy(c->lookup.ms, c->lookup.ms + 4, ms); }

}  // namespace starkhip
