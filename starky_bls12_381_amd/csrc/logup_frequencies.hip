// starkhip_logup_frequencies and the fill of prove() ("fill_frequencies") on the context's device: the LogUp lookups of an AIR in
// batches of G consecutive lookups (logup_freq_batch_size).  Per batch: the keys of its distinct table columns and their stable sort
// (kernels_multiset.hip, in the sorted-items buffers of the context, n items per table), then count and write of
// kernels_logup_freq.hip with grid.y = looked-up column and grid.y = lookup, under the host half of logup_frequencies.h.  A program with
// a lookup over Columns or Filters runs the general keys and count kernels over a descriptor of them; a plain one the kernels it always ran.  A device
// trace is read and written where it lies, in either layout (element r of column c at stride 1 or n_cols); of a host trace the
// distinct columns the fill reads go up in one copy and, for a lookup that holds, its frequencies column comes back.
// The write follows the count on the stream without a wait in between.  In the caller's trace it is gated on the device by the
// lookup's own missing count: a failed lookup writes nothing.  In prove() the trace is the prover's own copy, the write is not gated,
// and a failed lookup ends the proof.  Either way the host waits once per batch, for its missing counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ctx.h"
#include "kernels_logup_freq.h"
#include "kernels_multiset.h"
#include "logup.h"
#include "logup_frequencies.h"

namespace starkhip {

namespace {
struct DeviceFreqSteps : LogupFreqSteps {
    Ctx* c;
    const LogupFreqPlan& plan;
    const TraceInput& in;
    uint64_t* words;  // the trace `in` views, writable
    bool own;         // the trace is the prover's own copy: the write is not gated
    size_t n, W, K, last_g = 0;
    bool ev0 = false;            // kev[0] of the coming batch is on the stream already (prepare)
    std::vector<uint64_t> host;  // a host trace: [K + L][n] as Ctx::LogupFreqBufs::cols
    std::vector<uint32_t> desc;
    DeviceFreqSteps(Ctx* c_, const LogupFreqPlan& plan_, const TraceInput& in_, uint64_t* words_, bool own_)
        : c(c_), plan(plan_), in(in_), words(words_), own(own_), n(in_.n_rows), W((in_.n_rows + 63) / 64), K(plan_.named.size()) {}
    unsigned long long* d_mask() const { return c->logup_freq.mask.as<unsigned long long>(); }  // a batch of g: [g][W], then its uint32 counters
    // a column of the trace as the kernels number it: itself, or its slot in the staging of a host trace
    uint32_t tr(uint32_t col) const {
        return in.on_device ? col : (uint32_t)(std::lower_bound(plan.named.begin(), plan.named.end(), col) - plan.named.begin());
    }
    LogupFreqTrace view() const {
        if (!in.on_device) return {c->logup_freq.cols.as<gl_t>(), n, 1};
        return in.form == TraceForm::ColMajor ? LogupFreqTrace{words, n, 1} : LogupFreqTrace{words, 1, in.n_cols};
    }
    // a host trace: the columns the fill reads, staged and sent up in one copy
    int prepare() {
        HIPCHK(hipEventRecord(c->kev[0], c->st));
        ev0 = true;
        if (in.on_device) return STARKHIP_OK;
        host.resize((K + plan.L) * n);
        for (size_t k = 0; k < K; k++)
            for (size_t r = 0; r < n; r++) host[k * n + r] = in.words[in.at(r, plan.named[k])];
        HIPCHK(hipMemcpyAsync(c->logup_freq.cols.p, host.data(), K * n * 8, hipMemcpyHostToDevice, c->st));
        return STARKHIP_OK;
    }
    int run(size_t q0, size_t g, uint32_t* col_missing) override {
        if (!g || q0 + g > plan.L || g > logup_freq_batch_size(n, plan.L)) return STARKHIP_ERR_BAD_SHAPE;
        hipStream_t st = c->st;
        Ctx::LogupFreqBufs& lf = c->logup_freq;
        const size_t nc = plan.col_off[q0 + g] - plan.col_off[q0];
        last_g = g;
        if (!ev0) HIPCHK(hipEventRecord(c->kev[0], st));
        ev0 = false;
        // the batch's descriptors: its distinct tables in order of first use, its lookups, its looked-up columns
        std::vector<uint32_t> tabs, slot_of(g);  // (a table is named by the first lookup that has it)
        for (size_t i = 0; i < g; i++) {
            const uint32_t t = plan.table_of[q0 + i];
            const size_t s = (size_t)(std::find(tabs.begin(), tabs.end(), t) - tabs.begin());
            if (s == tabs.size()) tabs.push_back(t);
            slot_of[i] = (uint32_t)s;
        }
        const size_t S = tabs.size();
        desc.clear();
        if (!plan.general) {
            for (uint32_t t : tabs) desc.push_back(tr(plan.table[t]));
            for (size_t i = 0; i < g; i++) desc.insert(desc.end(), {slot_of[i], in.on_device ? plan.freq[q0 + i] : (uint32_t)(K + q0 + i)});
            for (size_t i = 0; i < g; i++)
                for (size_t k = plan.col_off[q0 + i]; k < plan.col_off[q0 + i + 1]; k++) desc.insert(desc.end(), {tr(plan.cols[k]), (uint32_t)i, slot_of[i]});
        } else {  // the same three tables with places in the descriptor for columns, then the Columns and Filters themselves
            desc.resize(S + 2 * g + 3 * nc);
            auto ref = [&](uint32_t col) { return tr(col); };
            for (size_t s = 0; s < S; s++) {
                desc[s] = (uint32_t)desc.size();
                logup_desc_push_column(desc, plan.prog->logups[tabs[s]].table, ref);
            }
            size_t e = S + 2 * g;
            for (size_t i = 0; i < g; i++) {
                const AirProgram::Logup& lk = plan.prog->logups[q0 + i];
                desc[S + 2 * i] = slot_of[i];
                desc[S + 2 * i + 1] = in.on_device ? plan.freq[q0 + i] : (uint32_t)(K + q0 + i);
                for (size_t k = 0; k < lk.cols.size(); k++, e += 3) {
                    desc[e] = (uint32_t)desc.size();
                    desc[e + 1] = (uint32_t)i;
                    desc[e + 2] = slot_of[i];
                    logup_desc_push_column(desc, lk.cols[k], ref);
                    logup_desc_push_filter(desc, lk.filters[k], ref);
                }
            }
            if (desc.size() > plan.desc_words) return STARKHIP_ERR_BAD_SHAPE;
        }
        const uint32_t* d_tabs = lf.desc.as<uint32_t>();
        const uint32_t *d_lks = d_tabs + S, *d_cols = d_lks + 2 * g;
        HIPCHK(hipMemcpyAsync(lf.desc.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, st));
        uint32_t* count = lf.count.as<uint32_t>();
        uint32_t* missing = (uint32_t*)(d_mask() + g * W);  // [g] by lookup, then [nc] by looked-up column
        HIPCHK(hipMemsetAsync(count, 0, g * n * 4, st));
        HIPCHK(hipMemsetAsync(d_mask(), 0, g * W * 8 + (g + nc) * 4, st));
        HIPCHK(hipEventRecord(c->kev[1], st));
        const LogupFreqTrace t = view();
        gl_t* keys = c->mset.keys.as<gl_t>();
        uint32_t *idx = c->mset.idx.as<uint32_t>(), *table = c->mset.table.as<uint32_t>();
        if (plan.general) HIPCHK(launch_logup_freq_keys_general(t, n, d_tabs, d_tabs, S, keys, idx, st));
        else HIPCHK(launch_logup_freq_keys(t, n, d_tabs, S, keys, idx, st));
        HIPCHK(launch_multiset_sort_batch(keys, idx, keys + S * n, idx + S * n, n, S, table, table + S * multiset_table_words(n), st));
        HIPCHK(hipEventRecord(c->kev[2], st));
        if (plan.general) HIPCHK(launch_logup_freq_count_general(t, n, d_tabs, d_cols, nc, g, keys, count, d_mask(), missing, c->opt_logup_count_combine != 0, st));
        else HIPCHK(launch_logup_freq_count(t, n, d_cols, nc, g, keys, count, d_mask(), missing, c->opt_logup_count_combine != 0, st));
        HIPCHK(hipEventRecord(c->kev[3], st));
        HIPCHK(launch_logup_freq_write(t, n, d_lks, g, idx, count, own ? nullptr : missing, st));
        HIPCHK(hipEventRecord(c->kev[4], st));
        std::vector<uint32_t> res(g + nc, 0);
        HIPCHK(read_back(c, res.data(), missing, res.size() * 4, st));
        HIPCHK(stream_wait(c));  // the one wait of the batch for its counts
        for (int i = 0; i < 4; i++) {  // upload, keys and sort, count, write
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, c->kev[i], c->kev[i + 1]));
            lf.ms[i] += ms;
        }
        std::copy(res.begin() + g, res.end(), col_missing);
        if (in.on_device) return STARKHIP_OK;
        const auto t1 = std::chrono::steady_clock::now();
        bool any = false;
        for (size_t i = 0; i < g; i++) {
            if (res[i]) continue;
            HIPCHK(hipMemcpyAsync(host.data() + (K + q0 + i) * n, lf.cols.as<gl_t>() + (K + q0 + i) * n, n * 8, hipMemcpyDeviceToHost, st));
            any = true;
        }
        if (any) HIPCHK(stream_wait(c));
        for (size_t i = 0; i < g; i++) {
            if (res[i]) continue;
            for (size_t r = 0; r < n; r++) words[in.at(r, plan.freq[q0 + i])] = host[(K + q0 + i) * n + r];
        }
        lf.ms[4] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
        return STARKHIP_OK;
    }
    int mask(size_t i, uint64_t* out) override {
        if (i >= last_g) return STARKHIP_ERR_BAD_SHAPE;
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(hipMemcpyAsync(out, d_mask() + i * W, W * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(stream_wait(c));
        c->logup_freq.ms[4] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return STARKHIP_OK;
    }
};

std::vector<LookupWant> freq_work_buffers(Ctx* c, const LogupFreqPlan& plan, size_t n, bool staged) {
    const size_t G = logup_freq_batch_size(n, plan.L), W = (n + 63) / 64;
    Ctx::LogupFreqBufs& lf = c->logup_freq;
    return {{&c->mset.keys, 2 * G * n * 8},
            {&c->mset.idx, 2 * G * n * 4},
            {&c->mset.table, G * (multiset_table_words(n) + multiset_scan_chunks(n)) * 4},
            {&lf.desc, plan.desc_words * 4},
            {&lf.cols, staged ? (plan.named.size() + plan.L) * n * 8 : 0},
            {&lf.count, G * n * 4},
            {&lf.mask, G * W * 8 + (plan.L + plan.n_values()) * 4}};
}

int freq_run(Ctx* c, const LogupFreqPlan& plan, const TraceInput& in, uint64_t* words, bool own, uint32_t* per_lookup, uint32_t* per_column, uint64_t* masks,
             uint64_t* list, size_t cap, starkhip_logup_report_t* out) {
    // Inside a proof (`own`) nothing is allocated here: the buffers are work_buffers()' (prover.hip), grown before the first phase, so
    // that a warmed context never allocates between two phases; one that is missing is an error, not a reason to grow it now.
    for (const LookupWant& w : freq_work_buffers(c, plan, in.n_rows, !in.on_device)) {
        if (!own) HIPCHK(w.b->ensure(w.bytes));
        else if (w.b->cap < w.bytes) return STARKHIP_ERR_HIP;
    }
    std::fill(c->logup_freq.ms, c->logup_freq.ms + 5, 0.f);
    DeviceFreqSteps steps(c, plan, in, words, own);
    if (int rc = steps.prepare()) return rc;
    return logup_freq_run(in.n_rows, plan, logup_freq_batch_size(in.n_rows, plan.L), steps, per_lookup, per_column, masks, list, cap, out);
}
}  // namespace

std::vector<LookupWant> logup_freq_work_buffers(Ctx* c, const AirProgram& P, size_t n_rows, bool staged) {
    return freq_work_buffers(c, LogupFreqPlan(P), n_rows, staged);
}

int logup_frequencies(Ctx* c, const AirInfo& air, const TraceInput& in, uint64_t* words, uint32_t* per_lookup, uint32_t* per_column, uint64_t* masks, uint64_t* list,
                      size_t cap, starkhip_logup_report_t* out) {
    HIPCHK(hipSetDevice(c->device));
    const LogupFreqPlan plan(air.prog);
    return freq_run(c, plan, in, words, false, per_lookup, per_column, masks, list, cap, out);
}

int logup_fill_in_prove(Ctx* c, const AirInfo& air, gl_t* d_trace, size_t n_rows, uint64_t** blob, size_t* words) {
    const LogupFreqPlan plan(air.prog);
    const TraceInput in = TraceInput::dense(d_trace, n_rows, air.prog.n_cols, 1, 1);
    const size_t cap = (size_t)c->opt_check_trace_list;
    std::vector<uint64_t> list(2 * std::max<size_t>(1, cap));
    starkhip_logup_report_t rep = {0, 0, 0, 0, 0};
    if (int rc = freq_run(c, plan, in, d_trace, true, nullptr, nullptr, nullptr, list.data(), cap, &rep)) return rc;
    if (!rep.lookups_failed) return STARKHIP_OK;
    c->traces_checked++;
    c->traces_rejected++;
    *blob = logup_blob_make(air.id, n_rows, rep, list.data(), words);
    return *blob ? STARKHIP_ERR_TRACE : STARKHIP_ERR_OOM;
}

void logup_frequency_timings(Ctx* c, float ms[5]) { std::copy(c->logup_freq.ms, c->logup_freq.ms + 5, ms); }

}  // namespace starkhip
