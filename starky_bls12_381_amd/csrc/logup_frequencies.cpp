// starkhip_logup_frequencies' host half (logup_frequencies.h) and its replay without a device.
#include "logup_frequencies.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "check_report.h"
#include "gl.h"
#include "logup.h"

namespace starkhip {

bool logup_fillable(const AirProgram& P, std::string* why) {
    auto refuse = [&](const std::string& m) {
        if (why) *why = m;
        return false;
    };
    for (size_t q = 0; q < P.logups.size(); q++) {
        const std::string who = "LogUp lookup " + std::to_string(q) + ": ";
        if (!P.logups[q].freq.plain()) return refuse(who + "its frequencies are a combination, not one plain column");
        const uint32_t f = P.logups[q].freq.col();
        for (size_t r = 0; r < P.logups.size(); r++) {
            const AirProgram::Logup& b = P.logups[r];
            if (r != q && b.freq.plain() && f == b.freq.col()) return refuse(who + "frequencies column " + std::to_string(f) + " is also the frequencies column of lookup " + std::to_string(r));
            bool read = false;
            auto see = [&](uint32_t col) { read |= col == f; };
            b.table.each_column(see);
            if (read) return refuse(who + "frequencies column " + std::to_string(f) + " is read by the table column of lookup " + std::to_string(r));
            for (const AirProgram::Column& v : b.cols) v.each_column(see);
            for (const AirProgram::Filter& fl : b.filters)
                for (const AirProgram::Column& c : fl.cols) c.each_column(see);
            if (read) return refuse(who + "frequencies column " + std::to_string(f) + " is read by a looked-up column or a filter of lookup " + std::to_string(r));
        }
    }
    return true;
}

LogupFreqPlan::LogupFreqPlan(const AirProgram& P) : L(P.logups.size()), prog(&P) {
    col_off.push_back(0);
    general = false;
    for (const AirProgram::Logup& l : P.logups) general |= !l.plain();
    size_t words = 0;
    auto column_words = [](const AirProgram::Column& c) { return 3 + 3 * c.terms.size(); };
    for (size_t q = 0; q < L; q++) {
        const AirProgram::Logup& l = P.logups[q];
        col_off.push_back(col_off.back() + (uint32_t)l.cols.size());
        freq.push_back(l.freq.col());  // (a fillable program: plain)
        size_t first = q;
        for (size_t r = 0; r < q && first == q; r++)
            if (P.logups[r].table == l.table) first = r;
        table_of.push_back((uint32_t)first);
        if (!general) {
            for (const AirProgram::Column& v : l.cols) cols.push_back(v.col());
            table.push_back(l.table.col());
        }
        l.table.each_column([&](uint32_t c) { named.push_back(c); });
        words += column_words(l.table);
        for (size_t k = 0; k < l.cols.size(); k++) {
            l.cols[k].each_column([&](uint32_t c) { named.push_back(c); });
            words += column_words(l.cols[k]) + 1;
            for (const AirProgram::Column& c : l.filters[k].cols) {
                c.each_column([&](uint32_t x) { named.push_back(x); });
                words += column_words(c);
            }
        }
    }
    desc_words = 3 * (L + n_values()) + (general ? words : 0);
    std::sort(named.begin(), named.end());
    named.erase(std::unique(named.begin(), named.end()), named.end());
}

int logup_freq_args(const AirInfo& air, const TraceInput& in, const uint64_t* list, size_t cap, const void* out) {
    unsigned log_n = 0;
    if (in.check(air) || !log2_rows(in.n_rows, &log_n) || log_n > STARKHIP_MAX_LOG_ROWS) return STARKHIP_ERR_BAD_SHAPE;
    if (cap > STARKHIP_CHECK_LIST_MAX || (cap && !list) || !out) return STARKHIP_ERR_BAD_SHAPE;
    return logup_fillable(air.prog, nullptr) ? STARKHIP_OK : STARKHIP_ERR_BAD_SHAPE;
}

int logup_freq_run(size_t n_rows, const LogupFreqPlan& plan, size_t batch, LogupFreqSteps& steps, uint32_t* per_lookup, uint32_t* per_column, uint64_t* masks,
                   uint64_t* list, size_t cap, starkhip_logup_report_t* out) {
    const size_t W = (n_rows + 63) / 64, L = plan.L;
    starkhip_logup_report_t rep = {L, 0, 0, 0, 0};
    if (!batch) return STARKHIP_ERR_BAD_SHAPE;
    std::vector<uint64_t> pm(W);
    std::vector<uint32_t> col_missing;
    if (masks) std::fill(masks, masks + L * W, 0);
    for (size_t q0 = 0; q0 < L; q0 += batch) {
        const size_t g = std::min(batch, L - q0), c0 = plan.col_off[q0];
        col_missing.assign(plan.col_off[q0 + g] - c0, 0);
        if (int rc = steps.run(q0, g, col_missing.data())) return rc;
        if (per_column) std::copy(col_missing.begin(), col_missing.end(), per_column + c0);
        for (size_t i = 0; i < g; i++) {
            const size_t q = q0 + i;
            uint64_t cells = 0;
            for (size_t k = plan.col_off[q]; k < plan.col_off[q + 1]; k++) {
                if (col_missing[k - c0] > n_rows) return STARKHIP_ERR_HIP;
                cells += col_missing[k - c0];
            }
            if (per_lookup) per_lookup[q] = (uint32_t)cells;
            if (!cells) continue;
            rep.lookups_failed++;
            rep.missing_cells += cells;
            if (int rc = steps.mask(i, pm.data())) return rc;
            const uint64_t lead = q;
            const uint64_t rows = mask_to_list(pm.data(), W, &lead, 1, list, cap, &rep.listed);
            if (!rows || rows > cells || rows > n_rows) return STARKHIP_ERR_HIP;  // the mask is the one that was counted
            rep.missing_rows += rows;
            if (masks) std::copy(pm.begin(), pm.end(), masks + q * W);
        }
    }
    *out = rep;
    return STARKHIP_OK;
}

namespace {
// one lookup as host loops over the caller's trace: the rule of logup_frequencies.h, literally
struct ReplayFreqSteps : LogupFreqSteps {
    const LogupFreqPlan& plan;
    const TraceInput& in;
    uint64_t* words;
    size_t n, W;
    std::vector<uint64_t> batch_masks;  // [g][W] of the last batch
    ReplayFreqSteps(const LogupFreqPlan& plan_, const TraceInput& in_, uint64_t* words_)
        : plan(plan_), in(in_), words(words_), n(in_.n_rows), W((in_.n_rows + 63) / 64) {}
    int run(size_t q0, size_t g, uint32_t* col_missing) override {
        batch_masks.assign(g * W, 0);
        for (size_t i = 0; i < g; i++) run_one(q0 + i, batch_masks.data() + i * W, col_missing + (plan.col_off[q0 + i] - plan.col_off[q0]));
        return STARKHIP_OK;
    }
    void run_one(size_t q, uint64_t* mask, uint32_t* col_missing) {
        const AirProgram::Logup& lk = plan.prog->logups[q];
        auto cell = [&](uint32_t col, size_t r) { return in.words[in.at(r, col)]; };
        std::vector<gl_t> t(n);
        for (size_t r = 0; r < n; r++) t[r] = logup_column_at(lk.table, cell, r, n);
        std::vector<uint32_t> order(n);  // the rows by (value, row): the first of a run of equal values is a FIRST
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return t[a] < t[b]; });
        std::vector<gl_t> sorted(n);
        for (size_t j = 0; j < n; j++) sorted[j] = t[order[j]];
        std::vector<uint32_t> count(n, 0);
        bool any = false;
        for (size_t k = 0; k < plan.m(q); k++) {
            for (size_t r = 0; r < n; r++) {
                const gl_t phi = logup_filter_at(lk.filters[k], cell, r, n);
                if (phi == 0) continue;  // skipped
                const gl_t v = logup_column_at(lk.cols[k], cell, r, n);
                const size_t pos = (size_t)(std::lower_bound(sorted.begin(), sorted.end(), v) - sorted.begin());
                if (phi == 1 && pos < n && sorted[pos] == v) count[pos]++;
                else {  // missing, or flagged
                    mask[r >> 6] |= 1ull << (r & 63);
                    col_missing[k]++;
                    any = true;
                }
            }
        }
        if (any) return;
        for (size_t j = 0; j < n; j++) words[in.at(order[j], plan.freq[q])] = count[j];
    }
    int mask(size_t i, uint64_t* out) override {
        if ((i + 1) * W > batch_masks.size()) return STARKHIP_ERR_BAD_SHAPE;
        std::copy(batch_masks.begin() + i * W, batch_masks.begin() + (i + 1) * W, out);
        return STARKHIP_OK;
    }
};
}  // namespace

int logup_frequencies_replay(const AirInfo& air, const TraceInput& in, uint64_t* words, uint32_t* per_lookup, uint32_t* per_column, uint64_t* masks, uint64_t* list,
                             size_t cap, starkhip_logup_report_t* out) {
    const LogupFreqPlan plan(air.prog);
    ReplayFreqSteps steps(plan, in, words);
    return logup_freq_run(in.n_rows, plan, logup_freq_batch_size(in.n_rows, plan.L), steps, per_lookup, per_column, masks, list, cap, out);
}

uint64_t* logup_blob_make(int air, size_t n_rows, const starkhip_logup_report_t& rep, const uint64_t* list, size_t* words) {
    const size_t total = LOGUP_BLOB_HEADER + 2 * (size_t)rep.listed;
    uint64_t* b = (uint64_t*)malloc(total * 8);
    if (!b) return nullptr;
    const uint64_t head[LOGUP_BLOB_HEADER] = {STARKHIP_LOGUP_MAGIC, (uint64_t)air, n_rows, rep.lookups, rep.lookups_failed, rep.missing_rows, rep.listed, rep.missing_cells};
    memcpy(b, head, sizeof head);
    if (rep.listed) memcpy(b + LOGUP_BLOB_HEADER, list, 2 * (size_t)rep.listed * 8);
    *words = total;
    return b;
}

bool logup_blob_read(const uint64_t* blob, size_t words, starkhip_logup_report_t* out, const uint64_t** list) {
    if (!blob || words < LOGUP_BLOB_HEADER || blob[0] != STARKHIP_LOGUP_MAGIC) return false;
    const uint64_t listed = blob[6];
    if (listed > STARKHIP_CHECK_LIST_MAX || listed > blob[5] || blob[5] > blob[7] || words != LOGUP_BLOB_HEADER + 2 * (size_t)listed) return false;
    *out = starkhip_logup_report_t{blob[3], blob[4], blob[7], blob[5], listed};
    if (list) *list = listed ? blob + LOGUP_BLOB_HEADER : nullptr;
    return true;
}

int logup_blob_replay(const AirInfo& air, const TraceInput& in, size_t cap, uint64_t** blob, size_t* words) {
    *blob = nullptr;
    *words = 0;
    std::vector<uint64_t> copy(in.words, in.words + in.n_rows * in.n_cols);  // the caller's trace is only read
    TraceInput mine = in;
    mine.words = copy.data();
    std::vector<uint64_t> list(2 * std::max<size_t>(1, cap));
    starkhip_logup_report_t rep = {0, 0, 0, 0, 0};
    if (int rc = logup_frequencies_replay(air, mine, copy.data(), nullptr, nullptr, nullptr, list.data(), cap, &rep)) return rc;
    if (!rep.lookups_failed) return STARKHIP_OK;
    *blob = logup_blob_make(air.id, in.n_rows, rep, list.data(), words);
    return *blob ? STARKHIP_ERR_TRACE : STARKHIP_ERR_OOM;
}

}  // namespace starkhip
