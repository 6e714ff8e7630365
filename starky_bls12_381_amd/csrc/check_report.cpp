// starkhip_check_trace_report's host half (check_report.h) and its replay without a device.
#include "check_report.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "air_validate.h"

namespace starkhip {

int check_trace_shape(const AirInfo& air, size_t n_rows, const uint64_t* pis, unsigned* log_n_out) {
    unsigned log_n = 0;
    if (!log2_rows(n_rows, &log_n) || log_n > max_log_rows(air)) return STARKHIP_ERR_BAD_SHAPE;
    for (size_t i = 0; i < air.prog.n_pis; i++)
        if (pis[i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    *log_n_out = log_n;
    return STARKHIP_OK;
}

int check_report_run(const AirProgram& P, size_t n_rows, CheckPasses& passes, uint32_t* per_constraint, uint64_t* row_mask, uint64_t* list,
                     size_t cap, starkhip_check_report_t* out) {
    const size_t K = P.n_constraints, W = (n_rows + 63) / 64;
    std::vector<uint32_t> counts(K, 0);
    std::vector<uint64_t> mask(W, 0);
    if (int rc = passes.count(counts.data(), mask.data())) return rc;
    starkhip_check_report_t rep = {0, 0, 0, 0};
    for (uint32_t c : counts) {
        rep.violations += c;
        rep.constraints_violated += c != 0;
    }
    for (uint64_t w : mask) rep.rows_violated += (uint64_t)__builtin_popcountll(w);
    rep.listed = std::min<uint64_t>(cap, rep.violations);
    if (per_constraint) std::copy(counts.begin(), counts.end(), per_constraint);
    if (row_mask) std::copy(mask.begin(), mask.end(), row_mask);
    *out = rep;
    if (!rep.listed) return STARKHIP_OK;
    // the listed constraints: the violated ones, in order, while what precedes them leaves room under `cap`.  The last one's rows may
    // reach past it -- by fewer than n_rows entries -- and are cut after the sort.
    std::vector<uint32_t> base(K, ~0u);
    size_t total = 0;
    for (size_t k = 0; k < K && total < cap; k++)
        if (counts[k]) {
            base[k] = (uint32_t)total;
            total += counts[k];
        }
    struct Entry { uint64_t k, row, value; };
    std::vector<Entry> entries(total);
    if (int rc = passes.list(base.data(), mask.data(), total, &entries[0].k)) return rc;
    // the passes fill a constraint's segment in any order: by row, the list is the same on every run
    for (size_t k = 0; k < K; k++) {
        if (base[k] == ~0u) continue;
        Entry* seg = entries.data() + base[k];
        for (uint32_t i = 0; i < counts[k]; i++)
            if (seg[i].k != k || seg[i].row >= n_rows) return STARKHIP_ERR_HIP;  // the second pass did not find what the first counted
        std::sort(seg, seg + counts[k], [](const Entry& a, const Entry& b) { return a.row < b.row; });
    }
    std::copy(&entries[0].k, &entries[0].k + 3 * rep.listed, list);
    return STARKHIP_OK;
}

namespace {
// the two passes as host loops over air_constraint_value
struct ReplayPasses : CheckPasses {
    const AirProgram& P;
    const uint64_t *rows, *pis;  // row-major [n][C]
    size_t n;
    std::vector<uint8_t> kind;  // per constraint
    ReplayPasses(const AirProgram& P_, const uint64_t* rows_, size_t n_, const uint64_t* pis_) : P(P_), rows(rows_), pis(pis_), n(n_), kind(P_.n_constraints) {
        for (size_t g = 0; g < P.group_off.size(); g++) {
            const uint32_t end = g + 1 < P.group_k0.size() ? P.group_k0[g + 1] : P.n_constraints;
            for (uint32_t k = P.group_k0[g]; k < end; k++) kind[k] = (uint8_t)GroupWord::decode(P.code[P.group_off[g]]).kind;
        }
    }
    bool applies(uint32_t k, size_t r) const {
        return constraint_applies(kind[k], r, n);
    }
    gl_t value(uint32_t k, size_t r) const { return air_constraint_value(P, k, rows + r * P.n_cols, rows + ((r + 1) % n) * P.n_cols, pis); }
    int count(uint32_t* counts, uint64_t* mask) override {
        for (size_t r = 0; r < n; r++)
            for (uint32_t k = 0; k < P.n_constraints; k++)
                if (applies(k, r) && value(k, r) != 0) {
                    counts[k]++;
                    mask[r >> 6] |= 1ull << (r & 63);
                }
        return STARKHIP_OK;
    }
    int list(const uint32_t* base, const uint64_t*, size_t total, uint64_t* entries) override {
        std::vector<uint32_t> cursor(P.n_constraints, 0);
        for (size_t i = 0; i < n; i++) {
            const size_t r = (i * 0x9E3779B1u + 5) & (n - 1);  // n is a power of two, the multiplier odd: every row once, scrambled
            for (uint32_t k = 0; k < P.n_constraints; k++) {
                if (base[k] == ~0u || !applies(k, r)) continue;
                const gl_t v = value(k, r);
                if (v == 0) continue;
                const size_t slot = (size_t)base[k] + cursor[k]++;
                if (slot >= total) return STARKHIP_ERR_HIP;
                entries[3 * slot] = k;
                entries[3 * slot + 1] = r;
                entries[3 * slot + 2] = v;
            }
        }
        return STARKHIP_OK;
    }
};
}  // namespace

int check_trace_report_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint32_t* per_constraint, uint64_t* row_mask,
                              uint64_t* list, size_t cap, starkhip_check_report_t* out) {
    unsigned log_n = 0;
    if (int rc = check_trace_shape(air, in.n_rows, pis, &log_n)) return rc;
    const AirProgram& P = air.prog;
    std::vector<uint64_t> rows;
    in.to_row_major(rows);
    ReplayPasses passes(P, rows.data(), in.n_rows, pis);
    return check_report_run(P, in.n_rows, passes, per_constraint, row_mask, list, cap, out);
}

uint64_t* check_blob_make(int air, size_t n_rows, const starkhip_check_report_t& rep, const uint64_t* list, size_t* words) {
    const size_t total = CHECK_BLOB_HEADER + 3 * (size_t)rep.listed;
    uint64_t* b = (uint64_t*)malloc(total * 8);
    if (!b) return nullptr;
    const uint64_t head[CHECK_BLOB_HEADER] = {STARKHIP_CHECK_MAGIC, (uint64_t)air, n_rows, rep.violations, rep.constraints_violated, rep.rows_violated, rep.listed, 0};
    memcpy(b, head, sizeof head);
    if (rep.listed) memcpy(b + CHECK_BLOB_HEADER, list, 3 * (size_t)rep.listed * 8);
    *words = total;
    return b;
}

bool check_blob_read(const uint64_t* blob, size_t words, starkhip_check_report_t* out, const uint64_t** list) {
    if (!blob || words < CHECK_BLOB_HEADER || blob[0] != STARKHIP_CHECK_MAGIC || blob[7] != 0) return false;
    const uint64_t listed = blob[6];
    if (listed > STARKHIP_CHECK_LIST_MAX || listed > blob[3] || words != CHECK_BLOB_HEADER + 3 * (size_t)listed) return false;
    *out = starkhip_check_report_t{blob[3], blob[4], blob[5], listed};
    if (list) *list = listed ? blob + CHECK_BLOB_HEADER : nullptr;
    return true;
}

int check_blob_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, size_t cap, uint64_t** blob, size_t* words) {
    *blob = nullptr;
    *words = 0;
    std::vector<uint64_t> list(3 * std::max<size_t>(1, cap));
    starkhip_check_report_t rep = {0, 0, 0, 0};
    if (int rc = check_trace_report_replay(air, in, pis, nullptr, nullptr, list.data(), cap, &rep)) return rc;
    if (!rep.violations) return STARKHIP_OK;
    *blob = check_blob_make(air.id, in.n_rows, rep, list.data(), words);
    return *blob ? STARKHIP_ERR_TRACE : STARKHIP_ERR_OOM;
}

}  // namespace starkhip
