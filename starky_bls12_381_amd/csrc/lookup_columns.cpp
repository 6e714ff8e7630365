// starkhip_lookup_columns' host half (lookup_columns.h) and its replay without a device.
#include "lookup_columns.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "check_report.h"
#include "gl.h"

namespace starkhip {

bool lookup_list_ok(size_t n_cols, const starkhip_lookup_t* lookups, size_t n_lookups, std::string* why) {
    auto refuse = [&](const std::string& m) {
        if (why) *why = m;
        return false;
    };
    if (!lookups || !n_lookups) return refuse("no lookups");
    if (n_lookups > STARKHIP_LOOKUPS_MAX) return refuse(std::to_string(n_lookups) + " lookups (at most " + std::to_string(STARKHIP_LOOKUPS_MAX) + ")");
    for (size_t q = 0; q < n_lookups; q++) {
        const starkhip_lookup_t& a = lookups[q];
        const std::string who = "lookup " + std::to_string(q) + ": ";
        for (uint32_t col : {a.input, a.table, a.permuted_input, a.permuted_table})
            if (col >= n_cols) return refuse(who + "column " + std::to_string(col) + " out of range (" + std::to_string(n_cols) + " columns)");
        if (a.permuted_input == a.permuted_table) return refuse(who + "permuted_input and permuted_table are both column " + std::to_string(a.permuted_input));
        for (size_t r = 0; r < n_lookups; r++) {  // an output column is nobody's input or table, and nobody else's output
            const starkhip_lookup_t& b = lookups[r];
            for (uint32_t o : {a.permuted_input, a.permuted_table}) {
                if (o == b.input || o == b.table)
                    return refuse(who + "output column " + std::to_string(o) + " is the " + (o == b.input ? "input" : "table") + " of lookup " + std::to_string(r));
                if (r != q && (o == b.permuted_input || o == b.permuted_table))
                    return refuse(who + "output column " + std::to_string(o) + " is also an output of lookup " + std::to_string(r));
            }
        }
    }
    return true;
}

bool air_lookups_ok(const AirProgram& P, const starkhip_lookup_t* lookups, size_t n_lookups, std::string* why) {
    if (!lookup_list_ok(P.n_cols, lookups, n_lookups, why)) return false;
    auto declared = [&](uint32_t lhs, uint32_t rhs) {
        const uint64_t e = (uint64_t)lhs | ((uint64_t)rhs << 32);
        for (const auto& pr : P.perm_pairs)
            if (pr.size() == 1 && pr[0] == e) return true;
        return false;
    };
    for (size_t q = 0; q < n_lookups; q++) {
        const starkhip_lookup_t& a = lookups[q];
        for (int t = 0; t < 2; t++) {
            const uint32_t lhs = t ? a.table : a.input, rhs = t ? a.permuted_table : a.permuted_input;
            if (declared(lhs, rhs)) continue;
            if (why)
                *why = "lookup " + std::to_string(q) + ": the program declares no permutation pair [(" + std::to_string(lhs) + ", " + std::to_string(rhs) + ")] (" +
                       (t ? "table, permuted_table" : "input, permuted_input") + "): the fill would write columns the proof does not bind";
            return false;
        }
    }
    return true;
}

int lookup_args(const TraceInput& in, const starkhip_lookup_t* lookups, size_t n_lookups, const uint64_t* list, size_t cap, const void* out) {
    unsigned log_n = 0;
    if (!in.words || in.unknown_layout || !in.n_cols || in.n_cols > UINT32_MAX) return STARKHIP_ERR_BAD_SHAPE;
    if (!log2_rows(in.n_rows, &log_n) || log_n > STARKHIP_MAX_LOG_ROWS) return STARKHIP_ERR_BAD_SHAPE;
    if (cap > STARKHIP_CHECK_LIST_MAX || (cap && !list) || !out) return STARKHIP_ERR_BAD_SHAPE;
    return lookup_list_ok(in.n_cols, lookups, n_lookups, nullptr) ? STARKHIP_OK : STARKHIP_ERR_BAD_SHAPE;
}

int lookup_run(size_t n_rows, const starkhip_lookup_t* lookups, size_t n_lookups, size_t batch, LookupSteps& steps, uint32_t* per_lookup, uint64_t* masks,
               uint64_t* list, size_t cap, starkhip_lookup_report_t* out) {
    const size_t W = (n_rows + 63) / 64;
    starkhip_lookup_report_t rep = {n_lookups, 0, 0, 0};
    std::vector<uint64_t> pm(W), missing(std::max<size_t>(1, batch));
    if (!batch) return STARKHIP_ERR_BAD_SHAPE;
    if (masks) std::fill(masks, masks + n_lookups * W, 0);
    for (size_t q0 = 0; q0 < n_lookups; q0 += batch) {
        const size_t g = std::min(batch, n_lookups - q0);
        std::fill(missing.begin(), missing.end(), 0);
        if (int rc = steps.run(q0, lookups + q0, g, missing.data())) return rc;
        for (size_t i = 0; i < g; i++) {
            const size_t q = q0 + i;
            if (missing[i] > n_rows) return STARKHIP_ERR_HIP;
            if (per_lookup) per_lookup[q] = (uint32_t)missing[i];
            rep.missing_rows += missing[i];
            if (!missing[i]) continue;
            rep.lookups_failed++;
            if (!masks && rep.listed >= cap) continue;
            if (int rc = steps.mask(i, pm.data())) return rc;
            const uint64_t lead = q;
            const uint64_t bits = mask_to_list(pm.data(), W, &lead, 1, list, cap, &rep.listed);
            if (bits != missing[i]) return STARKHIP_ERR_HIP;  // the mask is the one that was counted
            if (masks) std::copy(pm.begin(), pm.end(), masks + q * W);
        }
    }
    *out = rep;
    return STARKHIP_OK;
}

namespace {
// one lookup as host loops over the caller's trace: the rule of lookup_columns.h, literally
struct ReplaySteps : LookupSteps {
    const TraceInput& in;
    uint64_t* words;
    size_t n, W;
    std::vector<uint64_t> batch_masks;  // [g][W] of the last batch
    ReplaySteps(const TraceInput& in_, uint64_t* words_) : in(in_), words(words_), n(in_.n_rows), W((in_.n_rows + 63) / 64) {}
    int run(size_t, const starkhip_lookup_t* lks, size_t g, uint64_t* missing) override {
        batch_masks.assign(g * W, 0);
        for (size_t i = 0; i < g; i++)
            if (int rc = run_one(lks[i], batch_masks.data() + i * W, missing + i)) return rc;
        return STARKHIP_OK;
    }
    int run_one(const starkhip_lookup_t& lk, uint64_t* last, uint64_t* missing) {
        std::vector<gl_t> a(n), A, T(n);
        for (size_t r = 0; r < n; r++) {
            a[r] = gl_from_u64(in.words[in.at(r, lk.input)]);
            T[r] = gl_from_u64(in.words[in.at(r, lk.table)]);
        }
        A = a;
        std::stable_sort(A.begin(), A.end());
        std::stable_sort(T.begin(), T.end());
        *missing = 0;
        for (size_t r = 0; r < n; r++)
            if (!std::binary_search(T.begin(), T.end(), a[r])) {
                last[r >> 6] |= 1ull << (r & 63);
                ++*missing;
            }
        if (*missing) return STARKHIP_OK;
        std::vector<gl_t> unused;  // of T, ascending
        for (size_t j = 0; j < n; j++) {
            const bool used = (j == 0 || T[j] != T[j - 1]) && std::binary_search(A.begin(), A.end(), T[j]);
            if (!used) unused.push_back(T[j]);
        }
        size_t k = 0;
        for (size_t i = 0; i < n; i++) {
            const bool head = i == 0 || A[i] != A[i - 1];
            if (!head && k >= unused.size()) return STARKHIP_ERR_HIP;  // heads and used positions are equally many
            words[in.at(i, lk.permuted_input)] = A[i];
            words[in.at(i, lk.permuted_table)] = head ? A[i] : unused[k++];
        }
        return k == unused.size() ? STARKHIP_OK : STARKHIP_ERR_HIP;
    }
    int mask(size_t i, uint64_t* out) override {
        if ((i + 1) * W > batch_masks.size()) return STARKHIP_ERR_BAD_SHAPE;
        std::copy(batch_masks.begin() + i * W, batch_masks.begin() + (i + 1) * W, out);
        return STARKHIP_OK;
    }
};
}  // namespace

int lookup_columns_replay(const TraceInput& in, uint64_t* words, const starkhip_lookup_t* lookups, size_t n_lookups, uint32_t* per_lookup, uint64_t* masks,
                          uint64_t* list, size_t cap, starkhip_lookup_report_t* out, size_t batch) {
    ReplaySteps steps(in, words);
    return lookup_run(in.n_rows, lookups, n_lookups, lookup_batch_size(in.n_rows, n_lookups, batch), steps, per_lookup, masks, list, cap, out);
}

uint64_t* lookup_blob_make(int air, size_t n_rows, const starkhip_lookup_report_t& rep, const uint64_t* list, size_t* words) {
    const size_t total = LOOKUP_BLOB_HEADER + 2 * (size_t)rep.listed;
    uint64_t* b = (uint64_t*)malloc(total * 8);
    if (!b) return nullptr;
    const uint64_t head[LOOKUP_BLOB_HEADER] = {STARKHIP_LOOKUP_MAGIC, (uint64_t)air, n_rows, rep.lookups, rep.lookups_failed, rep.missing_rows, rep.listed, 0};
    memcpy(b, head, sizeof head);
    if (rep.listed) memcpy(b + LOOKUP_BLOB_HEADER, list, 2 * (size_t)rep.listed * 8);
    *words = total;
    return b;
}

bool lookup_blob_read(const uint64_t* blob, size_t words, starkhip_lookup_report_t* out, const uint64_t** list) {
    if (!blob || words < LOOKUP_BLOB_HEADER || blob[0] != STARKHIP_LOOKUP_MAGIC || blob[7] != 0) return false;
    const uint64_t listed = blob[6];
    if (listed > STARKHIP_CHECK_LIST_MAX || listed > blob[5] || words != LOOKUP_BLOB_HEADER + 2 * (size_t)listed) return false;
    *out = starkhip_lookup_report_t{blob[3], blob[4], blob[5], listed};
    if (list) *list = listed ? blob + LOOKUP_BLOB_HEADER : nullptr;
    return true;
}

int lookup_blob_replay(const AirInfo& air, const TraceInput& in, size_t cap, uint64_t** blob, size_t* words) {
    *blob = nullptr;
    *words = 0;
    if (air.lookups.empty()) return STARKHIP_OK;  // nothing is filled, nothing can be refused
    std::vector<uint64_t> copy(in.words, in.words + in.n_rows * in.n_cols);  // the caller's trace is only read
    TraceInput mine = in;
    mine.words = copy.data();
    std::vector<uint64_t> list(2 * std::max<size_t>(1, cap));
    starkhip_lookup_report_t rep = {0, 0, 0, 0};
    if (int rc = lookup_columns_replay(mine, copy.data(), air.lookups.data(), air.lookups.size(), nullptr, nullptr, list.data(), cap, &rep)) return rc;
    if (!rep.lookups_failed) return STARKHIP_OK;
    *blob = lookup_blob_make(air.id, in.n_rows, rep, list.data(), words);
    return *blob ? STARKHIP_ERR_TRACE : STARKHIP_ERR_OOM;
}

}  // namespace starkhip
