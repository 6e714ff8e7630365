// starkhip_lookup_columns' host half (lookup_columns.h) and its replay without a device.
#include "lookup_columns.h"

#include <algorithm>
#include <vector>

#include "check_report.h"
#include "gl.h"

namespace starkhip {

int lookup_args(const TraceInput& in, const starkhip_lookup_t* lookups, size_t n_lookups, const uint64_t* list, size_t cap, const void* out) {
    unsigned log_n = 0;
    if (!in.words || in.unknown_layout || !in.n_cols || in.n_cols > UINT32_MAX) return STARKHIP_ERR_BAD_SHAPE;
    if (!log2_rows(in.n_rows, &log_n) || log_n > STARKHIP_MAX_LOG_ROWS) return STARKHIP_ERR_BAD_SHAPE;
    if (!lookups || !n_lookups || n_lookups > STARKHIP_LOOKUPS_MAX) return STARKHIP_ERR_BAD_SHAPE;
    if (cap > STARKHIP_CHECK_LIST_MAX || (cap && !list) || !out) return STARKHIP_ERR_BAD_SHAPE;
    for (size_t q = 0; q < n_lookups; q++) {
        const starkhip_lookup_t& a = lookups[q];
        if (a.input >= in.n_cols || a.table >= in.n_cols || a.permuted_input >= in.n_cols || a.permuted_table >= in.n_cols) return STARKHIP_ERR_BAD_SHAPE;
        if (a.permuted_input == a.permuted_table) return STARKHIP_ERR_BAD_SHAPE;
        for (size_t r = 0; r < n_lookups; r++) {  // an output column is nobody's input or table, and nobody else's output
            const starkhip_lookup_t& b = lookups[r];
            for (uint32_t o : {a.permuted_input, a.permuted_table}) {
                if (o == b.input || o == b.table) return STARKHIP_ERR_BAD_SHAPE;
                if (r != q && (o == b.permuted_input || o == b.permuted_table)) return STARKHIP_ERR_BAD_SHAPE;
            }
        }
    }
    return STARKHIP_OK;
}

int lookup_run(size_t n_rows, const starkhip_lookup_t* lookups, size_t n_lookups, LookupSteps& steps, uint32_t* per_lookup, uint64_t* masks,
               uint64_t* list, size_t cap, starkhip_lookup_report_t* out) {
    const size_t W = (n_rows + 63) / 64;
    starkhip_lookup_report_t rep = {n_lookups, 0, 0, 0};
    std::vector<uint64_t> pm(W);
    if (masks) std::fill(masks, masks + n_lookups * W, 0);
    for (size_t q = 0; q < n_lookups; q++) {
        uint64_t missing = 0;
        if (int rc = steps.run(q, lookups[q], &missing)) return rc;
        if (missing > n_rows) return STARKHIP_ERR_HIP;
        if (per_lookup) per_lookup[q] = (uint32_t)missing;
        rep.missing_rows += missing;
        if (!missing) continue;
        rep.lookups_failed++;
        if (!masks && rep.listed >= cap) continue;
        if (int rc = steps.mask(pm.data())) return rc;
        const uint64_t lead = q;
        const uint64_t bits = mask_to_list(pm.data(), W, &lead, 1, list, cap, &rep.listed);
        if (bits != missing) return STARKHIP_ERR_HIP;  // the mask is the one that was counted
        if (masks) std::copy(pm.begin(), pm.end(), masks + q * W);
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
    std::vector<uint64_t> last;
    ReplaySteps(const TraceInput& in_, uint64_t* words_) : in(in_), words(words_), n(in_.n_rows), W((in_.n_rows + 63) / 64), last(W) {}
    int run(size_t, const starkhip_lookup_t& lk, uint64_t* missing) override {
        std::vector<gl_t> a(n), A, T(n);
        for (size_t r = 0; r < n; r++) {
            a[r] = gl_from_u64(in.words[in.at(r, lk.input)]);
            T[r] = gl_from_u64(in.words[in.at(r, lk.table)]);
        }
        A = a;
        std::stable_sort(A.begin(), A.end());
        std::stable_sort(T.begin(), T.end());
        std::fill(last.begin(), last.end(), 0);
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
    int mask(uint64_t* out) override {
        std::copy(last.begin(), last.end(), out);
        return STARKHIP_OK;
    }
};
}  // namespace

int lookup_columns_replay(const TraceInput& in, uint64_t* words, const starkhip_lookup_t* lookups, size_t n_lookups, uint32_t* per_lookup, uint64_t* masks,
                          uint64_t* list, size_t cap, starkhip_lookup_report_t* out) {
    ReplaySteps steps(in, words);
    return lookup_run(in.n_rows, lookups, n_lookups, steps, per_lookup, masks, list, cap, out);
}

}  // namespace starkhip
