// starkhip_check_trace_permutations' host half (permutation_check.h) and its replay without a device.
#include "permutation_check.h"

#include <algorithm>
#include <vector>

#include "check_report.h"

namespace starkhip {

int perm_check_args(const AirInfo* air, const TraceInput& in, uint64_t seed, const uint64_t* list, size_t cap, const void* out) {
    if (!air || air->prog.perm_pairs.empty()) return STARKHIP_ERR_BAD_AIR;
    unsigned log_n = 0;
    if (in.check(*air) || !log2_rows(in.n_rows, &log_n) || log_n > max_log_rows(*air)) return STARKHIP_ERR_BAD_SHAPE;
    if (perm_check_bad_seed(seed) || cap > STARKHIP_CHECK_LIST_MAX || (cap && !list) || !out) return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}

int perm_check_run(const AirProgram& P, size_t n_rows, PermCheckSteps& steps, uint64_t seed, uint32_t* per_pair, uint64_t* masks, uint64_t* list,
                   size_t cap, starkhip_perm_check_t* out) {
    const size_t np = P.perm_pairs.size(), W = (n_rows + 63) / 64;
    starkhip_perm_check_t rep = {np, 0, 0, 0, 0, 0};
    std::vector<uint64_t> pm(2 * W);
    if (masks) std::fill(masks, masks + np * 2 * W, 0);
    for (size_t q = 0; q < np; q++) {
        uint64_t counts[3] = {0, 0, 0};
        gl_t s = seed;
        bool decided = false;
        for (int k = 0; k < STARKHIP_PERM_CHECK_ATTEMPTS && !decided; k++, s = perm_check_next_seed(s)) {
            if (k) rep.reseeds++;
            if (int rc = steps.run(q, s, counts)) return rc;
            decided = counts[0] == 0;
        }
        if (!decided) {
            rep.pairs_undecided++;
            if (per_pair) per_pair[q] = UINT32_MAX;
            continue;
        }
        if (counts[1] != counts[2] || counts[1] > n_rows) return STARKHIP_ERR_HIP;  // both sides have n rows: the surpluses are equal
        if (per_pair) per_pair[q] = (uint32_t)counts[1];
        rep.unmatched += 2 * counts[1];
        if (!counts[1]) continue;
        rep.pairs_violated++;
        if (!masks && rep.listed >= cap) continue;
        if (int rc = steps.masks(pm.data())) return rc;
        for (size_t side = 0; side < 2; side++) {
            const uint64_t lead[2] = {q, side};
            const uint64_t bits = mask_to_list(pm.data() + side * W, W, lead, 2, list, cap, &rep.listed);
            if (bits != counts[1 + side]) return STARKHIP_ERR_HIP;  // the masks are the ones that were counted
        }
        if (masks) std::copy(pm.begin(), pm.end(), masks + q * 2 * W);
    }
    *out = rep;
    return STARKHIP_OK;
}

namespace {
// one pair under one seed as host loops over the row-major trace
struct ReplaySteps : PermCheckSteps {
    const AirProgram& P;
    const uint64_t* rows;  // [n][C]
    size_t n, C, W;
    std::vector<uint64_t> last;
    ReplaySteps(const AirProgram& P_, const uint64_t* rows_, size_t n_) : P(P_), rows(rows_), n(n_), C(P_.n_cols), W((n_ + 63) / 64), last(2 * W) {}
    gl_t cell(const std::vector<uint64_t>& pair, size_t e, uint32_t item) const {
        const uint32_t side = item >= n, row = item - side * (uint32_t)n;
        return gl_from_u64(rows[(size_t)row * C + (uint32_t)(pair[e] >> (32 * side))]);
    }
    int run(size_t q, gl_t seed, uint64_t counts[3]) override {
        const std::vector<uint64_t>& pair = P.perm_pairs[q];
        const size_t items = 2 * n;
        std::vector<gl_t> keys(items);
        std::vector<uint32_t> idx(items);
        for (size_t i = 0; i < items; i++) {
            gl_t key = 0, pw = 1;
            for (size_t e = 0; e < pair.size(); e++) {
                key = gl_add(key, gl_mul(cell(pair, e, (uint32_t)i), pw));
                pw = gl_mul(pw, seed);
            }
            keys[i] = key;
            idx[i] = (uint32_t)i;
        }
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
        std::fill(last.begin(), last.end(), 0);
        counts[0] = counts[1] = counts[2] = 0;
        for (size_t a = 0, b; a < items; a = b) {
            for (b = a + 1; b < items && keys[idx[b]] == keys[idx[a]]; b++)
                for (size_t e = 0; pair.size() > 1 && e < pair.size(); e++)
                    if (cell(pair, e, idx[b]) != cell(pair, e, idx[b - 1])) {
                        counts[0]++;
                        break;
                    }
            size_t m = a;  // the run's first rhs item: the sort kept lhs before rhs, rows ascending
            while (m < b && idx[m] < n) m++;
            const size_t L = m - a, R = b - m;
            for (size_t j = a; j < b; j++) {
                const uint32_t side = idx[j] >= n, row = idx[j] - side * (uint32_t)n;
                const size_t rank = side ? j - m : j - a, other = side ? L : R;
                if (rank < other) continue;
                last[side * W + (row >> 6)] |= 1ull << (row & 63);
                counts[1 + side]++;
            }
        }
        return STARKHIP_OK;
    }
    int masks(uint64_t* out) override {
        std::copy(last.begin(), last.end(), out);
        return STARKHIP_OK;
    }
};
}  // namespace

int check_trace_permutations_replay(const AirInfo& air, const TraceInput& in, uint64_t seed, uint32_t* per_pair, uint64_t* masks, uint64_t* list,
                                    size_t cap, starkhip_perm_check_t* out) {
    std::vector<uint64_t> rows;
    in.to_row_major(rows);
    ReplaySteps steps(air.prog, rows.data(), in.n_rows);
    return perm_check_run(air.prog, in.n_rows, steps, seed, per_pair, masks, list, cap, out);
}

}  // namespace starkhip
