// Host half of starkhip_check_trace_free_cell_classes and starkhip_check_trace_free_cells (free_cells.h): the compiled form the
// kernel walks, the summaries, the audit as a projection of the classes, and the one replay without a device behind both.
#include "free_cells.h"

#include <algorithm>

#include "air_validate.h"
#include "check_report.h"

namespace starkhip {

static const uint32_t PIVOT_KEY = REF_COL_MASK | REF_NEXT;

static void add_pivot(std::vector<uint32_t>& pivots, size_t first, uint32_t ref) {
    const uint32_t key = ref & PIVOT_KEY;
    if (std::find(pivots.begin() + first, pivots.end(), key) == pivots.end()) pivots.push_back(key);
}

FreeProgram compile_free_cells(const QProgram& Q) {
    FreeProgram F;
    uint32_t g0 = 0, g1 = 0, t0 = 0, kind = 0;
    const uint32_t n_ops = Q.chunk_batch.back() * QOP_BATCH;  // what follows are guard batches
    for (uint32_t i = 0; i < n_ops; i++) {
        const uint32_t hdr = Q.ops[i].hdr, op = hdr & 7u;
        if (op == QOP_GROUP) {
            g0 = i;
            kind = (hdr >> QOP_KIND_SHIFT) & 3u;
            g1 = i + 1;
            while ((Q.ops[g1].hdr & 7u) == QOP_GATE) g1++;
            t0 = g1;
            i = g1 - 1;
            continue;
        }
        if (op != QOP_TERM || !(hdr & QOP_FOLD)) continue;
        FreeCon c = {g0, g1, t0, i + 1, (uint32_t)F.pivots.size(), 0, kind, 0};
        for (uint32_t j = g0 + 1; j < g1; j++) add_pivot(F.pivots, c.piv0, Q.ops[j].ref);
        for (uint32_t j = t0; j <= i; j++)
            if (!(Q.ops[j].hdr & QOP_NOCELL)) add_pivot(F.pivots, c.piv0, Q.ops[j].ref);
        c.piv1 = (uint32_t)F.pivots.size();
        F.cons.push_back(c);
        t0 = i + 1;
    }
    return F;
}

starkhip_free_cells_t free_cells_summary(const uint32_t* per_column, size_t n_rows, size_t n_cols) {
    starkhip_free_cells_t s = {(uint64_t)n_rows * n_cols, 0, 0, 0};
    for (size_t c = 0; c < n_cols; c++) {
        s.free_cells += per_column[c];
        s.free_columns += per_column[c] == n_rows;
        s.partly_free_columns += per_column[c] != 0 && per_column[c] != n_rows;
    }
    return s;
}

starkhip_free_cell_classes_t free_cell_classes_summary(const uint32_t* per_column, const uint32_t* open_rows, size_t n_rows, size_t n_cols,
                                                       size_t n_constraints) {
    starkhip_free_cell_classes_t s = {(uint64_t)n_rows * n_cols, 0, 0, 0, 0, 0, 0};
    for (size_t c = 0; c < n_cols; c++) {
        s.silent += per_column[3 * c];
        s.gated += per_column[3 * c + 1];
        s.unread += per_column[3 * c + 2];
        s.silent_columns += per_column[3 * c] != 0;
    }
    s.caught = s.cells - s.silent - s.gated - s.unread;
    for (size_t k = 0; k < n_constraints; k++) s.constraints_never_open += open_rows[k] == 0;
    return s;
}

starkhip_free_cells_t free_cells_from_classes(const uint32_t* class_per_column, size_t n_rows, size_t n_cols, uint32_t* per_column, uint64_t* mask) {
    std::vector<uint32_t> per(n_cols);
    for (size_t c = 0; c < n_cols; c++) per[c] = class_per_column[3 * c] + class_per_column[3 * c + 1] + class_per_column[3 * c + 2];
    if (per_column) std::copy(per.begin(), per.end(), per_column);
    const size_t W = (n_rows + 63) / 64;
    const uint64_t all = n_rows >= 64 ? ~0ull : (1ull << n_rows) - 1;  // n_rows is a power of two: below 64 it is one word's low bits
    if (mask)
        for (size_t i = 0; i < n_cols * W; i++) mask[i] = ~mask[i] & all;
    return free_cells_summary(per.data(), n_rows, n_cols);
}

// The one replay: the planes, the per-column counts [C][3] and open_rows [K] of the rule in free_cells.h.
namespace {
struct ClassesReplay {
    std::vector<uint64_t> bits;  // [3][C][W]: read, open, caught
    std::vector<uint32_t> per, open;
};
}  // namespace

static int free_cell_classes_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, ClassesReplay* R) {
    unsigned log_n = 0;
    if (int rc = check_trace_shape(air, in.n_rows, pis, &log_n)) return rc;
    if (free_cells_bad_delta(delta)) return STARKHIP_ERR_BAD_SHAPE;
    const AirProgram& P = air.prog;
    const size_t n = in.n_rows, C = P.n_cols, W = (n + 63) / 64;
    std::vector<uint64_t> rows;  // row-major, and ours to change: a cell is raised in place, evaluated and put back
    in.to_row_major(rows);
    std::vector<uint64_t>& bits = R->bits;
    bits.assign(3 * C * W, 0);
    uint64_t *rd_p = bits.data(), *op_p = rd_p + C * W, *ca_p = op_p + C * W;
    std::vector<uint32_t>& open = R->open;
    open.assign(P.n_constraints, 0);
    AirReader rd(P);
    GroupWord grp;
    std::vector<uint32_t> pivots;
    size_t k = 0;
    for (size_t g = 0; rd.group(&grp); g++) {
        const uint32_t group_word = P.group_off[g];
        std::vector<uint32_t> gates(grp.n_gates);
        for (uint32_t& ref : gates) ref = rd.ref();
        for (uint32_t j = 0; j < grp.m; j++, k++) {
            const uint32_t term_word = (uint32_t)(rd.w - P.code.data());
            pivots.clear();
            for (uint32_t ref : gates) add_pivot(pivots, 0, ref);
            TermWord tw;
            do {
                tw = rd.term();
                for (uint32_t f = 0; f < tw.nf; f++) add_pivot(pivots, 0, rd.ref());
            } while (!tw.last);
            gl_t G, body;
            for (size_t r = 0; r < n; r++) {  // the unchanged trace: the frames this constraint's gates are open on
                if (!constraint_applies<size_t>(grp.kind, r, n)) continue;
                air_constraint_parts_at(P, group_word, term_word, &rows[r * C], &rows[(r + 1) % n * C], pis, &G, &body);
                open[k] += G != 0;
            }
            for (uint32_t piv : pivots) {
                const size_t col = piv & REF_COL_MASK;
                for (size_t r = 0; r < n; r++) {
                    const size_t frame = (piv & REF_NEXT) ? (r + n - 1) % n : r;
                    if (!constraint_applies<size_t>(grp.kind, frame, n)) continue;
                    uint64_t& cell = rows[r * C + col];
                    const uint64_t kept = cell;
                    cell = gl_add(gl_from_u64(kept), delta);  // the cell is any word of its class mod p
                    air_constraint_parts_at(P, group_word, term_word, &rows[frame * C], &rows[(frame + 1) % n * C], pis, &G, &body);
                    cell = kept;
                    const size_t at = col * W + (r >> 6);
                    const uint64_t bit = 1ull << (r & 63);
                    rd_p[at] |= bit;
                    if (G != 0) op_p[at] |= bit;
                    if (gl_mul(G, body) != 0) ca_p[at] |= bit;
                }
            }
        }
    }
    std::vector<uint32_t>& per = R->per;
    per.assign(3 * C, 0);
    for (size_t c = 0; c < C; c++) {
        uint32_t silent = 0, gated = 0, unread = 0;
        for (size_t w = 0; w < W; w++) {
            const uint64_t all = n - w * 64 >= 64 ? ~0ull : (1ull << (n - w * 64)) - 1;
            const uint64_t r_w = rd_p[c * W + w], o_w = op_p[c * W + w], c_w = ca_p[c * W + w];
            silent += (uint32_t)__builtin_popcountll(o_w & ~c_w);
            gated += (uint32_t)__builtin_popcountll(r_w & ~o_w);
            unread += (uint32_t)__builtin_popcountll(~r_w & all);
        }
        per[3 * c] = silent;
        per[3 * c + 1] = gated;
        per[3 * c + 2] = unread;
    }
    return STARKHIP_OK;
}

int check_trace_free_cell_classes_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                                         uint64_t* planes, uint32_t* open_rows, starkhip_free_cell_classes_t* out) {
    ClassesReplay R;
    if (int rc = free_cell_classes_replay(air, in, pis, delta, &R)) return rc;
    if (per_column) std::copy(R.per.begin(), R.per.end(), per_column);
    if (planes) std::copy(R.bits.begin(), R.bits.end(), planes);
    if (open_rows) std::copy(R.open.begin(), R.open.end(), open_rows);
    *out = free_cell_classes_summary(R.per.data(), R.open.data(), in.n_rows, air.prog.n_cols, air.prog.n_constraints);
    return STARKHIP_OK;
}

int check_trace_free_cells_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                                  uint64_t* free_mask, starkhip_free_cells_t* out) {
    ClassesReplay R;
    if (int rc = free_cell_classes_replay(air, in, pis, delta, &R)) return rc;
    if (free_mask) std::copy(R.bits.begin() + 2 * (R.bits.size() / 3), R.bits.end(), free_mask);  // the caught plane
    *out = free_cells_from_classes(R.per.data(), in.n_rows, air.prog.n_cols, per_column, free_mask);
    return STARKHIP_OK;
}

}  // namespace starkhip
