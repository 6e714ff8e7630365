// extern "C" surface of libstarkhip.so (declared in include/starkhip.h).
#include <dirent.h>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <new>

#include "air_eval.h"
#include "air_validate.h"
#include "airs.h"
#include "blob_arena.h"
#include "check_report.h"
#include "free_cells.h"
#include "kernels.h"
#include "lde_ranges.h"
#include "lookup_columns.h"
#include "logup_frequencies.h"
#include "logup.h"
#include "permutation.h"
#include "permutation_check.h"
#include "trace_log.h"

#include <atomic>
#include "poseidon.h"
#include "prover.h"
#include "proof.h"
#include "quotient_plan.h"
#include "verifier.h"

using namespace starkhip;

namespace starkhip {
TraceLog*& armed_trace_log() {
    static thread_local TraceLog* armed = nullptr;
    return armed;
}
static std::atomic<int> g_trace_threads(1);
static thread_local int tl_trace_threads = 0;  // a pool's generator thread sets its own share (pool.cpp)
int trace_threads() { return tl_trace_threads > 0 ? tl_trace_threads : g_trace_threads.load(); }
void set_thread_trace_threads(int n) { tl_trace_threads = n < 0 ? 0 : n > 64 ? 64 : n; }
}  // namespace starkhip

// a call below the C ABI from an entry that reads a trace: what it throws becomes a status
template <class F>
static int guarded(F call) {
    try {
        return call();
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    } catch (const std::exception&) {
        return STARKHIP_ERR_BAD_SHAPE;
    }
}

extern "C" {

void starkhip_config_standard_fast(starkhip_config_t* cfg) {
    // starky StarkConfig::standard_fast_config(): security 100, 2 challenges, FRI rate_bits 1, cap_height 4,
    // proof_of_work_bits 16, ConstantArityBits(4, 5), 84 query rounds
    cfg->security_bits = 100;
    cfg->num_challenges = 2;
    cfg->rate_bits = 1;
    cfg->cap_height = 4;
    cfg->proof_of_work_bits = 16;
    cfg->arity_bits = 4;
    cfg->final_poly_bits = 5;
    cfg->num_query_rounds = 84;
}

int starkhip_config_for_air(starkhip_air_t air, starkhip_config_t* cfg) {
    starkhip_config_standard_fast(cfg);
    switch (air) {
        case STARKHIP_AIR_PAIRING_PRECOMP:  // src/aggregate_proof.rs:32-33
        case STARKHIP_AIR_ECC_AGGREGATE:    // src/aggregate_proof.rs:186-187
        case STARKHIP_AIR_FINAL_EXP:        // src/aggregate_proof.rs:155-156
            cfg->rate_bits = 2;
            return STARKHIP_OK;
        case STARKHIP_AIR_MILLER_LOOP:  // :76
        case STARKHIP_AIR_FP12_MUL:     // :122
        case STARKHIP_AIR_TEST_FIBONACCI:
            return STARKHIP_OK;
        default:
            break;
    }
    const AirInfo* a = (int)air >= STARKHIP_AIR_CUSTOM_BASE ? air_get(air) : nullptr;
    if (!a) return STARKHIP_ERR_BAD_AIR;
    // a registered AIR: the quotient's degree factor degree - 1 must fit the blow-up (starkhip_prove's rule)
    while ((1u << cfg->rate_bits) + 1 < a->degree) cfg->rate_bits++;
    return STARKHIP_OK;
}

int starkhip_air_columns(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (int)a->cols : STARKHIP_ERR_BAD_AIR; }
int starkhip_air_public_inputs(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (int)a->pis : STARKHIP_ERR_BAD_AIR; }
int starkhip_air_constraint_degree(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (int)a->degree : STARKHIP_ERR_BAD_AIR; }
int starkhip_air_num_constraints(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (int)a->prog.n_constraints : STARKHIP_ERR_BAD_AIR; }
int starkhip_air_default_rows(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (int)a->default_rows : STARKHIP_ERR_BAD_AIR; }
int starkhip_air_program(starkhip_air_t air, const uint64_t** blob, size_t* words) {
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    *blob = a->blob.data();
    *words = a->blob.size();
    return STARKHIP_OK;
}

int starkhip_air_eval_frame(starkhip_air_t air, const uint64_t* local, const uint64_t* next, const uint64_t* public_inputs,
                            const uint64_t masks[8], const uint64_t* alphas, int n_alpha, uint64_t* acc_out) {
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    if (!local || !next || !masks || !alphas || !acc_out || n_alpha < 1 || (a->pis && !public_inputs)) return STARKHIP_ERR_BAD_SHAPE;
    try {
        std::vector<gl2_t> l(a->cols), n(a->cols), al(n_alpha), acc(n_alpha);
        for (size_t i = 0; i < a->cols; i++) {
            l[i] = gl2_make(local[2 * i], local[2 * i + 1]);
            n[i] = gl2_make(next[2 * i], next[2 * i + 1]);
        }
        gl2_t mk[4];
        for (int i = 0; i < 4; i++) mk[i] = gl2_make(masks[2 * i], masks[2 * i + 1]);
        for (int j = 0; j < n_alpha; j++) al[j] = gl2_make(alphas[2 * j], alphas[2 * j + 1]);
        air_eval_folded<ExtOps>(a->prog, l.data(), n.data(), public_inputs, mk, al.data(), n_alpha, acc.data());
        for (int j = 0; j < n_alpha; j++) {
            acc_out[2 * j] = acc[j].a0;
            acc_out[2 * j + 1] = acc[j].a1;
        }
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
    return STARKHIP_OK;
}

int starkhip_air_permutation_pairs(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (int)a->prog.perm_pairs.size() : STARKHIP_ERR_BAD_AIR; }
int starkhip_air_permutation_zs(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (int)a->prog.perm_zs() : STARKHIP_ERR_BAD_AIR; }

int starkhip_air_eval_frame_full(starkhip_air_t air, const uint64_t* local, const uint64_t* next, const uint64_t* public_inputs,
                                 const uint64_t masks[8], const uint64_t* alphas, int n_alpha, const uint64_t* zs, const uint64_t* zs_next,
                                 const uint64_t* challenges, uint64_t* acc_out) {
    const int rc = starkhip_air_eval_frame(air, local, next, public_inputs, masks, alphas, n_alpha, acc_out);
    if (rc != STARKHIP_OK) return rc;
    const AirInfo* a = air_get(air);
    const size_t nZ = a->prog.perm_zs();
    if (!nZ) return STARKHIP_OK;
    if (!zs || !zs_next || !challenges) return STARKHIP_ERR_BAD_SHAPE;
    for (size_t i = 0; i < (size_t)a->prog.perm_batch_size() * 4; i++)
        if (challenges[i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    try {
        std::vector<gl2_t> l(a->cols), z(nZ), zn(nZ), al(n_alpha), acc(n_alpha);
        for (size_t i = 0; i < a->cols; i++) l[i] = gl2_make(local[2 * i], local[2 * i + 1]);
        for (size_t i = 0; i < nZ; i++) {
            z[i] = ExtOps::canon(gl2_make(zs[2 * i], zs[2 * i + 1]));
            zn[i] = ExtOps::canon(gl2_make(zs_next[2 * i], zs_next[2 * i + 1]));
        }
        gl2_t mk[4];
        for (int i = 0; i < 4; i++) mk[i] = gl2_make(masks[2 * i], masks[2 * i + 1]);
        for (int j = 0; j < n_alpha; j++) {
            al[j] = gl2_make(alphas[2 * j], alphas[2 * j + 1]);
            acc[j] = gl2_make(acc_out[2 * j], acc_out[2 * j + 1]);
        }
        perm_eval_folded<ExtOps>(a->prog, l.data(), z.data(), zn.data(), challenges, mk, al.data(), n_alpha, acc.data());
        for (int j = 0; j < n_alpha; j++) {
            acc_out[2 * j] = acc[j].a0;
            acc_out[2 * j + 1] = acc[j].a1;
        }
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
    return STARKHIP_OK;
}

int starkhip_air_logups(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (int)a->prog.logups.size() : STARKHIP_ERR_BAD_AIR; }
int starkhip_air_logup_columns(starkhip_air_t air) {
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    size_t m = 0;
    for (const AirProgram::Logup& l : a->prog.logups) m += l.cols.size();
    return (int)m;
}
int starkhip_air_logup_general(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (a->prog.logup_general() ? 1 : 0) : STARKHIP_ERR_BAD_AIR; }
int starkhip_air_logup_polys(starkhip_air_t air) { const AirInfo* a = air_get(air); return a ? (int)a->prog.logup_polys() : STARKHIP_ERR_BAD_AIR; }

int starkhip_air_eval_frame_logup(starkhip_air_t air, const uint64_t* local, const uint64_t* next, const uint64_t* public_inputs,
                                  const uint64_t masks[8], const uint64_t* alphas, int n_alpha, const uint64_t* aux, const uint64_t* aux_next,
                                  const uint64_t* challenges, uint64_t* acc_out) {
    const int rc = starkhip_air_eval_frame(air, local, next, public_inputs, masks, alphas, n_alpha, acc_out);
    if (rc != STARKHIP_OK) return rc;
    const AirInfo* a = air_get(air);
    const size_t nA = a->prog.logup_polys();
    if (!nA) return STARKHIP_OK;
    if (!aux || !aux_next || !challenges || challenges[0] >= GL_P || challenges[1] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    try {
        std::vector<gl2_t> l(a->cols), nx(a->cols), x(nA), xn(nA), al(n_alpha), acc(n_alpha);
        for (size_t i = 0; i < a->cols; i++) {
            l[i] = gl2_make(local[2 * i], local[2 * i + 1]);
            nx[i] = gl2_make(next[2 * i], next[2 * i + 1]);
        }
        for (size_t i = 0; i < nA; i++) {
            x[i] = ExtOps::canon(gl2_make(aux[2 * i], aux[2 * i + 1]));
            xn[i] = ExtOps::canon(gl2_make(aux_next[2 * i], aux_next[2 * i + 1]));
        }
        gl2_t mk[4];
        for (int i = 0; i < 4; i++) mk[i] = gl2_make(masks[2 * i], masks[2 * i + 1]);
        for (int j = 0; j < n_alpha; j++) {
            al[j] = gl2_make(alphas[2 * j], alphas[2 * j + 1]);
            acc[j] = gl2_make(acc_out[2 * j], acc_out[2 * j + 1]);
        }
        logup_eval_folded<ExtOps>(a->prog, l.data(), nx.data(), x.data(), xn.data(), challenges, mk, al.data(), n_alpha, acc.data());
        for (int j = 0; j < n_alpha; j++) {
            acc_out[2 * j] = acc[j].a0;
            acc_out[2 * j + 1] = acc[j].a1;
        }
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
    return STARKHIP_OK;
}

// what the two LogUp entries refuse: as the two Z entries below, for an AIR without LogUp lookups and the two challenges
static int logup_polys_args(const AirInfo* a, const TraceInput& in, const uint64_t* challenges, const uint64_t* polys_out, const uint64_t* closing_out,
                            const uint64_t* zero_denominators_out) {
    if (!a || a->prog.logups.empty()) return STARKHIP_ERR_BAD_AIR;
    if (in.check(*a) || !challenges || !polys_out || !closing_out || !zero_denominators_out || in.n_rows < 2 ||
        in.n_rows > ((size_t)1 << STARKHIP_MAX_LOG_ROWS) || (in.n_rows & (in.n_rows - 1)) || challenges[0] >= GL_P || challenges[1] >= GL_P)
        return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}

int starkhip_logup_polys(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                         const uint64_t* challenges, uint64_t* polys_out, uint64_t* closing_out, uint64_t* zero_denominators_out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (int rc = logup_polys_args(a, in, challenges, polys_out, closing_out, zero_denominators_out)) return rc;
    return guarded([&] { return logup_polys((Ctx*)ctx, *a, in, challenges, polys_out, closing_out, zero_denominators_out); });
}

int starkhip_logup_polys_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, const uint64_t* challenges,
                                uint64_t* polys_out, uint64_t* closing_out, uint64_t* zero_denominators_out) {
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = logup_polys_args(a, in, challenges, polys_out, closing_out, zero_denominators_out)) return rc;
    return guarded([&] {
        const bool col_major = in.form == TraceForm::ColMajor;
        logup_polys_host(a->prog, n_rows, [&](uint32_t col, size_t row) { return col_major ? trace[(size_t)col * n_rows + row] : trace[row * n_cols + col]; }, challenges,
                         polys_out, closing_out, zero_denominators_out);
        return (int)STARKHIP_OK;
    });
}

// what the two Z entries refuse: an AIR that is unknown or has no pairs (BAD_AIR); a trace argument that cannot be one of it, rows that
// are no power of two in 2 .. 2^STARKHIP_MAX_LOG_ROWS, a missing argument or a challenge that is not canonical (BAD_SHAPE)
static int permutation_zs_args(const AirInfo* a, const TraceInput& in, const uint64_t* challenges, const uint64_t* zs_out, const uint64_t* closing_out) {
    if (!a || a->prog.perm_pairs.empty()) return STARKHIP_ERR_BAD_AIR;
    if (in.check(*a) || !challenges || !zs_out || !closing_out || in.n_rows < 2 || in.n_rows > ((size_t)1 << STARKHIP_MAX_LOG_ROWS) || (in.n_rows & (in.n_rows - 1)))
        return STARKHIP_ERR_BAD_SHAPE;
    for (size_t i = 0; i < (size_t)a->prog.perm_batch_size() * 4; i++)
        if (challenges[i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}

int starkhip_permutation_zs(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                            const uint64_t* challenges, uint64_t* zs_out, uint64_t* closing_out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (int rc = permutation_zs_args(a, in, challenges, zs_out, closing_out)) return rc;
    return guarded([&] { return permutation_zs((Ctx*)ctx, *a, in, challenges, zs_out, closing_out); });
}

int starkhip_permutation_zs_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, const uint64_t* challenges,
                                   uint64_t* zs_out, uint64_t* closing_out) {
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = permutation_zs_args(a, in, challenges, zs_out, closing_out)) return rc;
    return guarded([&] {
        const bool col_major = in.form == TraceForm::ColMajor;
        perm_zs_host(a->prog, n_rows, [&](uint32_t col, size_t row) { return col_major ? trace[(size_t)col * n_rows + row] : trace[row * n_cols + col]; }, challenges,
                     zs_out, closing_out);
        return (int)STARKHIP_OK;
    });
}

int starkhip_air_check_program(const uint64_t* blob, size_t words, char* why, size_t why_len) {
    std::string msg;
    bool ok;
    try {
        ok = air_parse_checked(blob, words, nullptr, &msg);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
    if (why && why_len) {
        const size_t n = std::min(msg.size(), why_len - 1);
        memcpy(why, msg.data(), n);
        why[n] = 0;
    }
    return ok ? STARKHIP_OK : STARKHIP_ERR_BAD_AIR;
}

int starkhip_air_register(const uint64_t* blob, size_t words, const char* name, uint32_t default_rows, starkhip_air_t* id_out) {
    if (!id_out || (default_rows && (default_rows < 2 || default_rows > (1u << STARKHIP_MAX_LOG_ROWS) || (default_rows & (default_rows - 1))))) return STARKHIP_ERR_BAD_SHAPE;
    try {
        AirProgram prog;
        if (!air_parse_checked(blob, words, &prog, nullptr)) return STARKHIP_ERR_BAD_AIR;
        int id = 0;
        const int rc = air_register(std::move(prog), std::vector<uint64_t>(blob, blob + words), name, default_rows, &id);
        if (rc == STARKHIP_OK) *id_out = (starkhip_air_t)id;
        return rc;
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}

static void copy_reason(const std::string& msg, char* why, size_t why_len) {
    if (!why || !why_len) return;
    const size_t n = std::min(msg.size(), why_len - 1);
    memcpy(why, msg.data(), n);
    why[n] = 0;
}

int starkhip_air_check_lookups(const uint64_t* blob, size_t words, const starkhip_lookup_t* lookups, size_t n_lookups, char* why, size_t why_len) {
    std::string msg;
    bool ok;
    try {
        AirProgram prog;
        ok = air_parse_checked(blob, words, &prog, &msg) && air_lookups_ok(prog, lookups, n_lookups, &msg);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
    copy_reason(msg, why, why_len);
    return ok ? STARKHIP_OK : STARKHIP_ERR_BAD_AIR;
}

int starkhip_air_register_lookups(const uint64_t* blob, size_t words, const char* name, uint32_t default_rows, const starkhip_lookup_t* lookups,
                                  size_t n_lookups, starkhip_air_t* id_out) {
    if (!id_out || (default_rows && (default_rows < 2 || default_rows > (1u << STARKHIP_MAX_LOG_ROWS) || (default_rows & (default_rows - 1))))) return STARKHIP_ERR_BAD_SHAPE;
    try {
        AirProgram prog;
        if (!air_parse_checked(blob, words, &prog, nullptr) || !air_lookups_ok(prog, lookups, n_lookups, nullptr)) return STARKHIP_ERR_BAD_AIR;
        int id = 0;
        const int rc = air_register(std::move(prog), std::vector<uint64_t>(blob, blob + words), name, default_rows, &id,
                                    std::vector<starkhip_lookup_t>(lookups, lookups + n_lookups));
        if (rc == STARKHIP_OK) *id_out = (starkhip_air_t)id;
        return rc;
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}

size_t starkhip_air_lookups(starkhip_air_t air, starkhip_lookup_t* out, size_t cap) {
    const AirInfo* a = air_get(air);
    if (!a) return 0;
    if (out) std::copy(a->lookups.begin(), a->lookups.begin() + std::min(cap, a->lookups.size()), out);
    return a->lookups.size();
}

int starkhip_lookup_blob_layout(const uint64_t* blob, size_t words, starkhip_lookup_report_t* out, const uint64_t** list) {
    if (!out || !lookup_blob_read(blob, words, out, list)) return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}

int starkhip_lookup_blob_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, size_t cap, uint64_t** blob,
                                size_t* words) {
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    unsigned log_n = 0;
    if (in.check(*a) || !blob || !words || cap > STARKHIP_CHECK_LIST_MAX || !log2_rows(n_rows, &log_n) || log_n > max_log_rows(*a)) return STARKHIP_ERR_BAD_SHAPE;
    return guarded([&] { return lookup_blob_replay(*a, in, cap, blob, words); });
}

int starkhip_check_trace(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                         const uint64_t* public_inputs, uint64_t* violations, uint64_t first[3]) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (in.check(*a) || !violations || !first || (a->pis && !public_inputs)) return STARKHIP_ERR_BAD_SHAPE;
    return guarded([&] { return check_trace((Ctx*)ctx, *a, in, public_inputs, violations, first); });
}

// what the checkers' entry points refuse before they look at the trace: an unknown AIR, a trace argument that cannot be one of it
// (TraceInput::check), missing public inputs or result -- and `extra`, what the entry refuses of its own arguments
static int checker_args(const AirInfo* a, const TraceInput& in, const uint64_t* public_inputs, const void* out, bool extra) {
    if (!a) return STARKHIP_ERR_BAD_AIR;
    if (in.check(*a) || !out || (a->pis && !public_inputs) || extra) return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}
static bool bad_list(const uint64_t* list, size_t cap) { return cap > STARKHIP_CHECK_LIST_MAX || (cap && !list); }

int starkhip_check_trace_report(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                                const uint64_t* public_inputs, uint32_t* per_constraint, uint64_t* row_mask, uint64_t* list, size_t cap,
                                starkhip_check_report_t* out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (int rc = checker_args(a, in, public_inputs, out, bad_list(list, cap))) return rc;
    return guarded([&] { return check_trace_report((Ctx*)ctx, *a, in, public_inputs, per_constraint, row_mask, list, cap, out); });
}

int starkhip_check_trace_report_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                       const uint64_t* public_inputs, uint32_t* per_constraint, uint64_t* row_mask, uint64_t* list, size_t cap,
                                       starkhip_check_report_t* out) {
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = checker_args(a, in, public_inputs, out, bad_list(list, cap))) return rc;
    return guarded([&] { return check_trace_report_replay(*a, in, public_inputs, per_constraint, row_mask, list, cap, out); });
}

int starkhip_check_blob_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, const uint64_t* public_inputs,
                               size_t cap, uint64_t** blob, size_t* words) {
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = checker_args(a, in, public_inputs, blob, !words || cap > STARKHIP_CHECK_LIST_MAX)) return rc;
    return guarded([&] { return check_blob_replay(*a, in, public_inputs, cap, blob, words); });
}

int starkhip_check_blob_layout(const uint64_t* blob, size_t words, starkhip_check_report_t* out, const uint64_t** list) {
    if (!out || !check_blob_read(blob, words, out, list)) return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}

int starkhip_check_stats(void* ctx, uint64_t out[2]) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    if (!out) return STARKHIP_ERR_BAD_SHAPE;
    ctx_check_stats((Ctx*)ctx, out);
    return STARKHIP_OK;
}

int starkhip_check_trace_free_cells(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                                    const uint64_t* public_inputs, uint64_t delta, uint32_t* per_column, uint64_t* free_mask,
                                    starkhip_free_cells_t* out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (int rc = checker_args(a, in, public_inputs, out, free_cells_bad_delta(delta))) return rc;
    return guarded([&] { return check_trace_free_cells((Ctx*)ctx, *a, in, public_inputs, delta, per_column, free_mask, out); });
}

int starkhip_check_trace_free_cells_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                           const uint64_t* public_inputs, uint64_t delta, uint32_t* per_column, uint64_t* free_mask,
                                           starkhip_free_cells_t* out) {
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = checker_args(a, in, public_inputs, out, free_cells_bad_delta(delta))) return rc;
    return guarded([&] { return check_trace_free_cells_replay(*a, in, public_inputs, delta, per_column, free_mask, out); });
}

int starkhip_check_trace_free_cell_classes(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                           int on_device, const uint64_t* public_inputs, uint64_t delta, uint32_t* per_column,
                                           uint64_t* planes, uint32_t* open_rows, starkhip_free_cell_classes_t* out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (int rc = checker_args(a, in, public_inputs, out, free_cells_bad_delta(delta))) return rc;
    return guarded([&] { return check_trace_free_cell_classes((Ctx*)ctx, *a, in, public_inputs, delta, per_column, planes, open_rows, out); });
}

int starkhip_check_trace_free_cell_classes_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                                  const uint64_t* public_inputs, uint64_t delta, uint32_t* per_column, uint64_t* planes,
                                                  uint32_t* open_rows, starkhip_free_cell_classes_t* out) {
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = checker_args(a, in, public_inputs, out, free_cells_bad_delta(delta))) return rc;
    return guarded([&] { return check_trace_free_cell_classes_replay(*a, in, public_inputs, delta, per_column, planes, open_rows, out); });
}

int starkhip_check_trace_permutations(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                      int on_device, uint64_t seed, uint32_t* per_pair, uint64_t* masks, uint64_t* list, size_t cap,
                                      starkhip_perm_check_t* out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (int rc = perm_check_args(a, in, seed, list, cap, out)) return rc;
    return guarded([&] { return check_trace_permutations((Ctx*)ctx, *a, in, seed, per_pair, masks, list, cap, out); });
}

int starkhip_check_trace_permutations_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, uint64_t seed,
                                             uint32_t* per_pair, uint64_t* masks, uint64_t* list, size_t cap, starkhip_perm_check_t* out) {
    const AirInfo* a = air_get(air);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = perm_check_args(a, in, seed, list, cap, out)) return rc;
    return guarded([&] { return check_trace_permutations_replay(*a, in, seed, per_pair, masks, list, cap, out); });
}

int starkhip_perm_check_seeds(uint64_t seed, uint64_t out[STARKHIP_PERM_CHECK_ATTEMPTS]) {
    if (perm_check_bad_seed(seed) || !out) return STARKHIP_ERR_BAD_SHAPE;
    perm_check_seeds(seed, out);
    return STARKHIP_OK;
}

int starkhip_perm_check_timings(void* ctx, float ms[4]) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    if (!ms) return STARKHIP_ERR_BAD_SHAPE;
    perm_check_timings((Ctx*)ctx, ms);
    return STARKHIP_OK;
}

int starkhip_lookup_columns(void* ctx, uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                            const starkhip_lookup_t* lookups, size_t n_lookups, uint32_t* per_lookup, uint64_t* missing_masks,
                            uint64_t* list, size_t cap, starkhip_lookup_report_t* out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (int rc = lookup_args(in, lookups, n_lookups, list, cap, out)) return rc;
    return guarded([&] { return lookup_columns((Ctx*)ctx, in, trace, lookups, n_lookups, per_lookup, missing_masks, list, cap, out); });
}

int starkhip_lookup_columns_replay(uint64_t* trace, size_t n_rows, size_t n_cols, int layout, const starkhip_lookup_t* lookups,
                                   size_t n_lookups, uint32_t* per_lookup, uint64_t* missing_masks, uint64_t* list, size_t cap,
                                   starkhip_lookup_report_t* out) {
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = lookup_args(in, lookups, n_lookups, list, cap, out)) return rc;
    return guarded([&] { return lookup_columns_replay(in, trace, lookups, n_lookups, per_lookup, missing_masks, list, cap, out); });
}

int starkhip_lookup_timings(void* ctx, float ms[4]) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    if (!ms) return STARKHIP_ERR_BAD_SHAPE;
    lookup_timings((Ctx*)ctx, ms);
    return STARKHIP_OK;
}

int starkhip_air_logup_fillable(starkhip_air_t air) {
    const AirInfo* a = air_get(air);
    if (!a || a->prog.logups.empty()) return STARKHIP_ERR_BAD_AIR;
    return guarded([&] { return logup_fillable(a->prog, nullptr) ? 1 : 0; });
}

int starkhip_logup_frequencies(void* ctx, starkhip_air_t air, uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                               uint32_t* per_lookup, uint32_t* per_column, uint64_t* missing_masks, uint64_t* list, size_t cap,
                               starkhip_logup_report_t* out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const AirInfo* a = air_get(air);
    if (!a || a->prog.logups.empty()) return STARKHIP_ERR_BAD_AIR;
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (int rc = logup_freq_args(*a, in, list, cap, out)) return rc;
    return guarded([&] { return logup_frequencies((Ctx*)ctx, *a, in, trace, per_lookup, per_column, missing_masks, list, cap, out); });
}

int starkhip_logup_frequencies_replay(starkhip_air_t air, uint64_t* trace, size_t n_rows, size_t n_cols, int layout, uint32_t* per_lookup,
                                      uint32_t* per_column, uint64_t* missing_masks, uint64_t* list, size_t cap,
                                      starkhip_logup_report_t* out) {
    const AirInfo* a = air_get(air);
    if (!a || a->prog.logups.empty()) return STARKHIP_ERR_BAD_AIR;
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = logup_freq_args(*a, in, list, cap, out)) return rc;
    return guarded([&] { return logup_frequencies_replay(*a, in, trace, per_lookup, per_column, missing_masks, list, cap, out); });
}

int starkhip_logup_frequency_timings(void* ctx, float ms[5]) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    if (!ms) return STARKHIP_ERR_BAD_SHAPE;
    logup_frequency_timings((Ctx*)ctx, ms);
    return STARKHIP_OK;
}

int starkhip_logup_blob_layout(const uint64_t* blob, size_t words, starkhip_logup_report_t* out, const uint64_t** list) {
    if (!out || !logup_blob_read(blob, words, out, list)) return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}

int starkhip_logup_blob_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, size_t cap, uint64_t** blob,
                               size_t* words) {
    const AirInfo* a = air_get(air);
    if (!a || a->prog.logups.empty()) return STARKHIP_ERR_BAD_AIR;
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    unsigned log_n = 0;
    if (in.check(*a) || !blob || !words || cap > STARKHIP_CHECK_LIST_MAX || !log2_rows(n_rows, &log_n) || log_n > max_log_rows(*a)) return STARKHIP_ERR_BAD_SHAPE;
    return guarded([&] { return logup_fillable(a->prog, nullptr) ? logup_blob_replay(*a, in, cap, blob, words) : (int)STARKHIP_ERR_BAD_AIR; });
}

int starkhip_lookup_air_register(uint32_t n_cols, uint32_t degree, const starkhip_lookup_t* lookups, size_t n_lookups, const char* name, uint32_t default_rows,
                                 starkhip_air_t* id_out) {
    if (!lookups || !id_out) return STARKHIP_ERR_BAD_SHAPE;
    return guarded([&] {
        AirBuilder b(n_cols, 0, degree);
        for (size_t q = 0; q < n_lookups; q++) b.lookup(lookups[q].input, lookups[q].table, lookups[q].permuted_input, lookups[q].permuted_table);
        const std::vector<uint64_t> w = b.finish().serialize();
        std::vector<starkhip_lookup_t> list;  // AirBuilder::lookups(), as the entry takes them
        for (const AirBuilder::Lookup& lk : b.lookups()) list.push_back({lk.input, lk.table, lk.permuted_input, lk.permuted_table});
        return starkhip_air_register_lookups(w.data(), w.size(), name, default_rows, list.data(), list.size(), id_out);
    });
}

int starkhip_lookup_air_blob(uint32_t n_cols, uint32_t degree, const starkhip_lookup_t* lookups, size_t n_lookups, uint64_t* blob,
                             size_t cap_words, size_t* words) {
    if (!lookups || !words || (cap_words && !blob)) return STARKHIP_ERR_BAD_SHAPE;
    return guarded([&] {
        AirBuilder b(n_cols, 0, degree);
        for (size_t q = 0; q < n_lookups; q++) b.lookup(lookups[q].input, lookups[q].table, lookups[q].permuted_input, lookups[q].permuted_table);
        const std::vector<uint64_t> w = b.finish().serialize();
        *words = w.size();
        if (w.size() > cap_words) return (int)STARKHIP_ERR_BAD_SHAPE;
        std::copy(w.begin(), w.end(), blob);
        return (int)STARKHIP_OK;
    });
}

int starkhip_quotient_plan_check(starkhip_air_t air, unsigned want_chunks, uint64_t seed, uint64_t stats[8]) {
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    try {
        QTPlan Q = build_quotient_plan(a->prog, want_chunks);
        uint64_t s = seed;
        auto rnd = [&]() {  // splitmix64, reduced
            s += 0x9E3779B97F4A7C15ULL;
            uint64_t z = s;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
            return gl_from_u64((z ^ (z >> 31)) % GL_P);
        };
        std::vector<gl_t> local(a->cols), next(a->cols), pis(a->pis ? a->pis : 1);
        for (auto& v : local) v = rnd();
        for (auto& v : next) v = rnd();
        for (auto& v : pis) v = rnd();
        gl_t masks[4] = {1, rnd(), rnd(), rnd()}, alphas[2] = {rnd(), rnd()}, want[2], got[2];
        air_eval_folded<BaseOps>(a->prog, local.data(), next.data(), pis.data(), masks, alphas, 2, want);
        quotient_plan_weights_host(a->prog, Q, alphas, pis.data());
        const bool ok = quotient_plan_eval_host(Q, local.data(), next.data(), masks, got);
        if (stats) {
            stats[0] = Q.n_chunks; stats[1] = Q.n_supergroups; stats[2] = Q.n_pieces; stats[3] = Q.recs.size();
            stats[4] = Q.n_cell_records; stats[5] = Q.n_direct_loads; stats[6] = Q.tile_list.size(); stats[7] = Q.contribs.size();
            if (seed == 0xBA1A) { stats[6] = Q.cost_sum_max; stats[7] = Q.cost_sum_mean; }  // balance figures (tools)
            if (seed == 0xBA1B) { stats[4] = Q.n_piece_ends; stats[5] = Q.tile_phases; stats[6] = Q.rec_sum_max; stats[7] = Q.rec_sum_total; }
            if (seed == 0xBA1C) {  // the announcements (tools): fast pairs, direct pairs, and the direct second factors there are
                uint64_t fast = 0, dpairs = 0, direct_b = 0, direct_b_end = 0;
                for (const QTRec& r : Q.recs) {
                    if ((r.ctl & QT_SPECIAL) != 0 && !(r.ctl & QT_SRC_GLOBAL) && !(r.ctl & QT_STOP)) {
                        fast += r.aux & QT_AUX_PAIRS_MASK;
                        dpairs += (r.aux >> QT_AUX_DPAIRS_SHIFT) & QT_AUX_DPAIRS_MASK;
                    }
                    if ((r.ctl & (QT_SRC_GLOBAL | QT_MULV | QT_SETV)) == (QT_SRC_GLOBAL | QT_MULV) && !(r.aux & QT_AUX_SLOT)) (r.ctl & QT_END ? direct_b_end : direct_b)++;
                }
                stats[4] = fast; stats[5] = dpairs; stats[6] = direct_b; stats[7] = direct_b_end;
            }
        }
        if (!ok) return STARKHIP_ERR_BAD_SHAPE;
        return (want[0] == got[0] && want[1] == got[1]) ? STARKHIP_OK : STARKHIP_ERR_VERIFY;
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    } catch (const std::exception&) {
        return STARKHIP_ERR_BAD_SHAPE;
    }
}

int starkhip_quotient_classes(starkhip_air_t air, uint8_t* classes, size_t n) {
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    if (!classes || n != a->prog.n_constraints) return STARKHIP_ERR_BAD_SHAPE;
    return guarded([&] {
        const std::vector<uint8_t> cls = quotient_constraint_classes(a->prog, quotient_factor(a->prog.degree));
        std::copy(cls.begin(), cls.end(), classes);
        return (int)STARKHIP_OK;
    });
}

int starkhip_quotient_solve_table(unsigned log_rows, unsigned quotient_degree_bits, uint64_t* out, size_t n) {
    if (!out || n != QT_SOLVE_WORDS || log_rows > 32) return STARKHIP_ERR_BAD_SHAPE;
    return guarded([&] {
        const std::vector<gl_t> tab = quotient_solve_table(log_rows, quotient_degree_bits);
        std::copy(tab.begin(), tab.end(), out);
        return (int)STARKHIP_OK;
    });
}

int starkhip_quotient_class_plan_check(starkhip_air_t air, unsigned want_chunks, uint64_t seed, uint64_t stats[32]) {
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    return guarded([&] {
        const AirProgram& P = a->prog;
        const unsigned n_classes = quotient_factor(P.degree), n_cosets = 1u << quotient_degree_bits(P.degree);
        QTClassPlan CP = build_quotient_class_plan(P, want_chunks, n_classes, n_cosets);
        const std::vector<uint8_t> cls = quotient_constraint_classes(P, n_classes);
        uint64_t s = seed;
        auto rnd = [&]() {  // splitmix64, reduced
            s += 0x9E3779B97F4A7C15ULL;
            uint64_t z = s;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
            return gl_from_u64((z ^ (z >> 31)) % GL_P);
        };
        std::vector<gl_t> local(a->cols), next(a->cols), pis(a->pis ? a->pis : 1);
        for (auto& v : local) v = rnd();
        for (auto& v : next) v = rnd();
        for (auto& v : pis) v = rnd();
        gl_t masks[4] = {1, rnd(), rnd(), rnd()}, alphas[2] = {rnd(), rnd()};
        // the plain fold acc alpha + mask c, restricted to each class: acc_j[class] = sum_k in class mask c_k alpha_j^(K-1-k)
        std::vector<gl_t> want(2 * (n_classes + 1), 0);
        {
            const uint32_t K = P.n_constraints;
            std::vector<gl_t> body(K);  // mask(kind) * gates * c_k
            AirReader rd(P);
            GroupWord grp;
            uint32_t k = 0;
            auto cell = [&](uint32_t ref) { return ((ref & REF_NEXT) ? next : local)[ref & REF_COL_MASK]; };
            while (rd.group(&grp)) {
                gl_t G = masks[grp.kind];
                for (uint32_t g = 0; g < grp.n_gates; g++) {
                    const uint32_t ref = rd.ref();
                    G = gl_mul(G, (ref & REF_COMPL) ? gl_sub(1, cell(ref)) : cell(ref));
                }
                for (uint32_t c = 0; c < grp.m; c++, k++) {
                    gl_t b = 0;
                    TermWord tw;
                    do {
                        tw = rd.term();
                        gl_t v = 1;
                        for (uint32_t f = 0; f < tw.nf; f++) v = gl_mul(v, cell(rd.ref()));
                        const gl_t coef = tw.ck == CK_PLUS ? 1 : tw.ck == CK_MINUS ? GL_P - 1 : tw.ck == CK_CONST ? P.consts[tw.idx] : tw.ck == CK_PI ? pis[tw.idx] : gl_neg(pis[tw.idx]);
                        b = gl_add(b, gl_mul(v, coef));
                    } while (!tw.last);
                    body[k] = gl_mul(G, b);
                }
            }
            for (int j = 0; j < 2; j++) {
                gl_t pw = 1;
                for (uint32_t e = 0; e < K; e++, pw = gl_mul(pw, alphas[j])) {
                    const uint32_t kk = K - 1 - e;
                    want[2 * (cls[kk] - 1) + j] = gl_add(want[2 * (cls[kk] - 1) + j], gl_mul(body[kk], pw));
                }
                for (unsigned c = 0; c < n_classes; c++) want[2 * n_classes + j] = gl_add(want[2 * n_classes + j], want[2 * c + j]);
            }
            gl_t full[2];
            air_eval_folded<BaseOps>(P, local.data(), next.data(), pis.data(), masks, alphas, 2, full);
            if (full[0] != want[2 * n_classes] || full[1] != want[2 * n_classes + 1]) return (int)STARKHIP_ERR_VERIFY;  // the classes sum to the full fold
        }
        quotient_plan_weights_host(P, CP.plan, alphas, pis.data());
        // coset t: its chunks are its work rows, and the sums of its accumulators are the restricted folds of the classes above t (a
        // spare coset: the whole fold in accumulator 0) -- nothing of a class at or below t
        bool ok = CP.coset_chunk_off.size() == n_cosets + 1 && CP.work.size() == CP.plan.n_chunks;
        for (unsigned t = 0; ok && t < n_cosets; t++) {
            gl_t got[2], by_acc[QT_MAX_ACCS][2];
            ok = quotient_plan_eval_host(CP.plan, local.data(), next.data(), masks, got, CP.coset_chunk_off[t], CP.coset_chunk_off[t + 1], by_acc);
            for (unsigned a = 0; ok && a < QT_MAX_ACCS; a++) {
                const bool runs = t < n_classes ? (a >= t && a < n_classes) : a == 0;
                const gl_t* w = t < n_classes ? &want[2 * a] : &want[2 * n_classes];
                if (runs ? (by_acc[a][0] != w[0] || by_acc[a][1] != w[1]) : (by_acc[a][0] != 0 || by_acc[a][1] != 0)) return (int)STARKHIP_ERR_VERIFY;
            }
            for (uint32_t r = CP.coset_chunk_off[t]; ok && r < CP.coset_chunk_off[t + 1]; r++)
                ok = CP.work[r].chunk == r && CP.work[r].coset == t && CP.work[r].acc_lo == (t < n_classes ? t : 0u) && CP.work[r].acc_hi == (t < n_classes ? n_classes : 1u);
        }
        if (stats) {
            for (int i = 0; i < 32; i++) stats[i] = 0;
            stats[0] = n_classes; stats[1] = n_cosets; stats[2] = CP.plan.n_chunks; stats[3] = CP.work.size(); stats[4] = CP.plan.recs.size();
            stats[5] = CP.plan.n_piece_ends; stats[6] = CP.plan.tile_phases; stats[7] = CP.plan.contribs.size();
            for (unsigned c = 0; c < n_classes && c < 8; c++) stats[8 + c] = CP.class_constraints[c];
            for (unsigned t = 0; t < n_cosets && t < 8; t++) stats[24 + t] = CP.coset_chunk_off[t + 1] - CP.coset_chunk_off[t];
        }
        return (int)(ok ? STARKHIP_OK : STARKHIP_ERR_BAD_SHAPE);
    });
}

int starkhip_init(int device_ordinal, void** ctx) {
    Ctx* c = nullptr;
    int rc = ctx_create(device_ordinal, &c);
    *ctx = c;
    return rc;
}
void starkhip_shutdown(void* ctx) { ctx_destroy((Ctx*)ctx); }

// the three starkhip_prove* entries once each has named its trace; `armed`: it is a recording that is still armed on this thread
static int prove_entry(void* ctx, starkhip_air_t air, const starkhip_config_t* cfg, const TraceInput& in, bool armed, const uint64_t* public_inputs,
                       size_t n_pis, uint64_t pow_witness, uint64_t** proof, size_t* proof_words) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    if (armed || in.check(*a) || !cfg || !proof || !proof_words || (n_pis && !public_inputs)) return STARKHIP_ERR_BAD_SHAPE;
    return guarded([&] { return prove((Ctx*)ctx, *a, *cfg, in, public_inputs, n_pis, pow_witness, proof, proof_words); });
}

int starkhip_prove(void* ctx, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* trace, size_t n_rows, size_t n_cols,
                   int trace_layout, int trace_on_device, const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness, uint64_t** proof,
                   size_t* proof_words) {
    return prove_entry(ctx, air, cfg, TraceInput::dense(trace, n_rows, n_cols, trace_layout, trace_on_device), false, public_inputs, n_pis, pow_witness,
                       proof, proof_words);
}

int starkhip_prove_columns(void* ctx, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* const* columns, size_t n_rows, size_t n_cols,
                           const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness, uint64_t** proof, size_t* proof_words) {
    return prove_entry(ctx, air, cfg, TraceInput::column_table(columns, n_rows, n_cols), false, public_inputs, n_pis, pow_witness, proof, proof_words);
}

int starkhip_set_option(void* ctx, const char* name, long value) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return ctx_set_option((Ctx*)ctx, name, value);
}

int starkhip_proof_layout(const uint64_t* proof, size_t proof_words, starkhip_proof_layout_t* out) {
    if (!proof || !out) return STARKHIP_ERR_BAD_SHAPE;
    ProofLayout pl;
    if (!pl.read_header(proof, proof_words)) return STARKHIP_ERR_BAD_SHAPE;
    memset(out, 0, sizeof *out);
    out->n_columns = pl.C; out->n_quotient_polys = pl.Q; out->degree_bits = pl.log_n; out->rate_bits = pl.rate_bits;
    out->cap_height = pl.cap_h; out->n_fri_layers = pl.L; out->n_query_rounds = pl.n_queries; out->final_poly_len = pl.final_len;
    out->n_public_inputs = pl.n_pis; out->arity_bits = pl.arity_bits;
    const MatrixLayout &t = pl.mat[0], z = pl.n_mats == 3 ? pl.mat[1] : MatrixLayout(), &q = pl.quotient();  // (z: all 0 for a proof without Zs)
    out->off_trace_cap = t.off_cap; out->off_quotient_cap = q.off_cap; out->off_local_values = t.off_open[0];
    out->off_next_values = t.off_open[1]; out->off_quotient_openings = q.off_open[0]; out->off_fri_caps = pl.off_fri_caps;
    out->off_query_rounds = pl.off_queries; out->query_round_words = pl.query_words; out->off_final_poly = pl.off_final;
    out->off_pow_witness = pl.off_pow; out->off_public_inputs = pl.off_pis; out->total_words = pl.total;
    const size_t d0 = pl.log_N - pl.cap_h;
    out->q_trace_leaf = t.q_leaf; out->q_trace_siblings = t.q_sib; out->q_quotient_leaf = q.q_leaf; out->q_quotient_siblings = q.q_sib;
    out->n_permutation_zs = pl.nZ; out->n_logup_polys = pl.nA; out->off_permutation_zs_cap = z.off_cap; out->off_permutation_zs = z.off_open[0];
    out->off_permutation_zs_next = z.off_open[1]; out->q_permutation_zs_leaf = z.q_leaf; out->q_permutation_zs_siblings = z.q_sib;
    out->n_ctl_polys = pl.nC; out->off_ctl_sums = pl.nC ? pl.off_sums : 0;  // (all 0 for a proof that is no table proof with endpoints)
    size_t o = q.q_sib + 4 * d0;
    for (size_t l = 0; l < pl.L && l < 16; l++) {
        out->q_step_evals[l] = o; o += 2 * ((size_t)1 << pl.arity_bits);
        out->q_step_siblings[l] = o; o += 4 * pl.layer_depth[l];
        out->step_sibling_count[l] = pl.layer_depth[l];
    }
    out->initial_sibling_count = d0;
    return STARKHIP_OK;
}

// ---- compact traces (trace_log.h)
int starkhip_trace_set_threads(int n) {
    if (n < 1) n = 1;
    if (n > 64) n = 64;
    return g_trace_threads.exchange(n);
}
int starkhip_trace_log_begin(void** log) {
    if (!log) return STARKHIP_ERR_BAD_SHAPE;
    *log = nullptr;
    if (armed_trace_log()) return STARKHIP_ERR_BAD_SHAPE;  // already recording on this thread
    TraceLog* l = new (std::nothrow) TraceLog();
    if (!l) return STARKHIP_ERR_OOM;
    armed_trace_log() = l;
    *log = l;
    return STARKHIP_OK;
}
int starkhip_trace_log_end(void* log) {
    if (!log || armed_trace_log() != (TraceLog*)log) return STARKHIP_ERR_BAD_SHAPE;
    armed_trace_log() = nullptr;
    TraceLog* l = (TraceLog*)log;
    l->open.clear();
    l->open.shrink_to_fit();
    return l->rows ? STARKHIP_OK : STARKHIP_ERR_BAD_SHAPE;  // no generator ran in between
}
void starkhip_trace_log_free(void* log) {
    if (log && armed_trace_log() == (TraceLog*)log) armed_trace_log() = nullptr;
    delete (TraceLog*)log;
}
int starkhip_trace_log_info(const void* log, size_t* n_rows, size_t* n_cols, size_t* n_records, size_t* n_words) {
    if (!log) return STARKHIP_ERR_BAD_SHAPE;
    const TraceLog* l = (const TraceLog*)log;
    if (n_rows) *n_rows = l->rows;
    if (n_cols) *n_cols = l->cols;
    if (n_records) *n_records = l->total_records();
    if (n_words) *n_words = l->total_words();
    return STARKHIP_OK;
}
int starkhip_trace_log_from_writes(size_t n_rows, size_t n_cols, const uint64_t* writes, size_t n_writes, void** log) {
    if (!log || (n_writes && !writes) || !n_rows || !n_cols) return STARKHIP_ERR_BAD_SHAPE;
    *log = nullptr;
    TraceLog* l = new (std::nothrow) TraceLog();
    if (!l) return STARKHIP_ERR_OOM;
    try {
        l->reset(n_rows, n_cols);
        for (size_t i = 0; i < n_writes; i++) l->set((size_t)writes[3 * i], (size_t)writes[3 * i + 1], writes[3 * i + 2]);
    } catch (const std::bad_alloc&) {
        delete l;
        return STARKHIP_ERR_OOM;
    } catch (const std::exception&) {  // a write outside the trace, a value of more than 32 bits
        delete l;
        return STARKHIP_ERR_BAD_SHAPE;
    }
    l->open.clear();
    l->open.shrink_to_fit();
    *log = l;
    return STARKHIP_OK;
}
int starkhip_trace_log_overwrites(const void* log, size_t* empty_runs, size_t* late_zeros) {
    if (!log) return STARKHIP_ERR_BAD_SHAPE;
    const TraceLog* l = (const TraceLog*)log;
    size_t empty = 0;
    l->for_each_part([&](const TraceLog& part) {
        for (uint32_t off : part.offsets) empty += part.words[off - part.base + 2] == 0;
    });
    if (empty_runs) *empty_runs = empty;
    if (late_zeros) *late_zeros = l->total_late_zeros() / 2;
    return STARKHIP_OK;
}
int starkhip_trace_log_expand_host(const void* log, uint64_t* trace_rowmajor, size_t* conflicts) {
    if (!log || !trace_rowmajor) return STARKHIP_ERR_BAD_SHAPE;
    const TraceLog* l = (const TraceLog*)log;
    memset(trace_rowmajor, 0, l->rows * l->cols * sizeof(uint64_t));
    size_t bad = 0;
    l->for_each_part([&](const TraceLog& part) {
        for (uint32_t off : part.offsets) {
            const uint32_t* r = &part.words[off - part.base];
            for (uint32_t k = 0; k < r[2]; k++)
                for (uint32_t i = 0; i < r[3]; i++) {
                    uint64_t& cell = trace_rowmajor[(size_t)(r[1] + k) * l->cols + r[0] + i];
                    if (cell && cell != r[4 + i]) bad++;  // two records disagree: parallel expansion would be order dependent
                    cell = r[4 + i];
                }
        }
    });
    l->for_each_part([&](const TraceLog& part) {
        for (size_t i = 0; i + 1 < part.late_zeros.size(); i += 2)
            trace_rowmajor[(size_t)part.late_zeros[i + 1] * l->cols + part.late_zeros[i]] = 0;
    });
    if (conflicts) *conflicts = bad;
    return STARKHIP_OK;
}
int starkhip_prove_compact(void* ctx, starkhip_air_t air, const starkhip_config_t* cfg, const void* log, const uint64_t* public_inputs,
                           size_t n_pis, uint64_t pow_witness, uint64_t** proof, size_t* proof_words) {
    return prove_entry(ctx, air, cfg, TraceInput::recording(log), log && armed_trace_log() == (const TraceLog*)log, public_inputs, n_pis, pow_witness,
                       proof, proof_words);
}

// ---- proof pool (pool.cpp)
// One hardware queue per in-flight proof: with HIP's default of 4, streams share queues and kernels of different proofs serialise behind
// each other (-6 % on the FinalExp pool).  The runtime reads GPU_MAX_HW_QUEUES ONCE, when the process first uses HIP, so setting it here
// works only in a process that has not.  Whether it has is visible without touching HIP: initialising the runtime opens the compute
// driver's device node, /dev/kfd.  0 = the variable was in the environment before the runtime came up (ours or the caller's own);
// 1 = the runtime was already up when the first pool set it: the pools run on HIP's default, and the caller should export the variable
// itself, earlier (bench.py does).
// The value IN EFFECT (starkhip_hw_queues_in_effect): the variable's when it was there before the runtime came up -- a caller's own value
// is respected, whatever it is --, HIP's default of 4 when it came late.
static std::atomic<int> g_hw_queues_late(-1), g_hw_queues_in_effect(0);
static bool hip_runtime_is_up() {
    DIR* d = opendir("/proc/self/fd");  // every descriptor, whatever its number (a server may hold thousands)
    if (!d) return false;
    bool up = false;
    char link[300], target[256];
    while (const dirent* e = readdir(d)) {
        if (e->d_name[0] == '.') continue;
        snprintf(link, sizeof link, "/proc/self/fd/%s", e->d_name);
        const ssize_t n = readlink(link, target, sizeof target - 1);
        if (n <= 0) continue;
        target[n] = 0;
        if (strcmp(target, "/dev/kfd") == 0) {
            up = true;
            break;
        }
    }
    closedir(d);
    return up;
}
static void ask_for_hw_queues() {
    static std::once_flag once;  // decided with the first pool, by one thread (setenv beside another thread's getenv is a race)
    std::call_once(once, [] {
        int late = 0;
        if (!getenv("GPU_MAX_HW_QUEUES")) {
            late = hip_runtime_is_up() ? 1 : 0;
            setenv("GPU_MAX_HW_QUEUES", "16", 0);
        }
        const int asked = atoi(getenv("GPU_MAX_HW_QUEUES"));
        g_hw_queues_in_effect.store(late || asked <= 0 ? 4 : asked);
        g_hw_queues_late.store(late);
    });
}
// Once per process, by the first pool whose default-class streams outnumber the queues: its contexts share hardware queues.
static void hint_hw_queues(unsigned budget) {
    const int have = g_hw_queues_in_effect.load();
    static std::atomic<bool> said(false);
    if (have <= 0 || (unsigned)have >= budget || said.exchange(true)) return;
    fprintf(stderr, "starkhip: this process has %d hardware queues per stream priority class (%s) and the pool keeps %u streams busy: contexts "
                    "share queues, and a kernel waits for the kernels enqueued before it on its queue (the pool's long launches hold none of "
                    "them; eight FinalExp contexts measured about 1 %% slower on 4 queues than on 16). To give every context a queue, export "
                    "GPU_MAX_HW_QUEUES=16 before the process first uses HIP.\n",
            have, g_hw_queues_late.load() == 1 ? "the HIP runtime was initialised before the first pool could set GPU_MAX_HW_QUEUES" : "GPU_MAX_HW_QUEUES in the environment",
            budget);
}
int starkhip_hw_queues_status(void) { return std::max(0, g_hw_queues_late.load()); }
int starkhip_hw_queues_in_effect(void) { return g_hw_queues_in_effect.load(); }

int starkhip_pool_create(const starkhip_pool_config_t* cfg, void** pool) {
    if (!cfg || !pool) return STARKHIP_ERR_BAD_SHAPE;
    *pool = nullptr;
    ask_for_hw_queues();
    Pool* p = nullptr;
    try {
        const int rc = pool_create(*cfg, &p);
        *pool = p;
        starkhip_pool_host_info_t hi;
        if (rc == STARKHIP_OK && pool_host_info(p, &hi) == STARKHIP_OK) hint_hw_queues(hi.stream_budget);
        return rc;
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    } catch (const std::exception&) {
        return STARKHIP_ERR_HIP;
    }
}
void starkhip_pool_destroy(void* pool) { pool_destroy((Pool*)pool); }
int starkhip_pool_submit(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* trace, size_t n_rows, size_t n_cols,
                         int trace_layout, int trace_on_device, const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness,
                         uint64_t* ticket) {
    if (!pool) return STARKHIP_ERR_NO_DEVICE;
    return pool_submit((Pool*)pool, air, cfg, TraceInput::dense(trace, n_rows, n_cols, trace_layout, trace_on_device), public_inputs, n_pis, pow_witness,
                       ticket);
}
int starkhip_pool_submit_columns(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* const* columns, size_t n_rows,
                                 size_t n_cols, const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness, uint64_t* ticket) {
    if (!pool) return STARKHIP_ERR_NO_DEVICE;
    return pool_submit((Pool*)pool, air, cfg, TraceInput::column_table(columns, n_rows, n_cols), public_inputs, n_pis, pow_witness, ticket);
}
int starkhip_pool_submit_compact(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const void* log, const uint64_t* public_inputs,
                                 size_t n_pis, uint64_t pow_witness, uint64_t* ticket) {
    if (!pool) return STARKHIP_ERR_NO_DEVICE;
    if (log && armed_trace_log() == (const TraceLog*)log) return STARKHIP_ERR_BAD_SHAPE;
    return pool_submit((Pool*)pool, air, cfg, TraceInput::recording(log), public_inputs, n_pis, pow_witness, ticket);
}
int starkhip_pool_submit_witness(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const uint32_t* operands, size_t n_limbs,
                                 uint64_t pow_witness, uint64_t* ticket) {
    if (!pool) return STARKHIP_ERR_NO_DEVICE;
    try {
        return pool_submit_witness((Pool*)pool, air, cfg, operands, n_limbs, pow_witness, ticket);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}
int starkhip_pool_wait(void* pool, uint64_t ticket, uint64_t** proof, size_t* proof_words, starkhip_ticket_info_t* info) {
    if (!pool) return STARKHIP_ERR_NO_DEVICE;
    return pool_wait((Pool*)pool, ticket, proof, proof_words, info);
}
int starkhip_pool_reservation(void* pool, starkhip_pool_reservation_t* out) {
    if (!pool || !out) return STARKHIP_ERR_BAD_SHAPE;
    return pool_reservation((Pool*)pool, out);
}
int starkhip_pool_host_info(void* pool, starkhip_pool_host_info_t* out) {
    if (!pool || !out) return STARKHIP_ERR_BAD_SHAPE;
    return pool_host_info((Pool*)pool, out);
}
unsigned starkhip_cpu_budget(void) { return cpu_budget(); }
void starkhip_host_cpu_seconds(double out[3]) {
    if (out) host_cpu_seconds(out);
}
int starkhip_pool_stats(void* pool, starkhip_pool_stats_t* out) {
    if (!pool || !out) return STARKHIP_ERR_BAD_SHAPE;
    return pool_stats((Pool*)pool, out);
}

int starkhip_pool_set_option(void* pool, const char* name, long value) {
    if (!pool) return STARKHIP_ERR_NO_DEVICE;
    try {
        return pool_set_option((Pool*)pool, name, value);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}
int starkhip_pool_submit_verify(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* proof, size_t proof_words,
                                uint64_t* ticket) {
    if (!pool) return STARKHIP_ERR_NO_DEVICE;
    try {
        return pool_submit_verify((Pool*)pool, air, cfg, proof, proof_words, ticket);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}
int starkhip_pool_verify_stats(void* pool, starkhip_pool_verify_stats_t* out) {
    if (!pool || !out) return STARKHIP_ERR_BAD_SHAPE;
    return pool_verify_stats((Pool*)pool, out);
}

int starkhip_pool_check_stats(void* pool, uint64_t out[2]) {
    if (!pool || !out) return STARKHIP_ERR_BAD_SHAPE;
    return pool_check_stats((Pool*)pool, out);
}

// ---- a pool per device behind one handle (multipool.cpp)
int starkhip_multipool_create(const int* devices, size_t n_devices, const starkhip_pool_config_t* cfg, void** mpool) {
    if (!devices || !n_devices || !cfg || !mpool) return STARKHIP_ERR_BAD_SHAPE;
    *mpool = nullptr;
    ask_for_hw_queues();
    MultiPool* mp = nullptr;
    try {
        const int rc = multipool_create(devices, n_devices, *cfg, &mp);
        *mpool = mp;
        starkhip_pool_host_info_t hi;
        if (rc == STARKHIP_OK && multipool_size(mp) && pool_host_info(multipool_pool(mp, 0), &hi) == STARKHIP_OK) hint_hw_queues(hi.stream_budget);
        return rc;
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    } catch (const std::exception&) {
        return STARKHIP_ERR_HIP;
    }
}
void starkhip_multipool_destroy(void* mpool) { multipool_destroy((MultiPool*)mpool); }
size_t starkhip_multipool_size(const void* mpool) { return mpool ? multipool_size((const MultiPool*)mpool) : 0; }
void* starkhip_multipool_pool(void* mpool, size_t slot) { return mpool ? (void*)multipool_pool((MultiPool*)mpool, slot) : nullptr; }
int starkhip_multipool_device(const void* mpool, size_t slot) { return mpool ? multipool_device((const MultiPool*)mpool, slot) : -1; }
int starkhip_multipool_submit(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* trace, size_t n_rows,
                              size_t n_cols, int trace_layout, int trace_on_device, const uint64_t* public_inputs, size_t n_pis,
                              uint64_t pow_witness, uint64_t* ticket) {
    if (!mpool) return STARKHIP_ERR_NO_DEVICE;
    return multipool_submit((MultiPool*)mpool, slot, air, cfg, TraceInput::dense(trace, n_rows, n_cols, trace_layout, trace_on_device), public_inputs,
                            n_pis, pow_witness, ticket);
}
int starkhip_multipool_submit_columns(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* const* columns,
                                      size_t n_rows, size_t n_cols, const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness,
                                      uint64_t* ticket) {
    if (!mpool) return STARKHIP_ERR_NO_DEVICE;
    return multipool_submit((MultiPool*)mpool, slot, air, cfg, TraceInput::column_table(columns, n_rows, n_cols), public_inputs, n_pis, pow_witness,
                            ticket);
}
int starkhip_multipool_submit_compact(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const void* log,
                                      const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness, uint64_t* ticket) {
    if (!mpool) return STARKHIP_ERR_NO_DEVICE;
    if (log && armed_trace_log() == (const TraceLog*)log) return STARKHIP_ERR_BAD_SHAPE;
    return multipool_submit((MultiPool*)mpool, slot, air, cfg, TraceInput::recording(log), public_inputs, n_pis, pow_witness, ticket);
}
int starkhip_multipool_submit_witness(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const uint32_t* operands,
                                      size_t n_limbs, uint64_t pow_witness, uint64_t* ticket) {
    if (!mpool) return STARKHIP_ERR_NO_DEVICE;
    try {
        return multipool_submit_witness((MultiPool*)mpool, slot, air, cfg, operands, n_limbs, pow_witness, ticket);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}
int starkhip_multipool_submit_witness_batch(void* mpool, size_t n_jobs, const starkhip_air_t* airs, const uint32_t* const* operands,
                                            const size_t* n_limbs, uint64_t pow_witness, uint64_t* tickets, int* rcs) {
    if (!mpool) return STARKHIP_ERR_NO_DEVICE;
    static_assert(sizeof(starkhip_air_t) == sizeof(int), "air ids travel as int");
    try {
        return multipool_submit_witness_batch((MultiPool*)mpool, n_jobs, (const int*)airs, operands, n_limbs, pow_witness, tickets, rcs);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}
int starkhip_multipool_ticket_slot(const void* mpool, uint64_t ticket) { return mpool ? multipool_ticket_slot((const MultiPool*)mpool, ticket) : -1; }
int starkhip_multipool_wait(void* mpool, uint64_t ticket, uint64_t** proof, size_t* proof_words, starkhip_ticket_info_t* info) {
    if (!mpool) return STARKHIP_ERR_NO_DEVICE;
    return multipool_wait((MultiPool*)mpool, ticket, proof, proof_words, info);
}
int starkhip_multipool_set_option(void* mpool, const char* name, long value) {
    if (!mpool) return STARKHIP_ERR_NO_DEVICE;
    try {
        return multipool_set_option((MultiPool*)mpool, name, value);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}
int starkhip_multipool_submit_verify(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* proof,
                                     size_t proof_words, uint64_t* ticket) {
    if (!mpool) return STARKHIP_ERR_NO_DEVICE;
    try {
        return multipool_submit_verify((MultiPool*)mpool, slot, air, cfg, proof, proof_words, ticket);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}
int starkhip_multipool_verify_batch(void* mpool, size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                                    const size_t* proof_words, int* results) {
    if (!mpool) return STARKHIP_ERR_NO_DEVICE;
    try {
        return multipool_verify_batch((MultiPool*)mpool, n, (const int*)airs, cfgs, proofs, proof_words, results);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}
int starkhip_plan_verify(size_t n, const starkhip_air_t* airs, size_t n_pools, int* slots, size_t* order) {
    if ((n && (!airs || !slots)) || !n_pools) return STARKHIP_ERR_BAD_SHAPE;
    plan_verify(n, (const int*)airs, n_pools, slots, order);
    return STARKHIP_OK;
}
double starkhip_air_verify_cost(starkhip_air_t air) { return air_verify_cost(air); }
int starkhip_plan_lpt(size_t n_jobs, const starkhip_air_t* airs, size_t n_pools, int* slots) {
    if ((n_jobs && (!airs || !slots)) || !n_pools) return STARKHIP_ERR_BAD_SHAPE;
    plan_lpt(n_jobs, (const int*)airs, n_pools, slots);
    return STARKHIP_OK;
}
double starkhip_air_cost(starkhip_air_t air) { return air_cost((int)air); }

int starkhip_last_timings(void* ctx, float ms[STARKHIP_N_PHASES]) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    memcpy(ms, ctx_timings((Ctx*)ctx), sizeof(float) * STARKHIP_N_PHASES);
    return STARKHIP_OK;
}

int starkhip_last_kernel_timings(void* ctx, float ms[3]) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    memcpy(ms, ctx_kernel_timings((Ctx*)ctx), sizeof(float) * 3);
    return STARKHIP_OK;
}

int starkhip_last_host_timings(void* ctx, float ms[2]) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    memcpy(ms, ctx_host_timings((Ctx*)ctx), sizeof(float) * 2);
    return STARKHIP_OK;
}

int starkhip_host_alloc(void* ctx, size_t bytes, void** out) {
    if (!out) return STARKHIP_ERR_BAD_SHAPE;
    *out = nullptr;
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return host_alloc((Ctx*)ctx, bytes, out);
}
void starkhip_host_free(void* p) { host_free(p); }

int starkhip_lde_batch(void* ctx, const uint64_t* values, size_t n_cols, unsigned log_n, unsigned rate_bits, uint64_t* coeffs_out,
                       uint64_t* lde_out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return lde_batch((Ctx*)ctx, values, n_cols, log_n, rate_bits, coeffs_out, lde_out);
}
int starkhip_ntt_long(void* ctx, uint64_t* data, size_t n_vecs, unsigned log_len, int inverse) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return ntt_long((Ctx*)ctx, data, n_vecs, log_len, inverse);
}
int starkhip_merkle_cap(void* ctx, const uint64_t* lde_colmajor, size_t n_cols, unsigned log_N, unsigned cap_height, uint64_t* cap_out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return merkle_cap((Ctx*)ctx, lde_colmajor, n_cols, log_N, cap_height, cap_out);
}
int starkhip_lde_bench(void* ctx, size_t n_cols, unsigned log_n, unsigned rate_bits, unsigned reps, unsigned const_per_64, const uint64_t* device_values, float* ms_per_launch, float* each_ms) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    if (!ms_per_launch) return STARKHIP_ERR_BAD_SHAPE;
    return lde_bench((Ctx*)ctx, n_cols, log_n, rate_bits, reps, const_per_64, device_values, ms_per_launch, each_ms);
}
int starkhip_trace_log_expand_device(void* ctx, const void* log, uint64_t* trace_colmajor) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    if (!log || !trace_colmajor || armed_trace_log() == (const TraceLog*)log) return STARKHIP_ERR_BAD_SHAPE;
    try {
        return expand_log((Ctx*)ctx, (const TraceLog*)log, trace_colmajor);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}
int starkhip_poseidon_permute_batch(void* ctx, uint64_t* states, size_t n_states) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return permute_batch((Ctx*)ctx, states, n_states);
}
int starkhip_poseidon_permute_batch_form(void* ctx, int form, int variant, uint64_t* states, size_t n_states) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return permute_batch_form((Ctx*)ctx, form, variant, states, n_states);
}
int starkhip_leaf_hash_lane_group(void* ctx, const uint64_t* mats, size_t n_segments, size_t n_cols, unsigned log_n, unsigned rate_bits, int grouped,
                                  int form, unsigned prefix_mask, uint64_t* digests_out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return leaf_hash_lane_group((Ctx*)ctx, mats, n_segments, n_cols, log_n, rate_bits, grouped, form, prefix_mask, digests_out);
}
int starkhip_leaf_prefix_table(void* ctx, unsigned log_n, unsigned rate_bits, uint64_t* cap_out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return leaf_prefix_table((Ctx*)ctx, log_n, rate_bits, cap_out);
}
int starkhip_field_ops_batch(void* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return field_ops((Ctx*)ctx, op, a, b, out, n);
}
int starkhip_selfcheck_hash_tables(unsigned n_states) {
    const int fours = merged_fours_selfcheck(n_states);   // the lane and pair forms' tables (poseidon_host.cpp)
    if (fours < 0) return -1;
    return quad_merged_tables_selfcheck(n_states) + fours;
}
size_t starkhip_hash_table_image(int form, void* out, size_t cap) {
    const void* image = nullptr;
    size_t bytes = 0;
    switch (form) {
        case FORM_QUAD: image = quad_merged_tables_host(); bytes = sizeof(QuadMergedTables); break;
        case FORM_ROW: image = row_merged_tables_host(); bytes = sizeof(RowMergedTables); break;
        case FORM_LANE: image = lane_tables_host(); bytes = sizeof(LaneTables); break;
        case FORM_PAIR: image = pair_tables_host(); bytes = sizeof(PairTables); break;
    }
    if (!image) return 0;
    if (out && cap >= bytes) memcpy(out, image, bytes);
    return bytes;
}
int starkhip_fri_geometry(const starkhip_config_t* cfg, unsigned log_n, unsigned* arities_out, size_t cap, size_t* n_layers, size_t* final_poly_len) {
    if (!cfg) return STARKHIP_ERR_BAD_SHAPE;
    FriGeometry g;
    if (!FriGeometry::make(*cfg, log_n, &g)) return STARKHIP_ERR_BAD_SHAPE;
    for (size_t l = 0; l < g.arities.size() && l < cap; l++) arities_out[l] = g.arities[l];
    if (n_layers) *n_layers = g.arities.size();
    if (final_poly_len) *final_poly_len = g.final_poly_len;
    return STARKHIP_OK;
}

size_t starkhip_lde_launch_ranges(size_t n_cols, unsigned rate_bits, uint64_t* triples, size_t cap) {
    const std::vector<LdeLaunch> plan = lde_launch_plan(n_cols, rate_bits);
    for (size_t i = 0; i < plan.size() && i < cap; i++) {
        triples[3 * i] = plan[i].a;
        triples[3 * i + 1] = plan[i].b;
        triples[3 * i + 2] = plan[i].from_copy ? 1 : 0;
    }
    return plan.size();
}
void starkhip_poseidon_permute_host(uint64_t state[12]) { poseidon_permute_host(state); }

/* --- the Keccak hasher's test entries (keccak.h) */
void starkhip_keccak256(const uint8_t* bytes, size_t len, uint8_t out32[32]) { keccak256_host(bytes, len, out32); }
void starkhip_keccak_permute_host(uint64_t state12[12]) { keccak_permute_host(state12); }
int starkhip_keccak_state_from_words(const uint64_t* words, size_t n, uint64_t state12[12]) {
    if (!words || !state12) return -1;
    int used = 0;
    const int have = keccak_take_words(words, (int)std::min<size_t>(n, 1u << 20), state12, 0, &used);
    return have == 12 ? used : -1;
}
int starkhip_keccak_permute_batch(void* ctx, uint64_t* states, size_t n) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return keccak_permute_batch((Ctx*)ctx, states, n);
}
int starkhip_merkle_tree_hasher(void* ctx, int hasher, const uint64_t* lde_colmajor, size_t n_cols, unsigned log_N, unsigned cap_height,
                                uint64_t* digests_out, uint64_t* cap_out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return merkle_tree_hasher((Ctx*)ctx, hasher, lde_colmajor, n_cols, log_N, cap_height, digests_out, cap_out);
}
int starkhip_hash_rows_hasher(void* ctx, int hasher, const uint64_t* rows, size_t width, size_t n_leaves, uint64_t* digests_out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    return hash_rows_hasher((Ctx*)ctx, hasher, rows, width, n_leaves, digests_out);
}
int starkhip_proof_hasher(const uint64_t* proof, size_t proof_words) {
    ProofLayout pl;
    if (!proof || !pl.read_header(proof, proof_words)) return STARKHIP_ERR_BAD_SHAPE;
    return (int)pl.hasher;
}
/* n chained permutations with the challenger's host permutation (which = 0) or the portable reference loop (which = 1);
 * lets the tests compare the two and the benchmark report the host hashing rate */
void starkhip_poseidon_permute_host_many(uint64_t state[12], size_t n, int which) {
    for (size_t i = 0; i < n; i++) {
        if (which == 0) poseidon_permute_host(state);
        else poseidon_permute(state);
    }
}

int starkhip_verify(starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* proof, size_t proof_words) {
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    return verify_proof(*a, *cfg, proof, proof_words);
}

int starkhip_verify_batch(void* ctx, size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                          const size_t* proof_words, int* results) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    try {
        return verify_batch_device((Ctx*)ctx, n, airs, cfgs, proofs, proof_words, results);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}

int starkhip_last_verify_timings(void* ctx, double out[4]) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    if (!out) return STARKHIP_ERR_BAD_SHAPE;
    memcpy(out, ctx_verify_timings((Ctx*)ctx), 4 * sizeof(double));
    return STARKHIP_OK;
}

int starkhip_verify_batch_replay(size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                                 const size_t* proof_words, int* results) {
    try {
        return verify_batch_replay(n, airs, cfgs, proofs, proof_words, results);
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    }
}

void starkhip_proof_blob_stats(uint64_t out[5]) {
    const starkhip::BlobArenaStats st = starkhip::blob_arena_stats();
    out[0] = st.blobs; out[1] = st.busy; out[2] = st.bytes; out[3] = st.taken; out[4] = st.missed;
}
void starkhip_free(void* p) { starkhip::blob_free(p); }  // a proof blob may be a recycled page-locked one (blob_arena.h)

const char* starkhip_error_string(int code) {
    switch (code) {
        case STARKHIP_OK: return "ok";
        case STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE: return "Quotient has failed, the vanishing polynomial is not divisible by Z_H";
        case STARKHIP_ERR_ZETA_IN_SUBGROUP: return "Opening point is in the subgroup";
        case STARKHIP_ERR_BAD_SHAPE: return "bad shape (columns / public inputs / rows / config do not match the AIR)";
        case STARKHIP_ERR_HIP: return "HIP runtime error";
        case STARKHIP_ERR_OOM: return "out of device memory";
        case STARKHIP_ERR_NO_DEVICE: return "no such HIP device / context";
        case STARKHIP_ERR_VERIFY: return "proof rejected";
        case STARKHIP_ERR_BAD_AIR: return "unknown or unbuildable AIR id";
        case STARKHIP_ERR_TRACE: return "the trace violates the AIR (\"check_trace\": a check blob is returned instead of a proof) or a lookup of it fails (\"fill_lookups\": a lookup blob; \"fill_frequencies\": a LogUp blob)";
        default: return "unknown error";
    }
}

}  // extern "C"
