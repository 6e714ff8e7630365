// Systems of tables tied by cross-table lookups (COMPAT.md 2d): the registry, the system prover above the two halves of
// prove() (prover.h) and the starkhip_system_* / starkhip_ctl_* entries of the C ABI.
#include <string.h>

#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "air_eval.h"
#include "air_validate.h"
#include "airs.h"
#include "blob_arena.h"
#include "ctl.h"
#include "kernels_permutation.h"
#include "logup.h"
#include "poseidon.h"
#include "proof.h"
#include "prover.h"
#include "system.h"
#include "trace_input.h"
#include "verifier.h"

namespace starkhip {

namespace {
std::mutex g_sys_mu;
std::vector<std::unique_ptr<SystemInfo>>& registry() {
    static std::vector<std::unique_ptr<SystemInfo>> r;
    return r;
}
const AirProgram* program_of(int id) {
    const AirInfo* a = id >= STARKHIP_AIR_CUSTOM_BASE ? air_get(id) : nullptr;  // tables are registered AIRs
    return a ? &a->prog : nullptr;
}
void copy_why(const std::string& msg, char* why, size_t why_len) {
    if (!why || !why_len) return;
    const size_t n = std::min(msg.size(), why_len - 1);
    memcpy(why, msg.data(), n);
    why[n] = 0;
}
template <class F>
int guarded_sys(F call) {
    try {
        return call();
    } catch (const std::bad_alloc&) {
        return STARKHIP_ERR_OOM;
    } catch (const std::exception&) {
        return STARKHIP_ERR_BAD_SHAPE;
    }
}
}  // namespace

const SystemInfo* system_get(int id) {
    std::lock_guard<std::mutex> lk(g_sys_mu);
    return id >= 0 && (size_t)id < registry().size() ? registry()[id].get() : nullptr;
}

// A system prover: one context per table on one device
struct SystemHandle {
    const SystemInfo* sys;
    std::vector<Ctx*> ctxs;
    ~SystemHandle() {
        for (Ctx* c : ctxs) ctx_destroy(c);
    }
};

// C1 - C3 and the one deviation: every table's first half, the system transcript over the trace caps, every table's CTL polynomials and
// sums, the balances -- a refusal names the CTL and commits nothing auxiliary --, then every second half from a copy of the transcript
static int system_prove(SystemHandle* h, const starkhip_config_t* cfgs, const std::vector<TraceInput>& ins, const uint64_t* const* pis, const size_t* n_pis, uint64_t pow_witness,
                        uint64_t** proof, size_t* proof_words, int* failing_ctl) {
    const SystemInfo& S = *h->sys;
    const size_t T = S.prog.airs.size();
    struct Jobs {
        std::vector<ProveJob*> j;
        std::vector<uint64_t*> blobs;
        ~Jobs() {
            for (ProveJob* x : j) prove_job_free(x);
            for (uint64_t* b : blobs) blob_free(b);
        }
    } jobs;
    jobs.j.assign(T, nullptr);
    jobs.blobs.assign(T, nullptr);
    std::vector<size_t> blob_words(T, 0);
    for (size_t t = 0; t < T; t++) {
        const AirInfo* a = air_get(S.prog.airs[t]);
        if (!a) return STARKHIP_ERR_BAD_AIR;
        uint64_t* refused = nullptr;
        size_t refused_words = 0;
        if (int rc = prove_first_half(h->ctxs[t], *a, cfgs[t], ins[t], pis[t], n_pis[t], pow_witness, &S.tables[t], &jobs.j[t], &refused, &refused_words)) {
            blob_free(refused);  // (a trace a context's "check_trace" refused: the system entry hands out no check blob)
            return rc;
        }
    }
    Challenger ch(prove_job_hasher(jobs.j[0]));  // every table under the same hasher (starkhip_system_set_option sets all the contexts)
    for (size_t t = 0; t < T; t++) {
        const uint64_t* cap = nullptr;
        size_t cap_words = 0;
        if (prove_job_hasher(jobs.j[t]) != ch.hasher) return STARKHIP_ERR_BAD_SHAPE;
        if (int rc = prove_trace_cap(jobs.j[t], &cap, &cap_words)) return rc;
        ch.observe_many(cap, cap_words);
    }
    gl_t chal[4];
    for (gl_t& x : chal) x = ch.get();
    std::vector<std::vector<gl_t>> sums_of(T);
    int bad = -1;  // the first CTL that does not balance or has an endpoint with a zero denominator
    for (size_t t = 0; t < T; t++) {
        const std::vector<CtlEndpoint>& eps = S.tables[t].eps;
        sums_of[t].assign(2 * eps.size(), 0);
        std::vector<uint64_t> zeros(eps.size() + 1, 0);
        if (int rc = prove_ctl_polys(jobs.j[t], chal, sums_of[t].data(), zeros.data())) return rc;
        for (size_t e = 0; e < eps.size(); e++)
            if (zeros[e] && (bad < 0 || (int)eps[e].ctl < bad)) bad = (int)eps[e].ctl;
    }
    const int unbalanced = ctl_first_unbalanced(S.prog, sums_of);
    if (unbalanced >= 0 && (bad < 0 || unbalanced < bad)) bad = unbalanced;
    if (bad >= 0) {
        if (failing_ctl) *failing_ctl = bad;
        return STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE;
    }
    for (size_t t = 0; t < T; t++) {
        ProveJob* j = jobs.j[t];
        jobs.j[t] = nullptr;  // the second half spends the job
        if (int rc = prove_second_half(j, &ch, &jobs.blobs[t], &blob_words[t])) {
            if (rc == STARKHIP_ERR_TRACE) {
                blob_free(jobs.blobs[t]);
                jobs.blobs[t] = nullptr;
            }
            return rc;
        }
    }
    size_t total = 3 + T;
    for (size_t t = 0; t < T; t++) total += blob_words[t];
    uint64_t* out = blob_alloc(total * 8);
    if (!out) return STARKHIP_ERR_OOM;
    out[0] = STARKHIP_SYSTEM_PROOF_MAGIC;
    out[1] = T;
    size_t at = 3 + T;
    for (size_t t = 0; t < T; t++) {
        out[2 + t] = at;
        memcpy(out + at, jobs.blobs[t], blob_words[t] * 8);
        at += blob_words[t];
    }
    out[2 + T] = at;
    *proof = out;
    *proof_words = total;
    return STARKHIP_OK;
}

}  // namespace starkhip

using namespace starkhip;

extern "C" {

int starkhip_system_check(const uint64_t* blob, size_t words, char* why, size_t why_len) {
    std::string msg;
    const int rc = guarded_sys([&] { return system_parse_checked(blob, words, program_of, nullptr, &msg) ? (int)STARKHIP_OK : (int)STARKHIP_ERR_BAD_AIR; });
    copy_why(msg, why, why_len);
    return rc;
}

int starkhip_system_register(const uint64_t* blob, size_t words, starkhip_system_t* id_out) {
    if (!id_out) return STARKHIP_ERR_BAD_SHAPE;
    return guarded_sys([&] {
        std::unique_ptr<SystemInfo> info(new SystemInfo());
        if (!system_parse_checked(blob, words, program_of, &info->prog, nullptr)) return (int)STARKHIP_ERR_BAD_AIR;
        info->blob.assign(blob, blob + words);
        for (size_t t = 0; t < info->prog.airs.size(); t++) info->tables.push_back(info->prog.table((uint32_t)t));
        std::lock_guard<std::mutex> lk(g_sys_mu);
        for (const auto& s : registry())
            if (s->blob == info->blob) {
                *id_out = s->id;
                return (int)STARKHIP_OK;
            }
        if (registry().size() >= STARKHIP_SYSTEM_CAPACITY) return (int)STARKHIP_ERR_BAD_AIR;
        info->id = (int)registry().size();
        *id_out = info->id;
        registry().push_back(std::move(info));
        return (int)STARKHIP_OK;
    });
}

int starkhip_system_tables(starkhip_system_t sys) { const SystemInfo* s = system_get(sys); return s ? (int)s->prog.airs.size() : STARKHIP_ERR_BAD_AIR; }
int starkhip_system_ctls(starkhip_system_t sys) { const SystemInfo* s = system_get(sys); return s ? (int)s->prog.ctls.size() : STARKHIP_ERR_BAD_AIR; }
int starkhip_system_table_air(starkhip_system_t sys, size_t table) {
    const SystemInfo* s = system_get(sys);
    if (!s) return STARKHIP_ERR_BAD_AIR;
    return table < s->prog.airs.size() ? s->prog.airs[table] : STARKHIP_ERR_BAD_SHAPE;
}
int starkhip_system_table_endpoints(starkhip_system_t sys, size_t table) {
    const SystemInfo* s = system_get(sys);
    if (!s) return STARKHIP_ERR_BAD_AIR;
    return table < s->tables.size() ? (int)s->tables[table].eps.size() : STARKHIP_ERR_BAD_SHAPE;
}

int starkhip_system_create(int device, starkhip_system_t sys, void** handle) {
    if (!handle) return STARKHIP_ERR_BAD_SHAPE;
    *handle = nullptr;
    const SystemInfo* s = system_get(sys);
    if (!s) return STARKHIP_ERR_BAD_AIR;
    return guarded_sys([&] {
        std::unique_ptr<SystemHandle> h(new SystemHandle{s, {}});
        for (size_t t = 0; t < s->prog.airs.size(); t++) {
            Ctx* c = nullptr;
            if (int rc = ctx_create(device, &c)) return rc;
            h->ctxs.push_back(c);
        }
        *handle = h.release();
        return (int)STARKHIP_OK;
    });
}
void starkhip_system_destroy(void* handle) { delete (SystemHandle*)handle; }
int starkhip_system_set_option(void* handle, const char* name, long value) {
    if (!handle) return STARKHIP_ERR_NO_DEVICE;
    for (Ctx* c : ((SystemHandle*)handle)->ctxs)
        if (int rc = ctx_set_option(c, name, value)) return rc;
    return STARKHIP_OK;
}

unsigned starkhip_ctl_span_rows(void) { return PERM_SPAN_ROWS; }

int starkhip_system_last_timings(void* handle, size_t table, float out_ms[STARKHIP_N_PHASES]) {
    if (!handle) return STARKHIP_ERR_NO_DEVICE;
    SystemHandle* h = (SystemHandle*)handle;
    if (table >= h->ctxs.size() || !out_ms) return STARKHIP_ERR_BAD_SHAPE;
    memcpy(out_ms, ctx_timings(h->ctxs[table]), STARKHIP_N_PHASES * sizeof(float));
    return STARKHIP_OK;
}

int starkhip_system_prove(void* handle, const starkhip_config_t* cfgs, const uint64_t* const* traces, const size_t* n_rows, const int* layouts, const int* on_device,
                          const uint64_t* const* public_inputs, const size_t* n_pis, uint64_t pow_witness, uint64_t** proof, size_t* proof_words, int* failing_ctl) {
    if (!handle) return STARKHIP_ERR_NO_DEVICE;
    SystemHandle* h = (SystemHandle*)handle;
    const size_t T = h->sys->prog.airs.size();
    if (failing_ctl) *failing_ctl = -1;
    if (!traces || !n_rows || !layouts || !public_inputs || !n_pis || !proof || !proof_words || !system_configs_ok(cfgs, T)) return STARKHIP_ERR_BAD_SHAPE;
    return guarded_sys([&] {
        std::vector<TraceInput> ins;
        for (size_t t = 0; t < T; t++) {
            const AirInfo* a = air_get(h->sys->prog.airs[t]);
            if (!a) return (int)STARKHIP_ERR_BAD_AIR;
            ins.push_back(TraceInput::dense(traces[t], n_rows[t], a->cols, layouts[t], on_device ? on_device[t] : 0));
            if (ins.back().check(*a) || (n_pis[t] && !public_inputs[t])) return (int)STARKHIP_ERR_BAD_SHAPE;
        }
        return system_prove(h, cfgs, ins, public_inputs, n_pis, pow_witness, proof, proof_words, failing_ctl);
    });
}

int starkhip_system_verify(starkhip_system_t sys, const starkhip_config_t* cfgs, const uint64_t* proof, size_t proof_words) {
    const SystemInfo* s = system_get(sys);
    if (!s) return STARKHIP_ERR_BAD_AIR;
    return guarded_sys([&] { return verify_system_proof(s->prog, cfgs, proof, proof_words); });
}

int starkhip_system_proof_layout(const uint64_t* proof, size_t proof_words, size_t* n_tables, size_t* offsets, size_t cap) {
    return guarded_sys([&] {
        std::vector<size_t> off;
        if (!n_tables || !offsets || !system_proof_offsets(proof, proof_words, &off) || off.size() > cap) return (int)STARKHIP_ERR_BAD_SHAPE;
        *n_tables = off.size() - 1;
        std::copy(off.begin(), off.end(), offsets);
        return (int)STARKHIP_OK;
    });
}

// what the two polys entries refuse
static int ctl_polys_args(const SystemInfo* s, size_t table, const TraceInput& in, const uint64_t* challenges, const uint64_t* polys_out, const uint64_t* sums_out,
                          const uint64_t* zeros_out) {
    if (!s || table >= s->tables.size() || s->tables[table].eps.empty()) return STARKHIP_ERR_BAD_AIR;
    const AirInfo* a = air_get(s->prog.airs[table]);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    if (in.check(*a) || !challenges || !polys_out || !sums_out || !zeros_out || in.n_rows < 2 || in.n_rows > ((size_t)1 << STARKHIP_MAX_LOG_ROWS) || (in.n_rows & (in.n_rows - 1)))
        return STARKHIP_ERR_BAD_SHAPE;
    for (int i = 0; i < 4; i++)
        if (challenges[i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    return STARKHIP_OK;
}

int starkhip_ctl_polys(void* ctx, starkhip_system_t sys, size_t table, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                       const uint64_t* challenges, uint64_t* polys_out, uint64_t* sums_out, uint64_t* zero_denominators_out) {
    if (!ctx) return STARKHIP_ERR_NO_DEVICE;
    const SystemInfo* s = system_get(sys);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, on_device);
    if (int rc = ctl_polys_args(s, table, in, challenges, polys_out, sums_out, zero_denominators_out)) return rc;
    return guarded_sys([&] { return ctl_polys((Ctx*)ctx, s->tables[table], in, challenges, polys_out, sums_out, zero_denominators_out); });
}

int starkhip_ctl_polys_replay(starkhip_system_t sys, size_t table, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, const uint64_t* challenges,
                              uint64_t* polys_out, uint64_t* sums_out, uint64_t* zero_denominators_out) {
    const SystemInfo* s = system_get(sys);
    const TraceInput in = TraceInput::dense(trace, n_rows, n_cols, layout, 0);
    if (int rc = ctl_polys_args(s, table, in, challenges, polys_out, sums_out, zero_denominators_out)) return rc;
    return guarded_sys([&] {
        const bool col_major = in.form == TraceForm::ColMajor;
        ctl_polys_host(s->tables[table], n_rows, [&](uint32_t col, size_t row) { return col_major ? trace[(size_t)col * n_rows + row] : trace[row * n_cols + col]; }, challenges,
                       polys_out, sums_out, zero_denominators_out);
        return (int)STARKHIP_OK;
    });
}

int starkhip_system_eval_frame_ctl(starkhip_system_t sys, size_t table, const uint64_t* local, const uint64_t* next, const uint64_t* public_inputs, const uint64_t masks[8],
                                   const uint64_t* alphas, int n_alpha, const uint64_t* aux, const uint64_t* aux_next, const uint64_t* logup_challenges,
                                   const uint64_t* ctl_challenges, const uint64_t* sums, uint64_t* acc_out) {
    const SystemInfo* s = system_get(sys);
    if (!s || table >= s->tables.size()) return STARKHIP_ERR_BAD_AIR;
    const int air = s->prog.airs[table];
    const AirInfo* a = air_get(air);
    if (!a) return STARKHIP_ERR_BAD_AIR;
    const CtlTable& T = s->tables[table];
    const size_t nA = a->prog.logup_polys(), nC = T.polys();
    // the AIR's own constraints and its LogUp ones (the first nA of aux), then the table's CTL constraints over the nC behind them
    const int rc = starkhip_air_eval_frame_logup((starkhip_air_t)air, local, next, public_inputs, masks, alphas, n_alpha, aux, aux_next, logup_challenges, acc_out);
    if (rc != STARKHIP_OK || !nC) return rc;
    if (!aux || !aux_next || !ctl_challenges || !sums) return STARKHIP_ERR_BAD_SHAPE;
    for (size_t i = 0; i < 4; i++)
        if (ctl_challenges[i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    for (size_t i = 0; i < nC / 2; i++)
        if (sums[i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    return guarded_sys([&] {
        std::vector<gl2_t> l(a->cols), nx(a->cols), x(nC), xn(nC), al(n_alpha), acc(n_alpha);
        for (size_t i = 0; i < a->cols; i++) {
            l[i] = gl2_make(local[2 * i], local[2 * i + 1]);
            nx[i] = gl2_make(next[2 * i], next[2 * i + 1]);
        }
        for (size_t i = 0; i < nC; i++) {
            x[i] = ExtOps::canon(gl2_make(aux[2 * (nA + i)], aux[2 * (nA + i) + 1]));
            xn[i] = ExtOps::canon(gl2_make(aux_next[2 * (nA + i)], aux_next[2 * (nA + i) + 1]));
        }
        gl2_t mk[4];
        for (int i = 0; i < 4; i++) mk[i] = gl2_make(masks[2 * i], masks[2 * i + 1]);
        for (int j = 0; j < n_alpha; j++) {
            al[j] = gl2_make(alphas[2 * j], alphas[2 * j + 1]);
            acc[j] = gl2_make(acc_out[2 * j], acc_out[2 * j + 1]);
        }
        ctl_eval_folded<ExtOps>(T, l.data(), nx.data(), x.data(), xn.data(), ctl_challenges, sums, mk, al.data(), n_alpha, acc.data());
        for (int j = 0; j < n_alpha; j++) {
            acc_out[2 * j] = acc[j].a0;
            acc_out[2 * j + 1] = acc[j].a1;
        }
        return (int)STARKHIP_OK;
    });
}

}  // extern "C"
