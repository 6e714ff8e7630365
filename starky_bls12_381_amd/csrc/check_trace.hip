// Host halves of the trace checkers: starkhip_check_trace, starkhip_check_trace_report (under check_report.h; kernels_check.hip),
// starkhip_check_trace_free_cell_classes with starkhip_check_trace_free_cells, one run and a projection of it (free_cells.h;
// kernels_free_classes.hip), and the check prove() runs on its own copy of the trace ("check_trace": check_trace_in_prove).  The check
// of the permutation pairs is not here: permutation_check.hip.  What the stand-alone ones share is check_trace_prepare: the shape
// checks, the cached op stream of the AIR (check_program, Ctx::CheckProgram), the trace and the public inputs on the device -- the
// CheckView the kernels read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "air_validate.h"
#include "check_report.h"
#include "ctx.h"
#include "free_cells.h"
#include "quotient_ops.h"

namespace starkhip {

// The op stream of `air` for a trace of n_rows, compiled and uploaded once and cached per context like the quotient's (Ctx::CheckProgram),
// and the part of the view that comes from it.  It allocates only the program's own buffers: prove() calls it with a trace parked in the
// LDE buffer.  A device allocation all the same, so the first check of an AIR on a context waits for every stream of the device.
static int check_program(Ctx* c, const AirInfo& air, size_t n, CheckView* V) {
    const AirProgram& P = air.prog;
    hipStream_t st = c->st;
    // (n / 64) x chunks waves: enough to fill 256 CUs several times over, at most one chunk per group
    const size_t blocks = (n + 63) / 64;
    const unsigned want = (unsigned)std::min<size_t>({1024, P.group_off.size(), std::max<size_t>(1, (32768 + blocks - 1) / blocks)});
    if (c->chk.air != air.id || c->chk.want != want) {
        c->chk.air = -1;
        const QProgram Q = compile_quotient_ops(P, want);
        const size_t nc = Q.chunk_k_after.size();
        std::vector<uint32_t> meta(2 * nc + 1);  // chunk_op[nc + 1], chunk_k0[nc]
        for (size_t j = 0; j <= nc; j++) meta[j] = Q.chunk_batch[j] * QOP_BATCH;
        for (size_t j = 0; j < nc; j++) meta[nc + 1 + j] = j ? P.n_constraints - Q.chunk_k_after[j - 1] : 0;
        HIPCHK(c->chk.ops.ensure(Q.ops.size() * sizeof(QOp)));
        HIPCHK(c->chk.meta.ensure(meta.size() * 4));
        HIPCHK(hipMemcpyAsync(c->chk.ops.p, Q.ops.data(), Q.ops.size() * sizeof(QOp), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c->chk.meta.p, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(stream_wait(c));  // Q and meta go out of scope
        c->chk.k0.assign(meta.begin() + nc + 1, meta.end());
        c->chk.k0.push_back(P.n_constraints);
        c->chk.air = air.id;
        c->chk.want = want;
        c->chk.chunks = (unsigned)nc;
    }
    HIPCHK(c->chk.out.ensure(2 * sizeof(unsigned long long)));
    V->ops = c->chk.ops.as<QOp>();
    V->n_chunks = c->chk.chunks;
    V->chunk_op = c->chk.meta.as<uint32_t>();  // chunk_op[n_chunks + 1], chunk_k0[n_chunks]
    V->chunk_k0 = V->chunk_op + V->n_chunks + 1;
    return STARKHIP_OK;
}

// What the stand-alone checkers do before their kernels: the shape checks, the op stream of `air` (check_program), then the trace where
// prove() would put it -- column-major in `values`, or the caller's own device memory, with the LDE buffer as the upload staging of
// row-major host rows -- and the public inputs in c->pis; *V is what the kernels read of it.
static int check_trace_prepare(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, CheckView* V) {
    const AirProgram& P = air.prog;
    if (int rc = check_trace_shape(air, in.n_rows, pis, &V->log_n)) return rc;
    const size_t n = in.n_rows, C = P.n_cols;
    if (in.n_cols != C) return STARKHIP_ERR_BAD_SHAPE;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->st;
    if (int rc = check_program(c, air, n, V)) return rc;
    if (!in.callers_columns()) HIPCHK(c->values.ensure(C * n * 8));
    if (in.park_words(C)) HIPCHK(c->lde.ensure(in.park_words(C) * 8));  // the staging of row-major host rows
    if (int rc = upload_dense(c, in, c->values.as<gl_t>(), &V->trace)) return rc;
    HIPCHK(c->pis.ensure(std::max<size_t>(1, P.n_pis) * 8));
    if (P.n_pis) HIPCHK(hipMemcpyAsync(c->pis.p, pis, P.n_pis * 8, hipMemcpyHostToDevice, st));
    V->pis = c->pis.as<gl_t>();
    return STARKHIP_OK;
}

// the plain check over a view: res = {violations, (constraint << 32 | row) of the lowest violated constraint on its lowest row}, after
// the next stream_wait
static int enqueue_check(Ctx* c, const CheckView& V, unsigned long long res[2]) {
    hipStream_t st = c->st;
    const unsigned long long init[2] = {0, ~0ull};
    HIPCHK(hipMemcpyAsync(c->chk.out.p, init, sizeof init, hipMemcpyHostToDevice, st));
    HIPCHK(launch_check_trace(V, c->chk.out.as<unsigned long long>(), st));
    HIPCHK(read_back(c, res, c->chk.out.p, 2 * sizeof(unsigned long long), st));
    return STARKHIP_OK;
}

int check_trace(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t* violations, uint64_t first[3]) {
    const AirProgram& P = air.prog;
    CheckView V = {};
    if (int rc = check_trace_prepare(c, air, in, pis, &V)) return rc;
    const gl_t* d_trace = V.trace;
    const size_t n = in.n_rows, C = P.n_cols;
    hipStream_t st = c->st;
    unsigned long long res[2];
    if (int rc = enqueue_check(c, V, res)) return rc;
    HIPCHK(stream_wait(c));
    *violations = res[0];
    first[0] = first[1] = first[2] = 0;
    if (!res[0]) return STARKHIP_OK;
    // the value of the first violation, from its frame: rows r and r + 1 (mod n) of every column
    const uint32_t k = (uint32_t)(res[1] >> 32), r = (uint32_t)res[1];
    std::vector<gl_t> frame(2 * C);
    HIPCHK(hipMemcpy2DAsync(frame.data(), 8, d_trace + r, n * 8, 8, C, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpy2DAsync(frame.data() + C, 8, d_trace + ((r + 1) & (n - 1)), n * 8, 8, C, hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(c));
    first[0] = k;
    first[1] = r;
    first[2] = air_constraint_value(P, k, frame.data(), frame.data() + C, pis);
    return STARKHIP_OK;
}

// starkhip_check_trace_report: the two report passes of kernels_check.hip under the host half of check_report.h.  chk.rep holds
// counts[K] (the cursors of the second pass), row_mask[W], base[K] and the launched chunks[nc]; chk.list the entries.
namespace {
struct DevicePasses : CheckPasses {
    Ctx* c;
    const AirProgram& P;
    const CheckView& V;
    size_t K, W, off_mask, off_base, off_chunks;
    DevicePasses(Ctx* c_, const AirProgram& P_, const CheckView& V_) : c(c_), P(P_), V(V_) {
        K = P.n_constraints;
        W = (((size_t)1 << V.log_n) + 63) / 64;
        off_mask = (K * 4 + 7) / 8 * 8;
        off_base = off_mask + W * 8;
        off_chunks = off_base + K * 4;
    }
    uint32_t* d_counts() const { return c->chk.rep.as<uint32_t>(); }
    unsigned long long* d_mask() const { return (unsigned long long*)((char*)c->chk.rep.p + off_mask); }
    int count(uint32_t* counts, uint64_t* mask) override {
        HIPCHK(c->chk.rep.ensure(off_chunks + (size_t)V.n_chunks * 4));
        HIPCHK(hipMemsetAsync(c->chk.rep.p, 0, off_base, c->st));
        HIPCHK(launch_check_report_count(V, d_counts(), d_mask(), c->st));
        HIPCHK(hipMemcpyAsync(mask, d_mask(), W * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipMemcpyAsync(counts, d_counts(), K * 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(stream_wait(c));
        return STARKHIP_OK;
    }
    int list(const uint32_t* base, const uint64_t*, size_t total, uint64_t* entries) override {
        std::vector<uint32_t> chunks;  // those with a listed constraint
        for (unsigned j = 0; j < V.n_chunks; j++)
            for (uint32_t k = c->chk.k0[j]; k < c->chk.k0[j + 1]; k++)
                if (base[k] != ~0u) {
                    chunks.push_back(j);
                    break;
                }
        if (chunks.empty() || total > 0xFFFFFFFFull / 2) return STARKHIP_ERR_HIP;
        HIPCHK(c->chk.list.ensure(total * 24));
        char* rep = (char*)c->chk.rep.p;
        HIPCHK(hipMemsetAsync(rep, 0, K * 4, c->st));  // the counts become the cursors
        HIPCHK(hipMemcpyAsync(rep + off_base, base, K * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemcpyAsync(rep + off_chunks, chunks.data(), chunks.size() * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemsetAsync(c->chk.list.p, 0xFF, total * 24, c->st));  // an entry nobody wrote fails the host's check of its segment
        HIPCHK(launch_check_report_list(V, (const uint32_t*)(rep + off_chunks), (unsigned)chunks.size(), d_counts(), d_mask(),
                                        (const uint32_t*)(rep + off_base), c->chk.list.as<unsigned long long>(), (uint32_t)total, c->st));
        HIPCHK(hipMemcpyAsync(entries, c->chk.list.p, total * 24, hipMemcpyDeviceToHost, c->st));
        HIPCHK(stream_wait(c));  // `chunks` goes out of scope
        return STARKHIP_OK;
    }
};
}  // namespace

int check_trace_report(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint32_t* per_constraint, uint64_t* row_mask,
                       uint64_t* list, size_t cap, starkhip_check_report_t* out) {
    CheckView V = {};
    if (int rc = check_trace_prepare(c, air, in, pis, &V)) return rc;
    DevicePasses passes(c, air.prog, V);
    return check_report_run(air.prog, in.n_rows, passes, per_constraint, row_mask, list, cap, out);
}

// "check_trace" inside prove(): the trace is where phase 0 left it (`d_trace`, column-major: parked in the LDE buffer, in `values`, or
// the caller's own memory), c->pis is allocated, and nothing here touches `values` or `lde`.  The plain kernel with its 16-byte
// read-back decides; only a violated trace pays for the report's two passes, whose summary and first `cap` entries make the check
// blob (check_report.h).  STARKHIP_OK, or STARKHIP_ERR_TRACE with *blob.
int check_trace_in_prove(Ctx* c, const AirInfo& air, const gl_t* d_trace, size_t n_rows, const uint64_t* pis, uint64_t** blob, size_t* words) {
    const AirProgram& P = air.prog;
    CheckView V = {};
    if (!log2_rows(n_rows, &V.log_n)) return STARKHIP_ERR_BAD_SHAPE;
    if (int rc = check_program(c, air, n_rows, &V)) return rc;
    if (P.n_pis) HIPCHK(hipMemcpyAsync(c->pis.p, pis, P.n_pis * 8, hipMemcpyHostToDevice, c->st));
    V.trace = d_trace;
    V.pis = c->pis.as<gl_t>();
    unsigned long long res[2] = {0, 0};
    if (int rc = enqueue_check(c, V, res)) return rc;
    HIPCHK(stream_wait(c));
    c->traces_checked++;
    if (!res[0]) return STARKHIP_OK;
    c->traces_rejected++;
    const size_t cap = (size_t)c->opt_check_trace_list;
    std::vector<uint64_t> list(3 * std::max<size_t>(1, std::min<size_t>(cap, res[0])));
    starkhip_check_report_t rep = {0, 0, 0, 0};
    DevicePasses passes(c, P, V);
    if (int rc = check_report_run(P, n_rows, passes, nullptr, nullptr, list.data(), cap, &rep)) return rc;
    if (rep.violations != res[0]) return STARKHIP_ERR_HIP;  // the two kernels walk one op stream over one trace
    *blob = check_blob_make(air.id, n_rows, rep, list.data(), words);
    return *blob ? STARKHIP_ERR_TRACE : STARKHIP_ERR_OOM;
}

// What the two free-cell entries walk: compile_free_cells of the op stream check_trace_prepare cached for `air`, on the device, cached
// in c->free_chk.  Op indices of that stream: the same cut gives the same ones.
static int free_cells_program(Ctx* c, const AirInfo& air) {
    const AirProgram& P = air.prog;
    hipStream_t st = c->st;
    Ctx::FreeCellsProgram& fc = c->free_chk;
    if (fc.air == air.id && fc.want == c->chk.want) return STARKHIP_OK;
    fc.air = -1;
    const FreeProgram F = compile_free_cells(compile_quotient_ops(P, c->chk.want));
    if (F.cons.size() != P.n_constraints) return STARKHIP_ERR_HIP;
    HIPCHK(fc.cons.ensure(F.cons.size() * sizeof(FreeCon)));
    HIPCHK(fc.pivots.ensure(std::max<size_t>(1, F.pivots.size()) * 4));
    HIPCHK(hipMemcpyAsync(fc.cons.p, F.cons.data(), F.cons.size() * sizeof(FreeCon), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(fc.pivots.p, F.pivots.data(), F.pivots.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(stream_wait(c));  // F goes out of scope
    fc.air = air.id;
    fc.want = c->chk.want;
    return STARKHIP_OK;
}

// What both free-cell entries do on the device: the kernel of kernels_free_classes.hip over the view the checkers share, then the count
// per column.  One launch each: a FinalExp run stays far below a second.  `counts` comes back as per_column [C][3]
// followed by open_rows [K]; of the planes, what the caller asks for comes back into `planes_out`: all three, the caught one, or none.
enum class FreePlanes { NONE, CAUGHT, ALL };
static int free_cell_classes_run(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, FreePlanes planes,
                                 uint64_t* planes_out, std::vector<uint32_t>* counts) {
    const AirProgram& P = air.prog;
    if (free_cells_bad_delta(delta)) return STARKHIP_ERR_BAD_SHAPE;
    CheckView V = {};
    if (int rc = check_trace_prepare(c, air, in, pis, &V)) return rc;
    const size_t n = in.n_rows, C = P.n_cols, W = (n + 63) / 64, K = P.n_constraints;
    hipStream_t st = c->st;
    Ctx::FreeCellsProgram& fc = c->free_chk;
    if (int rc = free_cells_program(c, air)) return rc;
    HIPCHK(fc.planes.ensure(3 * C * W * 8));
    HIPCHK(fc.class_counts.ensure((3 * C + K) * 4));
    unsigned long long* d_planes = fc.planes.as<unsigned long long>();
    uint32_t* d_per = fc.class_counts.as<uint32_t>();
    uint32_t* d_open = d_per + 3 * C;
    HIPCHK(hipMemsetAsync(d_planes, 0, 3 * C * W * 8, st));
    HIPCHK(hipMemsetAsync(d_open, 0, K * 4, st));
    HIPCHK(launch_free_cell_classes(V, fc.cons.as<FreeCon>(), fc.pivots.as<uint32_t>(), P.n_constraints, delta, d_planes, C * W, d_open, st));
    HIPCHK(launch_free_cell_classes_count(d_planes, C * W, (uint32_t)C, V.log_n, d_per, st));
    counts->resize(3 * C + K);
    HIPCHK(hipMemcpyAsync(counts->data(), d_per, counts->size() * 4, hipMemcpyDeviceToHost, st));
    if (planes == FreePlanes::ALL) HIPCHK(hipMemcpyAsync(planes_out, d_planes, 3 * C * W * 8, hipMemcpyDeviceToHost, st));
    if (planes == FreePlanes::CAUGHT) HIPCHK(hipMemcpyAsync(planes_out, d_planes + 2 * C * W, C * W * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(c));
    return STARKHIP_OK;
}

// starkhip_check_trace_free_cell_classes.  The planes come back only when asked for.
int check_trace_free_cell_classes(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                                  uint64_t* planes, uint32_t* open_rows, starkhip_free_cell_classes_t* out) {
    const size_t C = air.prog.n_cols, K = air.prog.n_constraints;
    std::vector<uint32_t> counts;
    if (int rc = free_cell_classes_run(c, air, in, pis, delta, planes ? FreePlanes::ALL : FreePlanes::NONE, planes, &counts)) return rc;
    if (per_column) std::copy(counts.begin(), counts.begin() + 3 * C, per_column);
    if (open_rows) std::copy(counts.begin() + 3 * C, counts.end(), open_rows);
    *out = free_cell_classes_summary(counts.data(), counts.data() + 3 * C, in.n_rows, C, K);
    return STARKHIP_OK;
}

// starkhip_check_trace_free_cells: the same run, and of its result the projection of free_cells.h.  The bitmap is the caught plane,
// read back only when asked for and complemented in the caller's buffer.
int check_trace_free_cells(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                           uint64_t* free_mask, starkhip_free_cells_t* out) {
    std::vector<uint32_t> counts;
    if (int rc = free_cell_classes_run(c, air, in, pis, delta, free_mask ? FreePlanes::CAUGHT : FreePlanes::NONE, free_mask, &counts)) return rc;
    *out = free_cells_from_classes(counts.data(), in.n_rows, air.prog.n_cols, per_column, free_mask);
    return STARKHIP_OK;
}

}  // namespace starkhip
