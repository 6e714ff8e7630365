// Trace checker's report on gfx950 (starkhip_check_trace_report): which constraints of an AIR fail on which rows of a trace, and the
// values of the first of them.  Two passes over the geometry of check_trace_kernel (kernels_check.hip): a workgroup is one wave =
// 64 consecutive rows x one chunk of the op stream of compile_quotient_ops, ops are wave-uniform, a lane evaluates its own row
// (next = (r + 1) mod n) of the column-major trace, and each FOLD op ends one constraint whose mask-free value G * body is compared
// with zero on the rows its kind applies to.
//
// Pass 1 (count): at each FOLD the wave forms the ballot of its violating lanes.  A nonzero ballot -- a wave-uniform branch -- has
// lane 0 add its popcount to counts[k]; at the end of the chunk the OR of the ballots, the wave's 64 rows, goes into row_mask.  One
// atomic per (wave, violated constraint), and none on a satisfying trace.
//
// Pass 2 (list): launched over the chunks that hold a constraint the host selected (its entries start at base[k] of the list; ~0:
// not selected), and a wave whose 64 rows pass 1 found clean leaves at once.  At a FOLD of a selected constraint with a nonzero
// ballot, lane 0 reserves popcount slots from the constraint's cursor, the reservation is broadcast, and each violating lane writes
// {k, row, G * body} at base[k] + reservation + its rank in the ballot.  Waves reserve in any order: the host sorts each
// constraint's segment by row.
//
// Every result word leaves through vector stores and vector atomics.  No LDS.
#include <hip/hip_runtime.h>

#include "air_ir.h"
#include "gl.h"
#include "kernels.h"
#include "quotient_ops.h"

namespace starkhip {

struct CheckReportParams {
    const QOp* ops;                // compile_quotient_ops() output
    const uint32_t* chunk_op;      // [n_chunks + 1] first op of each chunk
    const uint32_t* chunk_k0;      // [n_chunks] index of each chunk's first constraint
    const gl_t* trace;             // column-major [C][n]
    const gl_t* pis;
    uint32_t* counts;              // [K], zeroed.  Pass 1: rows on which each constraint is violated; pass 2: the constraints' cursors
    unsigned long long* row_mask;  // [(n + 63) / 64]: bit (r & 63) of word r >> 6.  Pass 1 ORs into it (zeroed), pass 2 reads it
    const uint32_t* chunks;        // pass 2: [gridDim.y] the chunks launched
    const uint32_t* base;          // pass 2: [K] first list entry of each selected constraint, ~0 for the others
    unsigned long long* list;      // pass 2: [list_len] x {constraint, row, value}
    uint32_t list_len;
    unsigned log_n;
};

template <bool LIST>
__global__ __launch_bounds__(64) void check_report_kernel(CheckReportParams P) { STARKHIP_PRIO_ENTRY
    if (LIST && P.row_mask[blockIdx.x] == 0) return;
    const uint32_t n = 1u << P.log_n;
    const uint32_t r_raw = blockIdx.x * 64u + threadIdx.x;
    const bool live = r_raw < n;  // traces shorter than a wave: idle lanes shadow row 0 and report nothing
    const uint32_t r = live ? r_raw : 0u, rn = (r + 1u) & (n - 1u);
    const bool is_first = r == 0, is_last = r == n - 1u;
    const uint32_t chunk = LIST ? P.chunks[blockIdx.y] : blockIdx.y;
    const uint32_t op_end = P.chunk_op[chunk + 1];
    uint32_t k = P.chunk_k0[chunk];
    gl_t G = 1, body = 0, v = 1;
    bool active = true;
    unsigned long long rows = 0;  // wave-uniform: the lanes that saw a violation
    for (uint32_t i = P.chunk_op[chunk]; i < op_end; i++) {
        const uint32_t hdr = P.ops[i].hdr, ref = P.ops[i].ref, op = hdr & 7u;
        if (op == QOP_GROUP) {
            const uint32_t kind = (hdr >> QOP_KIND_SHIFT) & 3u;
            active = live && (kind == KIND_PLAIN || (kind == KIND_TRANSITION && !is_last) || (kind == KIND_FIRST && is_first) || (kind == KIND_LAST && is_last));
            G = 1;
            continue;
        }
        if (op != QOP_GATE && op != QOP_FACTOR && op != QOP_TERM) continue;  // NOP padding, ENDGROUP
        gl_t x = 1;
        if (!(hdr & QOP_NOCELL)) x = P.trace[((size_t)(ref & REF_COL_MASK) << P.log_n) + ((ref & REF_NEXT) ? rn : r)];  // 64-bit: 4.8 GB
        if (op == QOP_GATE) {
            G = gl_mul(G, (ref & REF_COMPL) ? gl_sub(1, x) : x);
            continue;
        }
        if (op == QOP_FACTOR) {
            v = (hdr & QOP_PREV) ? gl_mul(v, x) : x;
            continue;
        }
        const gl_t u = (hdr & QOP_PREV) ? gl_mul(v, x) : x;  // NOCELL: x = 1
        const uint32_t ck = (hdr >> QOP_CK_SHIFT) & 7u;
        if (ck == CK_PLUS) body = gl_add(body, u);
        else if (ck == CK_MINUS) body = gl_sub(body, u);
        else if (ck == CK_CONST) body = gl_add(body, gl_mul(u, P.ops[i].k));
        else if (ck == CK_PI) body = gl_add(body, gl_mul(u, P.pis[hdr >> QOP_IDX_SHIFT]));
        else body = gl_sub(body, gl_mul(u, P.pis[hdr >> QOP_IDX_SHIFT]));
        if (hdr & QOP_FOLD) {
            const uint32_t first = LIST ? P.base[k] : 0u;
            if (!LIST || first != ~0u) {
                const gl_t value = gl_mul(G, body);
                const bool bad = active && value != 0;
                const unsigned long long ballot = __ballot(bad);
                if (ballot) {
                    const uint32_t cnt = (uint32_t)__popcll(ballot);
                    if (!LIST) {
                        if (threadIdx.x == 0) atomicAdd(&P.counts[k], cnt);
                        rows |= ballot;
                    } else {
                        uint32_t at = 0;
                        if (threadIdx.x == 0) at = atomicAdd(&P.counts[k], cnt);
                        at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);  // every lane is here: the first one is lane 0
                        const uint32_t slot = first + at + (uint32_t)__popcll(ballot & ((1ull << threadIdx.x) - 1ull));
                        if (bad && slot < P.list_len) {
                            unsigned long long* e = P.list + (size_t)slot * 3;
                            e[0] = k;
                            e[1] = r;
                            e[2] = value;
                        }
                    }
                }
            }
            k++;
            body = 0;
        }
    }
    if (!LIST && rows && threadIdx.x == 0) atomicOr(&P.row_mask[blockIdx.x], rows);
}

hipError_t launch_check_report_count(const QOp* ops, const uint32_t* chunk_op, const uint32_t* chunk_k0, unsigned n_chunks, const gl_t* trace,
                                     const gl_t* pis, unsigned log_n, uint32_t* counts, unsigned long long* row_mask, hipStream_t st) {
    CheckReportParams P = {};
    P.ops = ops; P.chunk_op = chunk_op; P.chunk_k0 = chunk_k0; P.trace = trace; P.pis = pis; P.counts = counts; P.row_mask = row_mask;
    P.log_n = log_n;
    const unsigned blocks = (unsigned)((((size_t)1 << log_n) + 63) / 64);
    hipLaunchKernelGGL(check_report_kernel<false>, dim3(blocks, n_chunks), dim3(64), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_check_report_list(const QOp* ops, const uint32_t* chunk_op, const uint32_t* chunk_k0, const uint32_t* chunks, unsigned n_launched,
                                    const gl_t* trace, const gl_t* pis, unsigned log_n, uint32_t* cursors, const unsigned long long* row_mask,
                                    const uint32_t* base, unsigned long long* list, uint32_t list_len, hipStream_t st) {
    CheckReportParams P = {};
    P.ops = ops; P.chunk_op = chunk_op; P.chunk_k0 = chunk_k0; P.trace = trace; P.pis = pis; P.counts = cursors;
    P.row_mask = const_cast<unsigned long long*>(row_mask); P.chunks = chunks; P.base = base; P.list = list; P.list_len = list_len;
    P.log_n = log_n;
    const unsigned blocks = (unsigned)((((size_t)1 << log_n) + 63) / 64);
    hipLaunchKernelGGL(check_report_kernel<true>, dim3(blocks, n_launched), dim3(64), 0, st, P);
    return hipGetLastError();
}

}  // namespace starkhip
