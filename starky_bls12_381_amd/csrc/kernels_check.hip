// Trace checker on gfx950 (starkhip_check_trace): every constraint of an AIR on every row of a trace, the device twin of
// oracle_check_trace.  It is what someone who writes an AIR, or changes a trace generator, runs before a proof: FinalExp is
// 8192 rows x 360 800 constraints.
//
// The AIR arrives as the op stream of quotient_ops.h (compile_quotient_ops), cut at group boundaries into chunks; a workgroup is
// one wave = 64 consecutive rows x one chunk, and the grid is (n / 64) x chunks waves.  Ops are wave-uniform and every lane
// evaluates its own row over the trace domain itself (no coset): local = row r, next = row (r + 1) mod n of the column-major
// trace, so the 64 lanes of a cell load read 512 contiguous bytes.  Each FOLD op ends one constraint, whose mask-free value
// G * body is tested for zero instead of being Horner-folded; the constraint's kind decides whether row r is one it applies to
// (transition: r < n - 1, first: r = 0, last: r = n - 1).  A lane counts its violations and keeps the first (lowest constraint
// index: they arrive in order) as (k << 32) | row; at the end of the chunk, lanes with violations add their count and take the
// minimum of their keys with 64-bit vector atomics, so a satisfying trace issues no atomic at all.  The host recomputes the
// value of the first violation from that one frame.
#include <hip/hip_runtime.h>

#include "air_ir.h"
#include "gl.h"
#include "kernels.h"
#include "quotient_ops.h"

namespace starkhip {

struct CheckParams {
    const QOp* ops;             // compile_quotient_ops() output
    const uint32_t* chunk_op;   // [n_chunks + 1] first op of each chunk
    const uint32_t* chunk_k0;   // [n_chunks] index of each chunk's first constraint
    const gl_t* trace;          // column-major [C][n]
    const gl_t* pis;
    unsigned long long* out;    // [0] violations, [1] min over violations of (k << 32) | row; preset to 0 and ~0
    unsigned log_n;
};

__global__ __launch_bounds__(64) void check_trace_kernel(CheckParams P) { STARKHIP_PRIO_ENTRY
    const uint32_t n = 1u << P.log_n;
    const uint32_t r_raw = blockIdx.x * 64u + threadIdx.x;
    const bool live = r_raw < n;  // traces shorter than a wave: idle lanes shadow row 0 and report nothing
    const uint32_t r = live ? r_raw : 0u, rn = (r + 1u) & (n - 1u);
    const bool is_first = r == 0, is_last = r == n - 1u;
    const uint32_t chunk = blockIdx.y;
    const uint32_t op_end = P.chunk_op[chunk + 1];
    uint32_t k = P.chunk_k0[chunk];
    gl_t G = 1, body = 0, v = 1;
    bool active = true;
    unsigned long long cnt = 0, key = ~0ull;
    for (uint32_t i = P.chunk_op[chunk]; i < op_end; i++) {
        const uint32_t hdr = P.ops[i].hdr, ref = P.ops[i].ref, op = hdr & 7u;
        if (op == QOP_GROUP) {
            const uint32_t kind = (hdr >> QOP_KIND_SHIFT) & 3u;
            active = kind == KIND_PLAIN || (kind == KIND_TRANSITION && !is_last) || (kind == KIND_FIRST && is_first) || (kind == KIND_LAST && is_last);
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
            if (active && gl_mul(G, body) != 0) {
                if (!cnt) key = ((unsigned long long)k << 32) | r;
                cnt++;
            }
            k++;
            body = 0;
        }
    }
    if (live && cnt) {
        atomicAdd(&P.out[0], cnt);
        atomicMin(&P.out[1], key);
    }
}

hipError_t launch_check_trace(const QOp* ops, const uint32_t* chunk_op, const uint32_t* chunk_k0, unsigned n_chunks, const gl_t* trace,
                              const gl_t* pis, unsigned log_n, unsigned long long* out, hipStream_t st) {
    CheckParams P;
    P.ops = ops; P.chunk_op = chunk_op; P.chunk_k0 = chunk_k0; P.trace = trace; P.pis = pis; P.out = out; P.log_n = log_n;
    const unsigned blocks = (unsigned)((((size_t)1 << log_n) + 63) / 64);
    hipLaunchKernelGGL(check_trace_kernel, dim3(blocks, n_chunks), dim3(64), 0, st, P);
    return hipGetLastError();
}

}  // namespace starkhip
