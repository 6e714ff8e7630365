// Free-cell audit on gfx950 (starkhip_check_trace_free_cells): for every cell of a trace, does some constraint that reads it turn
// nonzero when delta is added to that one cell?  The rule is in free_cells.h; the host half is check_trace_free_cells in
// check_trace.hip.
//
// Geometry and op stream are the trace checkers' (kernels_check.hip): a workgroup is one wave = 64 consecutive rows x one chunk
// of the op stream, ops are wave-uniform, one lane per row, 64-bit trace offsets, idle lanes of a short trace shadow row 0 and
// no constraint applies to them.  What differs is the walk.  For each constraint of its chunk (FreeCon: the op span of the
// group's gates, the op span of the constraint's terms, its pivots) and each pivot -- a (column | next) reference the constraint
// reads -- the wave re-walks the two spans, adding delta to a loaded cell when its reference is the pivot, a scalar compare.
//
// A lane stands for the CHANGED CELL's row rc, not for the frame's: a local pivot tests frame rc (local cells at rc, next cells
// at rc + 1), a next pivot frame (rc - 1) mod n (local cells at rc - 1, next cells at rc), and `applies` is taken for the frame.
// So the wave's 64 result bits always belong to one word of the pivot column's bitmap, caught[column][blockIdx.x].  Waves of other
// chunks and other constraints of this chunk share that word: lane 0 ORs the ballot in with a 64-bit vector atomic, and only for
// bits a load of the word shows are still missing.  The same load lets the wave skip the re-walk altogether when the word already
// holds every live row: a re-walk can only add bits, so neither skip can change the result, whatever order the waves run in.  On a
// well-constrained trace the first constraint that reads a column fills its words and the later ones leave after one load.  The
// load is an agent-scope atomic one: a plain load may be served by the CU's vector cache, which the atomics of this very wave
// go past.
//
// free_cells_count_kernel then turns caught words into free words in place (bits at or beyond row n stay zero) and counts them per
// column.  Every result word leaves through vector stores and vector atomics.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "air_ir.h"
#include "free_cells.h"
#include "gl.h"
#include "kernels.h"
#include "quotient_ops.h"

namespace starkhip {

struct FreeCellsParams {
    CheckView v;
    const FreeCon* cons;         // [n_constraints]
    const uint32_t* pivots;
    unsigned long long* caught;  // [C][(n + 63) / 64], zeroed
    gl_t delta;
    uint32_t n_constraints;
};

static __device__ __forceinline__ unsigned long long wave_uniform(unsigned long long x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void free_cells_kernel(FreeCellsParams P) { STARKHIP_PRIO_ENTRY
    const CheckView& V = P.v;
    const uint32_t n = 1u << V.log_n, W = (n + 63u) >> 6;
    const uint32_t rc_raw = blockIdx.x * 64u + threadIdx.x;
    const bool live = rc_raw < n;
    const uint32_t rc = live ? rc_raw : 0u, rp = (rc - 1u) & (n - 1u), rn = (rc + 1u) & (n - 1u);
    const unsigned long long all = n >= 64u ? ~0ull : (1ull << n) - 1ull;  // the live lanes' bits
    const uint32_t chunk = blockIdx.y;
    const uint32_t k_end = chunk + 1 < V.n_chunks ? V.chunk_k0[chunk + 1] : P.n_constraints;
    for (uint32_t k = V.chunk_k0[chunk]; k < k_end; k++) {
        const FreeCon cn = P.cons[k];
        const bool applies_local = live & constraint_applies(cn.kind, rc, n), applies_next = live & constraint_applies(cn.kind, rp, n);
        for (uint32_t p = cn.piv0; p < cn.piv1; p++) {
            const uint32_t piv = P.pivots[p];
            unsigned long long* word = P.caught + (size_t)(piv & REF_COL_MASK) * W + blockIdx.x;
            const unsigned long long have = wave_uniform(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if ((have & all) == all) continue;  // wave-uniform
            const bool next_pivot = (piv & REF_NEXT) != 0;
            const uint32_t r_local = next_pivot ? rp : rc, r_next = next_pivot ? rc : rn;
            // a cell is any 64-bit word of its class mod p, reduced where walk_chunk reduces it: as a subtrahend (gl_add takes it raw)
            auto cell = [&](uint32_t ref) {
                const gl_t x = V.trace[((size_t)(ref & REF_COL_MASK) << V.log_n) + ((ref & REF_NEXT) ? r_next : r_local)];
                return (ref & (REF_COL_MASK | REF_NEXT)) == piv ? gl_add(P.delta, x) : x;
            };
            gl_t G = 1, body = 0, v = 1;
            for (uint32_t i = cn.g0 + 1; i < cn.g1; i++) {  // the gates; op g0 is the GROUP
                const uint32_t ref = V.ops[i].ref;
                const gl_t x = cell(ref);
                G = gl_mul(G, (ref & REF_COMPL) ? gl_sub(1, gl_from_u64(x)) : x);
            }
            for (uint32_t i = cn.t0; i < cn.t1; i++) {  // FACTOR and TERM ops alone: as walk_chunk evaluates them
                const uint32_t hdr = V.ops[i].hdr, ref = V.ops[i].ref;
                const gl_t x = (hdr & QOP_NOCELL) ? 1 : cell(ref);
                const bool prev = (hdr & QOP_PREV) != 0;
                if ((hdr & 7u) == QOP_FACTOR) {
                    v = prev ? gl_mul(v, x) : x;
                    continue;
                }
                const gl_t u = prev ? gl_mul(v, x) : x;
                const uint32_t ck = (hdr >> QOP_CK_SHIFT) & 7u;
                if (ck == CK_PLUS) body = gl_add(body, u);
                else if (ck == CK_MINUS) body = gl_sub(body, prev ? u : gl_from_u64(u));
                else if (ck == CK_CONST) body = gl_add(body, gl_mul(u, V.ops[i].k));
                else if (ck == CK_PI) body = gl_add(body, gl_mul(u, V.pis[hdr >> QOP_IDX_SHIFT]));
                else body = gl_sub(body, gl_mul(u, V.pis[hdr >> QOP_IDX_SHIFT]));
            }
            const bool bad = (next_pivot ? applies_next : applies_local) && gl_mul(G, body) != 0;
            const unsigned long long missing = __ballot(bad) & ~have;  // every lane is here: the skip above is wave-uniform
            if (missing && threadIdx.x == 0) atomicOr(word, missing);
        }
    }
}

// One wave per column: caught words -> free words (in place), per_column[c] = their bits.
__global__ __launch_bounds__(64) void free_cells_count_kernel(unsigned long long* words, uint32_t W, uint32_t n, uint32_t* per_column) {
    unsigned long long* col = words + (size_t)blockIdx.x * W;
    const unsigned long long all = n >= 64u ? ~0ull : (1ull << n) - 1ull;  // n < 64: one word, its low n bits
    uint32_t cnt = 0;
    for (uint32_t w = threadIdx.x; w < W; w += 64u) {
        const unsigned long long free_w = ~col[w] & all;
        col[w] = free_w;
        cnt += (uint32_t)__popcll(free_w);
    }
    for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (threadIdx.x == 0) per_column[blockIdx.x] = cnt;
}

hipError_t launch_free_cells(const CheckView& v, const FreeCon* cons, const uint32_t* pivots, uint32_t n_constraints, gl_t delta,
                             unsigned long long* caught, hipStream_t st) {
    const FreeCellsParams P = {v, cons, pivots, caught, delta, n_constraints};
    hipLaunchKernelGGL(free_cells_kernel, dim3((unsigned)((((size_t)1 << v.log_n) + 63) / 64), v.n_chunks), dim3(64), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_free_cells_count(unsigned long long* words, uint32_t n_cols, unsigned log_n, uint32_t* per_column, hipStream_t st) {
    const uint32_t n = 1u << log_n;
    hipLaunchKernelGGL(free_cells_count_kernel, dim3(n_cols), dim3(64), 0, st, words, (n + 63u) >> 6, n, per_column);
    return hipGetLastError();
}

}  // namespace starkhip
