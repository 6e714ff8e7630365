// The free-cell kernel on gfx950, behind starkhip_check_trace_free_cell_classes and starkhip_check_trace_free_cells: for every cell
// of a trace, does a constraint that applies read it (read), does one read it with its gate product nonzero (open), does one
// notice delta added to it (caught)?  And per constraint: on how many frames of the unchanged trace are its gates open?  The rule
// is in free_cells.h; the host half is free_cell_classes_run in check_trace.hip.  The audit is the caught plane of this kernel,
// complemented on the host.
//
// Geometry and op stream are the trace checkers' (kernels_check.hip): a workgroup is one wave = 64 consecutive rows x one chunk of
// the op stream, ops are wave-uniform, one lane per row, 64-bit trace offsets, idle lanes of a short trace shadow row 0 and no
// constraint applies to them.  What differs is the walk.  For each constraint of its chunk (FreeCon: the op span of the group's
// gates, the op span of the constraint's terms, its pivots) and each pivot -- a (column | next) reference the constraint reads --
// the wave re-walks the two spans (gate_product, constraint_body), adding delta to a loaded cell when its reference is the pivot,
// a scalar compare.
//
// A lane stands for the CHANGED CELL's row rc, not for the frame's: a local pivot tests frame rc (local cells at rc, next cells at
// rc + 1), a next pivot frame (rc - 1) mod n (local cells at rc - 1, next cells at rc), and `applies` is taken for the frame.  So the
// wave's 64 result bits always belong to one word per plane, [pivot column][blockIdx.x].  Per (constraint, pivot) the wave forms
// three ballots -- applies, applies & G' != 0, applies & G' * body' != 0 -- for that word of the three planes.  Waves of other
// chunks and other constraints of this chunk share the word: lane 0 ORs each ballot in with a 64-bit vector atomic, and only for
// bits a load of the word shows are still missing.  Every OR only adds bits, so the planes do not depend on the order the waves
// run in.  The load is an agent-scope atomic one: a plain load may be served by the CU's vector cache, which the atomics of this
// very wave go past.
//
// THE INVARIANT BEHIND THE SKIP.  caught is contained in open is contained in read, ballot by ballot (G' * body' != 0 needs G' != 0,
// and both need `applies`), and a walk sends all three of its ballots or none.  So the walk that sets a row's caught bit also sets
// that row's open and read bits, or found them set.  A caught word that holds every live row therefore stands for three finished
// words, and a wave that loads such a word skips its walk: nothing it could add is missing in any plane once the kernel has ended.
// (While it runs, the ORs of the other wave may still be in flight; nobody reads open or read bits to decide anything.)  On a
// well-constrained trace the first constraint that reads a column fills its words and the later ones leave after one load.
//
// Two more wave-uniform skips, neither of which can change a bit.  A pivot whose constraint applies to none of the wave's frames (a
// first-row constraint away from row 0) has three empty ballots.  And where the gate product G' is zero on every lane the
// constraint applies to, the open ballot is empty, so the caught one is: the body is not walked, only the read bits go out.  That
// is the common case of a gadget outside the rows of its own operation.
//
// open_rows[k]: once per group of the chunk -- the gates and the kind are the group's -- the wave takes G on the unchanged local frame
// and ballots live & applies & G != 0; each constraint of the group then has lane 0 add the popcount to open_rows[k] with one 32-bit
// vector atomic, when it is nonzero.  A constraint is in one chunk, so each (constraint, 64 rows) is counted once.
//
// free_cell_classes_count_kernel, one wave per column, counts silent = open & ~caught, gated = read & ~open and unread = ~read (of
// the live rows) and leaves the planes as they are.  Every result word leaves through vector stores and vector atomics.  No LDS,
// no scratch.
#include <hip/hip_runtime.h>

#include "air_ir.h"
#include "free_cells.h"
#include "gl.h"
#include "kernels.h"
#include "quotient_ops.h"

namespace starkhip {

struct FreeClassesParams {
    CheckView v;
    const FreeCon* cons;         // [n_constraints]
    const uint32_t* pivots;
    unsigned long long* planes;  // [3][C][(n + 63) / 64]: read, open, caught; zeroed
    uint32_t* open_rows;         // [n_constraints], zeroed
    size_t plane_words;          // C * ((n + 63) / 64)
    gl_t delta;
    uint32_t n_constraints;
};

static __device__ __forceinline__ unsigned long long wave_uniform(unsigned long long x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// The two span walks, over the cells cell(ref) hands out.  A cell is ANY 64-bit word of its class mod p, reduced where walk_chunk
// (kernels_check.hip) reduces it: gl_mul reduces any operands and gl_add takes one of them raw (gl.h), a subtrahend has to be
// canonical, so a complemented gate's cell and a single-cell minus term are reduced first -- wave-uniform choices, nothing per load.

// G: the product of a group's gates, ops (g0, g1) -- op g0 is the GROUP.  A gate is its cell x, or 1 - x under REF_COMPL.
template <class Cell>
static __device__ __forceinline__ gl_t gate_product(const CheckView& V, uint32_t g0, uint32_t g1, Cell cell) {
    gl_t G = 1;
    for (uint32_t i = g0 + 1; i < g1; i++) {
        const uint32_t ref = V.ops[i].ref;
        const gl_t x = cell(ref);
        G = gl_mul(G, (ref & REF_COMPL) ? gl_sub(1, gl_from_u64(x)) : x);
    }
    return G;
}

// body: a constraint's FACTOR and TERM ops [t0, t1) alone, with walk_chunk's values.  u is the op's cell x (1 under QOP_NOCELL), or
// v * x under QOP_PREV; a FACTOR keeps it as the running product v, a TERM adds it to the body with the coefficient CK_* names.
template <class Cell>
static __device__ __forceinline__ gl_t constraint_body(const CheckView& V, uint32_t t0, uint32_t t1, Cell cell) {
    gl_t body = 0, v = 1;
    for (uint32_t i = t0; i < t1; i++) {
        const uint32_t hdr = V.ops[i].hdr, ref = V.ops[i].ref;
        const gl_t x = (hdr & QOP_NOCELL) ? 1 : cell(ref);
        const bool prev = (hdr & QOP_PREV) != 0;
        const gl_t u = prev ? gl_mul(v, x) : x;
        if ((hdr & 7u) == QOP_FACTOR) {
            v = u;
            continue;
        }
        const uint32_t ck = (hdr >> QOP_CK_SHIFT) & 7u;
        if (ck == CK_PLUS) body = gl_add(body, u);
        else if (ck == CK_MINUS) body = gl_sub(body, prev ? u : gl_from_u64(u));  // a product is canonical, a lone cell need not be
        else if (ck == CK_CONST) body = gl_add(body, gl_mul(u, V.ops[i].k));
        else if (ck == CK_PI) body = gl_add(body, gl_mul(u, V.pis[hdr >> QOP_IDX_SHIFT]));
        else body = gl_sub(body, gl_mul(u, V.pis[hdr >> QOP_IDX_SHIFT]));
    }
    return body;
}

__global__ __launch_bounds__(64) void free_cell_classes_kernel(FreeClassesParams P) { STARKHIP_PRIO_ENTRY
    const CheckView& V = P.v;
    const uint32_t n = 1u << V.log_n, W = (n + 63u) >> 6;
    const uint32_t rc_raw = blockIdx.x * 64u + threadIdx.x;
    const bool live = rc_raw < n;
    const uint32_t rc = live ? rc_raw : 0u, rp = (rc - 1u) & (n - 1u), rn = (rc + 1u) & (n - 1u);
    const unsigned long long all = n >= 64u ? ~0ull : (1ull << n) - 1ull;  // the live lanes' bits
    const uint32_t chunk = blockIdx.y;
    const uint32_t k_end = chunk + 1 < V.n_chunks ? V.chunk_k0[chunk + 1] : P.n_constraints;
    uint32_t group = ~0u, open_here = 0;  // the GROUP op of the last constraint, its open frames among the wave's rows
    for (uint32_t k = V.chunk_k0[chunk]; k < k_end; k++) {
        const FreeCon cn = P.cons[k];
        const bool applies_local = live & constraint_applies(cn.kind, rc, n), applies_next = live & constraint_applies(cn.kind, rp, n);
        if (cn.g0 != group) {  // wave-uniform
            group = cn.g0;
            const gl_t G = gate_product(V, cn.g0, cn.g1, [&](uint32_t ref) {  // the unchanged local frame
                return V.trace[((size_t)(ref & REF_COL_MASK) << V.log_n) + ((ref & REF_NEXT) ? rn : rc)];
            });
            open_here = (uint32_t)__popcll(__ballot(applies_local && G != 0));
        }
        if (open_here && threadIdx.x == 0) atomicAdd(P.open_rows + k, open_here);
        for (uint32_t p = cn.piv0; p < cn.piv1; p++) {
            const uint32_t piv = P.pivots[p];
            const bool next_pivot = (piv & REF_NEXT) != 0;
            const bool applies = next_pivot ? applies_next : applies_local;
            const unsigned long long b_read = __ballot(applies);
            if (!b_read) continue;  // wave-uniform, as every branch on a ballot or a loaded word below
            unsigned long long* word_r = P.planes + (size_t)(piv & REF_COL_MASK) * W + blockIdx.x;
            unsigned long long *word_o = word_r + P.plane_words, *word_c = word_o + P.plane_words;
            const unsigned long long have_c = wave_uniform(__hip_atomic_load(word_c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if ((have_c & all) == all) continue;  // and then open and read hold them too: the invariant in the header
            const unsigned long long seen_o = __hip_atomic_load(word_o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // awaited after the walk
            const unsigned long long seen_r = __hip_atomic_load(word_r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t r_local = next_pivot ? rp : rc, r_next = next_pivot ? rc : rn;
            // the changed frame; delta goes onto the raw word, which gl_add takes as it is
            auto cell = [&](uint32_t ref) {
                const gl_t x = V.trace[((size_t)(ref & REF_COL_MASK) << V.log_n) + ((ref & REF_NEXT) ? r_next : r_local)];
                return (ref & (REF_COL_MASK | REF_NEXT)) == piv ? gl_add(P.delta, x) : x;
            };
            const gl_t G = gate_product(V, cn.g0, cn.g1, cell);
            const unsigned long long b_open = __ballot(applies && G != 0);
            unsigned long long b_caught = 0;  // within b_open: a zero G gives a zero product
            if (b_open) b_caught = __ballot(applies && gl_mul(G, constraint_body(V, cn.t0, cn.t1, cell)) != 0);
            const unsigned long long miss_r = b_read & ~wave_uniform(seen_r), miss_o = b_open & ~wave_uniform(seen_o);
            const unsigned long long miss_c = b_caught & ~have_c;
            if (threadIdx.x == 0) {  // all three of this walk, or those already there
                if (miss_r) atomicOr(word_r, miss_r);
                if (miss_o) atomicOr(word_o, miss_o);
                if (miss_c) atomicOr(word_c, miss_c);
            }
        }
    }
}

// One wave per column: per_column[c] = {silent, gated, unread} rows from the three planes, which stay as they are.
__global__ __launch_bounds__(64) void free_cell_classes_count_kernel(const unsigned long long* planes, size_t plane_words, uint32_t W, uint32_t n,
                                                                     uint32_t* per_column) {
    const unsigned long long* rd = planes + (size_t)blockIdx.x * W;
    const unsigned long long *op = rd + plane_words, *ca = op + plane_words;
    uint32_t silent = 0, gated = 0, unread = 0;
    for (uint32_t w = threadIdx.x; w < W; w += 64u) {
        const unsigned long long all = n >= 64u ? ~0ull : (1ull << n) - 1ull;  // n < 64: one word, its low n bits
        const unsigned long long r = rd[w], o = op[w], c = ca[w];
        silent += (uint32_t)__popcll(o & ~c);
        gated += (uint32_t)__popcll(r & ~o);
        unread += (uint32_t)__popcll(~r & all);
    }
    for (int off = 32; off; off >>= 1) {
        silent += __shfl_xor(silent, off);
        gated += __shfl_xor(gated, off);
        unread += __shfl_xor(unread, off);
    }
    if (threadIdx.x == 0) {
        uint32_t* out = per_column + (size_t)blockIdx.x * 3;
        out[0] = silent;
        out[1] = gated;
        out[2] = unread;
    }
}

hipError_t launch_free_cell_classes(const CheckView& v, const FreeCon* cons, const uint32_t* pivots, uint32_t n_constraints, gl_t delta,
                                    unsigned long long* planes, size_t plane_words, uint32_t* open_rows, hipStream_t st) {
    const FreeClassesParams P = {v, cons, pivots, planes, open_rows, plane_words, delta, n_constraints};
    hipLaunchKernelGGL(free_cell_classes_kernel, dim3((unsigned)((((size_t)1 << v.log_n) + 63) / 64), v.n_chunks), dim3(64), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_free_cell_classes_count(const unsigned long long* planes, size_t plane_words, uint32_t n_cols, unsigned log_n,
                                          uint32_t* per_column, hipStream_t st) {
    const uint32_t n = 1u << log_n;
    hipLaunchKernelGGL(free_cell_classes_count_kernel, dim3(n_cols), dim3(64), 0, st, planes, plane_words, (n + 63u) >> 6, n, per_column);
    return hipGetLastError();
}

}  // namespace starkhip
