// Trace checkers on gfx950: every constraint of an AIR on every row of a trace, the device twin of oracle_check_trace.  It is what
// someone who writes an AIR, or changes a trace generator, runs before a proof: FinalExp is 8192 rows x 360 800 constraints.
// starkhip_check_trace counts the violations and names the first; starkhip_check_trace_report says which constraints fail on which
// rows, with the values of the first of them.
//
// The AIR arrives as the op stream of quotient_ops.h (compile_quotient_ops), cut at group boundaries into chunks; a workgroup is
// one wave = 64 consecutive rows x one chunk, and the grid is (n / 64) x chunks waves.  Ops are wave-uniform and every lane
// evaluates its own row over the trace domain itself (no coset): local = row r, next = row (r + 1) mod n of the column-major
// trace, so the 64 lanes of a cell load read 512 contiguous bytes.  Each FOLD op ends one constraint, whose mask-free value
// G * body is tested for zero instead of being Horner-folded; the constraint's kind decides whether row r is one it applies to
// (constraint_applies, air_ir.h).  walk_chunk is that machine; the three kernels differ in what they do at a FOLD.
//
// Plain check: a lane counts its violations and keeps the first (lowest constraint index: they arrive in order) as (k << 32) | row;
// at the end of the chunk, lanes with violations add their count and take the minimum of their keys with 64-bit vector atomics, so
// a satisfying trace issues no atomic at all.  The host recomputes the value of the first violation from that one frame.
//
// Report, pass 1 (count): at each FOLD the wave forms the ballot of its violating lanes.  A nonzero ballot -- a wave-uniform branch
// -- has lane 0 add its popcount to counts[k]; at the end of the chunk the OR of the ballots, the wave's 64 rows, goes into
// row_mask.  One atomic per (wave, violated constraint), and none on a satisfying trace.
//
// Report, pass 2 (list): launched over the chunks that hold a constraint the host selected (its entries start at base[k] of the
// list; ~0: not selected), and a wave whose 64 rows pass 1 found clean leaves at once.  At a FOLD of a selected constraint with a
// nonzero ballot, lane 0 reserves popcount slots from the constraint's cursor, the reservation is broadcast, and each violating
// lane writes {k, row, G * body} at base[k] + reservation + its rank in the ballot.  Waves reserve in any order: the host sorts
// each constraint's segment by row.
//
// Every result word leaves through vector stores and vector atomics.  No LDS.
#include <hip/hip_runtime.h>

#include "air_ir.h"
#include "gl.h"
#include "kernels.h"
#include "quotient_ops.h"

namespace starkhip {

// One wave's walk over the ops of `chunk` on rows blockIdx.x * 64 .. + 63.  At every FOLD it calls at_fold(k, r, applies, G, body):
// constraint k, this lane's row, whether k applies to it, and the two factors of its value -- not their product, which only the
// callee knows whether it needs.  at_fold is reached by all 64 lanes in wave-uniform control flow (the ops are wave-uniform, and
// `applies` is handed over, not branched on): the report's ballot and readfirstlane rely on it, so never put the call under a
// per-lane condition.
template <class AtFold>
__device__ __forceinline__ void walk_chunk(const CheckView& V, uint32_t chunk, AtFold at_fold) {
    const uint32_t n = 1u << V.log_n;
    const uint32_t r_raw = blockIdx.x * 64u + threadIdx.x;
    const bool live = r_raw < n;  // traces shorter than a wave: idle lanes shadow row 0 and no constraint applies to them
    const uint32_t r = live ? r_raw : 0u, rn = (r + 1u) & (n - 1u);
    const uint32_t op_end = V.chunk_op[chunk + 1];
    uint32_t k = V.chunk_k0[chunk];
    gl_t G = 1, body = 0, v = 1;
    bool applies = true;
    for (uint32_t i = V.chunk_op[chunk]; i < op_end; i++) {
        const uint32_t hdr = V.ops[i].hdr, ref = V.ops[i].ref, op = hdr & 7u;
        if (op == QOP_GROUP) {
            applies = live && constraint_applies((hdr >> QOP_KIND_SHIFT) & 3u, r, n);
            G = 1;
            continue;
        }
        if (op != QOP_GATE && op != QOP_FACTOR && op != QOP_TERM) continue;  // NOP padding, ENDGROUP
        // A cell is ANY 64-bit word of its class mod p (starkhip.h, starkhip_prove), and x, v and u below may be one.  gl_mul reduces
        // any operands and gl_add takes one of them raw (gl.h); a subtrahend has to be canonical, so the two places a raw word could be
        // one reduce it first -- a wave-uniform choice, nothing per load (a reduction at the load cost 3.5 % of a FinalExp check).
        gl_t x = 1;
        if (!(hdr & QOP_NOCELL)) x = V.trace[((size_t)(ref & REF_COL_MASK) << V.log_n) + ((ref & REF_NEXT) ? rn : r)];  // 64-bit: 4.8 GB
        if (op == QOP_GATE) {
            G = gl_mul(G, (ref & REF_COMPL) ? gl_sub(1, gl_from_u64(x)) : x);
            continue;
        }
        const bool prev = (hdr & QOP_PREV) != 0;
        if (op == QOP_FACTOR) {
            v = prev ? gl_mul(v, x) : x;
            continue;
        }
        const gl_t u = prev ? gl_mul(v, x) : x;  // NOCELL: x = 1
        const uint32_t ck = (hdr >> QOP_CK_SHIFT) & 7u;
        if (ck == CK_PLUS) body = gl_add(body, u);
        else if (ck == CK_MINUS) body = gl_sub(body, prev ? u : gl_from_u64(u));
        else if (ck == CK_CONST) body = gl_add(body, gl_mul(u, V.ops[i].k));
        else if (ck == CK_PI) body = gl_add(body, gl_mul(u, V.pis[hdr >> QOP_IDX_SHIFT]));
        else body = gl_sub(body, gl_mul(u, V.pis[hdr >> QOP_IDX_SHIFT]));
        if (hdr & QOP_FOLD) {
            at_fold(k, r, applies, G, body);
            k++;
            body = 0;
        }
    }
}

// Each kernel takes one parameter block with the view in front, so that the words the op loop reads are fetched together, and waited
// for, ahead of the loop.
struct CheckParams {
    CheckView v;
    unsigned long long* out;  // [0] violations, [1] min over violations of (k << 32) | row; preset to 0 and ~0
};

__global__ __launch_bounds__(64) void check_trace_kernel(CheckParams P) { STARKHIP_PRIO_ENTRY
    unsigned long long cnt = 0, key = ~0ull;
    walk_chunk(P.v, blockIdx.y, [&](uint32_t k, uint32_t r, bool applies, gl_t G, gl_t body) {
        const bool bad = applies & (gl_mul(G, body) != 0);
        key = (bad & !cnt) ? ((unsigned long long)k << 32) | r : key;
        cnt += bad;
    });
    if (cnt) {
        atomicAdd(&P.out[0], cnt);
        atomicMin(&P.out[1], key);
    }
}

struct CheckReportParams {
    CheckView v;
    uint32_t* counts;              // [K], zeroed.  Pass 1: rows on which each constraint is violated; pass 2: the constraints' cursors
    unsigned long long* row_mask;  // [(n + 63) / 64]: bit (r & 63) of word r >> 6.  Pass 1 ORs into it (zeroed), pass 2 reads it
    const uint32_t* chunks;        // pass 2: [gridDim.y] the chunks launched
    const uint32_t* base;          // pass 2: [K] first list entry of each selected constraint, ~0 for the others
    unsigned long long* list;      // pass 2: [list_len] x {constraint, row, value}
    uint32_t list_len;
};

template <bool LIST>
__global__ __launch_bounds__(64) void check_report_kernel(CheckReportParams P) { STARKHIP_PRIO_ENTRY
    if (LIST && P.row_mask[blockIdx.x] == 0) return;
    unsigned long long rows = 0;  // wave-uniform: the lanes that saw a violation
    walk_chunk(P.v, LIST ? P.chunks[blockIdx.y] : blockIdx.y, [&](uint32_t k, uint32_t r, bool applies, gl_t G, gl_t body) {
        const uint32_t first = LIST ? P.base[k] : 0u;
        if (LIST && first == ~0u) return;
        const gl_t value = gl_mul(G, body);
        const bool bad = applies && value != 0;
        const unsigned long long ballot = __ballot(bad);
        if (!ballot) return;
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
    });
    if (!LIST && rows && threadIdx.x == 0) atomicOr(&P.row_mask[blockIdx.x], rows);
}

static dim3 check_grid(const CheckView& v, unsigned chunks) { return dim3((unsigned)((((size_t)1 << v.log_n) + 63) / 64), chunks); }

hipError_t launch_check_trace(const CheckView& v, unsigned long long* out, hipStream_t st) {
    hipLaunchKernelGGL(check_trace_kernel, check_grid(v, v.n_chunks), dim3(64), 0, st, CheckParams{v, out});
    return hipGetLastError();
}

hipError_t launch_check_report_count(const CheckView& v, uint32_t* counts, unsigned long long* row_mask, hipStream_t st) {
    const CheckReportParams P = {v, counts, row_mask, nullptr, nullptr, nullptr, 0};
    hipLaunchKernelGGL(check_report_kernel<false>, check_grid(v, v.n_chunks), dim3(64), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_check_report_list(const CheckView& v, const uint32_t* chunks, unsigned n_launched, uint32_t* cursors, const unsigned long long* row_mask,
                                    const uint32_t* base, unsigned long long* list, uint32_t list_len, hipStream_t st) {
    const CheckReportParams P = {v, cursors, const_cast<unsigned long long*>(row_mask), chunks, base, list, list_len};
    hipLaunchKernelGGL(check_report_kernel<true>, check_grid(v, n_launched), dim3(64), 0, st, P);
    return hipGetLastError();
}

}  // namespace starkhip
