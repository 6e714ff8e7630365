// What the trace transforms of kernels_lde.hip (whole columns on chip, 2^8 .. 2^13 rows) and kernels_lde_long.hip (columns split over
// workgroups, 2^14 .. 2^20 rows) share: the register radix-16 sub-transforms, the Stockham pass structure of one 2^LOGN-point transform
// and the host builder of its inter-pass twiddle table.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "gl_dev.h"

namespace starkhip {

// ---------------------------------------------------------------- register sub-transforms
constexpr int bitrev_c(int k, int bits) {
    int r = 0;
    for (int i = 0; i < bits; i++) r |= ((k >> i) & 1) << (bits - 1 - i);
    return r;
}
constexpr int ilog2_c(int x) { return x <= 1 ? 0 : 1 + ilog2_c(x >> 1); }

// Decimation-in-frequency radix-2 network of size R on v[BASE + STRIDE * i], root w_R = 2^(39 * 64 / R) (or its
// inverse).  Leaves X[k] at i = bitrev(k).
template <int R, bool INV, int BASE, int STRIDE>
struct Dif {
    static __device__ __forceinline__ void run(gl_t (&v)[16]) {
        constexpr int H = R / 2;
        constexpr int E_FWD = (39 * (64 / R)) % 192;
        constexpr int E = INV ? (192 - E_FWD) % 192 : E_FWD;
#pragma unroll
        for (int i = 0; i < H; i++) {
            const int e = (E * i) % 192;
            const gl_t a = v[BASE + STRIDE * i], b = v[BASE + STRIDE * (i + H)];
#ifdef STARKHIP_LDE_NN_BUTTERFLY  // the round-2 form: both operands arbitrary representatives, two wrap corrections per sum and difference
            v[BASE + STRIDE * i] = gl_add_nn(a, b);
            v[BASE + STRIDE * (i + H)] = e < 96 ? gl_mul_pow2_nn(gl_sub_nn(a, b), e) : gl_mul_pow2_nn(gl_sub_nn(b, a), e - 96);
#else
            // One operand canonical (3 instructions) makes both the sum and the difference single-correction forms (4 + 5
            // instead of 7 + 8): the second wrap of a + b or a - b needs BOTH operands >= p - 1 (gl_dev.h).  The subtrahend is
            // the canonical one: b for (a - b) 2^e, a for the negated form (b - a) 2^(e - 96).
            if (e < 96) {
                const gl_t bc = gl_canon(b);
                v[BASE + STRIDE * i] = gl_add_nc(a, bc);
                v[BASE + STRIDE * (i + H)] = gl_mul_pow2_nn(gl_sub_nc(a, bc), e);
            } else {
                const gl_t ac = gl_canon(a);
                v[BASE + STRIDE * i] = gl_add_nc(b, ac);
                v[BASE + STRIDE * (i + H)] = gl_mul_pow2_nn(gl_sub_nc(b, ac), e - 96);
            }
#endif
        }
        Dif<H, INV, BASE, STRIDE>::run(v);
        Dif<H, INV, BASE + STRIDE * H, STRIDE>::run(v);
    }
};
template <bool INV, int BASE, int STRIDE>
struct Dif<1, INV, BASE, STRIDE> {
    static __device__ __forceinline__ void run(gl_t (&)[16]) {}
};

// S = 16 / R independent size-R transforms: transform m lives in v[m + S * i]; natural order in and out.
template <int R, bool INV, int M>
struct SubNtts {
    static __device__ __forceinline__ void run(gl_t (&v)[16]) {
        constexpr int S = 16 / R;
        Dif<R, INV, M, S>::run(v);
        if constexpr (M + 1 < S) SubNtts<R, INV, M + 1>::run(v);
    }
};
template <int R>
__device__ __forceinline__ void unscramble(gl_t (&v)[16]) {
    constexpr int S = 16 / R, LOGR = ilog2_c(R);
    gl_t w[16];
#pragma unroll
    for (int m = 0; m < S; m++)
#pragma unroll
        for (int k = 0; k < R; k++) w[m + S * k] = v[m + S * bitrev_c(k, LOGR)];
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = w[i];
}

// ---------------------------------------------------------------- pass structure
template <int LOGN>
struct LdePlan {
    static constexpr int N = 1 << LOGN;
    static constexpr int T = N / 16;                       // threads per column
    static constexpr int FULL = LOGN / 4;                  // radix-16 passes
    static constexpr int TAIL = LOGN % 4;                  // log2 of the last pass's radix (0: none)
    static constexpr int NP = FULL + (TAIL ? 1 : 0);
    static constexpr int radix(int p) { return p < FULL ? 16 : (1 << TAIL); }
    static constexpr int ns(int p) { return p == 0 ? 1 : ns(p - 1) * radix(p - 1); }
    // twiddle table: passes 1 .. NP-1, each radix(p) rows of ns(p) entries
    static constexpr int tw_off(int p) { return p <= 1 ? 0 : tw_off(p - 1) + radix(p - 1) * ns(p - 1); }
    static constexpr int tw_words() { return tw_off(NP); }
    static constexpr int THREADS = T < 256 ? 256 : T;
    static constexpr int CPB = THREADS / T;                // columns per workgroup
    static constexpr int LDS_COL = N + N / 16;             // padded elements per column
};

#ifdef STARKHIP_LDE_FULL_BARRIER
__device__ __forceinline__ void lde_lds_barrier() { __syncthreads(); }
#else
__device__ __forceinline__ void lde_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#endif

// ---------------------------------------------------------------- host side: the inter-pass twiddles of LdePlan<LOGN>, [i][j mod Ns] per pass
template <int LOGN>
inline void fill_tw(std::vector<gl_t>& out, bool inv) {
    using PL = LdePlan<LOGN>;
    out.assign(PL::tw_words() ? PL::tw_words() : 1, 1);
    const gl_t ninv = gl_inv((gl_t)PL::N);
    if (PL::NP == 1) out[0] = inv ? ninv : 1;
    for (int p = 1; p < PL::NP; p++) {
        const int R = PL::radix(p), NS = PL::ns(p);
        gl_t w = gl_root_of_unity(ilog2_c(NS * R));
        if (inv) w = gl_inv(w);
        const gl_t scale = (inv && p == PL::NP - 1) ? ninv : 1;
        for (int i = 0; i < R; i++) {
            const gl_t wi = gl_pow(w, i);
            gl_t acc = scale;
            for (int jj = 0; jj < NS; jj++) {
                out[PL::tw_off(p) + i * NS + jj] = acc;
                acc = gl_mul(acc, wi);
            }
        }
    }
}

}  // namespace starkhip
