// Transforms of 2^14 .. 2^26 points: trace-column IFFT + coset LDE for long traces (the same function as kernels_lde.hip: plonky2's
// PolynomialBatch::from_values / from_coeffs) and the few long vectors of a proof (the quotient's inverse coset
// transform, the FRI polynomial's layers) that kernels_ntt.hip's one-workgroup kernel would take seconds for.
//
// A column of that length does not fit one workgroup's LDS, so the index is split, n = A * B with A = 2^a, B = 2^b, a = floor(log n / 2),
// b = log n - a, both in 7 .. 13 (tools/lde_long_model.py is the executable specification of everything below).  A tile is W adjacent words
// wide: W = 16, one 128-byte line, for sub-transforms of up to 2^10 points -- every length up to 2^20, so every trace column --, and 8, 4, 2
// words for 2^11, 2^12, 2^13 points (a tile of M points is M W words of LDS, at most 2^14): the vectors of 2^21 .. 2^26 words that
// proofs of the longest traces have (the quotient's n 2^qdb values, the FRI polynomial's N) move in runs of 64, 32 or 16 bytes.
//
//     X[k1 + A k0] = sum_j0 w_B^(j0 k0) * ( w_n^(j0 k1) * sum_j1 w_A^(j1 k1) x[j1 B + j0] )
//
//   pass 1  A-point transforms over j1 (stride B in memory), one workgroup per TILE of 16 adjacent j0: element (p = j1, w = j0 - j0base).
//           A workgroup reads A runs of 16 words (128 B, one cache line each), and writes its result TRANSPOSED, Y'[j0][k1] at j0 A + k1:
//           16 runs of A consecutive words.  The optional pre-scale (the coset powers (7 w_N^s)^j, a FRI layer's shift powers) is applied
//           to the words as they are read.
//   pass 2  B-point transforms over j0, one workgroup per tile of 16 adjacent k1: element (p = j0, w = k1 - k1base) at p A + k1 -- again
//           B runs of 16 words in, and B runs of 16 words out at k0 A + k1, which is the natural order of X.  The inter-pass twiddles
//           w_n^(-+j0 k1) (a table of n words laid out like the data, [j0][k1]; the inverse's n^-1 = A^-1 B^-1 is in the sub-transforms'
//           own inverse tables, not here) are applied to the words as they are read; the optional post-scale to the results.  A workgroup reads and writes the same addresses, so the
//           pass may run in place.
//
// Inside a workgroup the 16 side-by-side transforms are Stockham radix-16 passes exactly as in lde_columns_v2_kernel (LdePlan<LOGM>, the
// register sub-transforms of lde_radix.h), but the LDS image is [point][W].  With W = 16 the 16 lanes that share a point index hold the 16
// adjacent words of a line, so every exchange access of a 16-lane group is one 128-byte row (conflict-free for ds_write_b64, whose banks
// repeat every 128 B) and the two rows a 32-lane half reads are consecutive (conflict-free for ds_read_b64, 256 B).  With W < 16 the reads
// stay conflict-free (32 lanes read 256 consecutive bytes) and the scattered writes of a 16-lane group, 16 / W rows a multiple of 128 B
// apart, are 16 / W-way conflicts (the model counts them).  Pass 1's transposed write-out goes through a second image [W][M + 1].
//
// Per column and transform a word makes one more round trip than in the resident kernels: 8 * 4 n bytes for the inverse transform and
// 8 * 4 n per coset (+ the two tables, shared by all columns of a launch: the grid is ordered column-fastest so that they stay in L2).
#include <hip/hip_runtime.h>

#include <atomic>
#include <vector>

#include "gl_dev.h"
#include "kernels.h"
#include "lde_radix.h"

namespace starkhip {

static constexpr unsigned LONG_MIN_LOG = 14, LONG_MAX_LOG = 26, LONG_MIN_SUB = 7, LONG_MAX_SUB = 13;
// words of a tile row of M = 2^LOGM points: one 128-byte line while M W <= 2^14 words of LDS allow it
constexpr int long_log_w(int logm) { return logm <= 10 ? 4 : 14 - logm; }

// sub-transform twiddle tables (fill_tw<LOGM>), forward then inverse, LOGM = 7 .. 13 back to back
template <int LOGM>
constexpr size_t long_sub_off() {
    if constexpr (LOGM == (int)LONG_MIN_SUB) return 0;
    else return long_sub_off<LOGM - 1>() + 2 * (size_t)LdePlan<LOGM - 1>::tw_words();
}
size_t lde_long_sub_words() { return long_sub_off<LONG_MAX_SUB>() + 2 * (size_t)LdePlan<LONG_MAX_SUB>::tw_words(); }

// One Stockham pass of W side-by-side M-point transforms; thread (q, w) holds points q + i T of transform w.  As lde_pass
// (kernels_lde.hip) with the image [point][W].
template <int LOGM, int P, bool INV>
__device__ __forceinline__ void long_pass(gl_t (&v)[16], gl_t* __restrict__ lds, const gl_t* __restrict__ tw, int q, int w) {
    using PL = LdePlan<LOGM>;
    constexpr int LONG_W = 1 << long_log_w(LOGM);
    constexpr int R = PL::radix(P), S = 16 / R, NS = PL::ns(P), T = PL::T;
    constexpr bool LAST = P == PL::NP - 1;
    if constexpr (P > 0) {
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = lds[(q + i * T) * LONG_W + w];
        constexpr int TW_OFF = PL::tw_off(P);
#pragma unroll
        for (int m = 0; m < S; m++) {
            const int jj = (q + m * T) % NS;
#pragma unroll
            for (int i = (INV && LAST) ? 0 : 1; i < R; i++) v[m + S * i] = gl_mul_nc(v[m + S * i], tw[TW_OFF + i * NS + jj]);
        }
    }
    SubNtts<R, INV, 0>::run(v);
    unscramble<R>(v);
    if constexpr (!LAST) {
        lde_lds_barrier();  // every thread has read its inputs
#pragma unroll
        for (int m = 0; m < S; m++) {
            const int j = q + m * T;
            const int base = (j / NS) * NS * R + (j % NS);
#pragma unroll
            for (int k = 0; k < R; k++) lds[(base + k * NS) * LONG_W + w] = v[m + S * k];
        }
        lde_lds_barrier();
    }
}
template <int LOGM, int P, bool INV>
__device__ __forceinline__ void long_passes(gl_t (&v)[16], gl_t* lds, const gl_t* tw, int q, int w) {
    long_pass<LOGM, P, INV>(v, lds, tw, q, w);
    if constexpr (P + 1 < LdePlan<LOGM>::NP) long_passes<LOGM, P + 1, INV>(v, lds, tw, q, w);
}

// grid (vector, tile, z): vector v of slice z is read at src + v * src_stride (+ pre-scale pre[z n + j]) and written at
// dst + v * dst_stride + z * n.  src and dst must not overlap.
template <int LOGA, bool INV>
__global__ __launch_bounds__(1 << (LOGA - 4 + long_log_w(LOGA))) void lde_long_pass1_kernel(const gl_t* __restrict__ src, size_t src_stride, gl_t* __restrict__ dst,
                                                                    size_t dst_stride, unsigned log_b, const gl_t* __restrict__ pre,
                                                                    const gl_t* __restrict__ tw_sub) { STARKHIP_PRIO_ENTRY
    constexpr int A = 1 << LOGA, T = A / 16, LOG_W = long_log_w(LOGA), LONG_W = 1 << LOG_W, THREADS = T * LONG_W;
    extern __shared__ gl_t lds[];  // W * (A + 1) words
    const int w = threadIdx.x & (LONG_W - 1), q = threadIdx.x >> LOG_W;
    const size_t n = (size_t)A << log_b;
    const size_t j0base = (size_t)blockIdx.y * LONG_W;
    const gl_t* in = src + (size_t)blockIdx.x * src_stride + j0base + w;
    const gl_t* pz = pre ? pre + (size_t)blockIdx.z * n + j0base + w : nullptr;
    gl_t v[16];
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = in[(size_t)(q + i * T) << log_b];
    if (pz) {
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = gl_mul_nc(v[i], pz[(size_t)(q + i * T) << log_b]);
    }
    long_passes<LOGA, 0, INV>(v, lds, tw_sub, q, w);
    // v[i] = Y[k1 = q + i T] of j0 = j0base + w; transposed through the second image [w][A + 1]
    lde_lds_barrier();  // the last exchange image has been read
#pragma unroll
    for (int i = 0; i < 16; i++) lds[w * (A + 1) + q + i * T] = v[i];
    lde_lds_barrier();
    // the tile's W runs of A words back to back: word e = r A + k1 of them, 16 per thread, adjacent lanes on adjacent words
    gl_t* out = dst + (size_t)blockIdx.x * dst_stride + (size_t)blockIdx.z * n + j0base * A;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int e = (int)threadIdx.x + i * THREADS;
        out[e] = lds[(e >> LOGA) * (A + 1) + (e & (A - 1))];
    }
}

// grid (vector, tile, z): vector v of slice z at src + v * src_stride + z * n -> dst + v * dst_stride + z * n (may be the same words)
template <int LOGB, bool INV>
__global__ __launch_bounds__(1 << (LOGB - 4 + long_log_w(LOGB))) void lde_long_pass2_kernel(const gl_t* src, size_t src_stride, gl_t* dst, size_t dst_stride, unsigned log_a,
                                                                    const gl_t* __restrict__ tw, const gl_t* __restrict__ post,
                                                                    const gl_t* __restrict__ tw_sub) { STARKHIP_PRIO_ENTRY
    constexpr int B = 1 << LOGB, T = B / 16, LOG_W = long_log_w(LOGB), LONG_W = 1 << LOG_W;
    extern __shared__ gl_t lds[];  // B * W words
    const int w = threadIdx.x & (LONG_W - 1), q = threadIdx.x >> LOG_W;
    const size_t n = (size_t)B << log_a;
    const size_t off = (size_t)blockIdx.y * LONG_W + w;  // k1
    const gl_t* in = src + (size_t)blockIdx.x * src_stride + (size_t)blockIdx.z * n + off;
    gl_t v[16];
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = in[(size_t)(q + i * T) << log_a];
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = gl_mul_nc(v[i], tw[((size_t)(q + i * T) << log_a) + off]);
    long_passes<LOGB, 0, INV>(v, lds, tw_sub, q, w);
    gl_t* out = dst + (size_t)blockIdx.x * dst_stride + (size_t)blockIdx.z * n + off;
    if (post) {
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = gl_mul_nc(v[i], post[((size_t)(q + i * T) << log_a) + off]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[(size_t)(q + i * T) << log_a] = gl_canon(v[i]);
}

// tw[j0 A + k1] = scale * root^(j0 k1), n = A * B words
__global__ void lde_long_twiddle_kernel(gl_t* out, unsigned log_n, unsigned log_a, gl_t root, gl_t scale) { STARKHIP_PRIO_ENTRY
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= ((size_t)1 << log_n)) return;
    const uint64_t j0 = i >> log_a, k1 = i & (((size_t)1 << log_a) - 1);
    out[i] = gl_mul(scale, gl_pow(root, j0 * k1));
}

// ---------------------------------------------------------------- host side
bool lde_long_supported(unsigned log_n) { return log_n >= LONG_MIN_LOG && log_n <= LONG_MAX_LOG; }
static unsigned long_log_a(unsigned log_n) { return log_n / 2; }

template <int LOGM>
static void long_fill_sub(std::vector<gl_t>& tab) {
    std::vector<gl_t> t;
    for (int inv = 0; inv < 2; inv++) {
        fill_tw<LOGM>(t, inv != 0);
        std::copy(t.begin(), t.begin() + LdePlan<LOGM>::tw_words(), tab.begin() + long_sub_off<LOGM>() + (size_t)inv * LdePlan<LOGM>::tw_words());
    }
}
hipError_t lde_long_upload_sub_tables(gl_t* d_sub, hipStream_t st) {
    std::vector<gl_t> tab(lde_long_sub_words());
    long_fill_sub<7>(tab);
    long_fill_sub<8>(tab);
    long_fill_sub<9>(tab);
    long_fill_sub<10>(tab);
    long_fill_sub<11>(tab);
    long_fill_sub<12>(tab);
    long_fill_sub<13>(tab);
    hipError_t e = hipMemcpyAsync(d_sub, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);  // the host vector goes out of scope
}
// the inter-pass tables of one length, n words each: forward w_n^(j0 k1), inverse w_n^(-j0 k1) -- the sub-transforms' inverse tables
// carry A^-1 and B^-1, so the inverse table here carries no n^-1
hipError_t lde_long_fill_twiddles(gl_t* d_fwd, gl_t* d_inv, unsigned log_n, hipStream_t st) {
    if (!lde_long_supported(log_n)) return hipErrorInvalidValue;
    const gl_t w = gl_root_of_unity(log_n);
    const unsigned blocks = (unsigned)((((size_t)1 << log_n) + 255) / 256);
    hipLaunchKernelGGL(lde_long_twiddle_kernel, dim3(blocks), dim3(256), 0, st, d_fwd, log_n, long_log_a(log_n), w, (gl_t)1);
    hipLaunchKernelGGL(lde_long_twiddle_kernel, dim3(blocks), dim3(256), 0, st, d_inv, log_n, long_log_a(log_n), gl_inv(w), (gl_t)1);
    return hipGetLastError();
}

// more than 64 KB of dynamic LDS has to be allowed once per device and kernel: `fn` is one kernel's, `done` that kernel's device mask
static hipError_t long_allow_lds(const void* fn, size_t lds_bytes, std::atomic<uint64_t>& done) {
    if (lds_bytes <= 64 * 1024) return hipSuccess;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    if (hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes); e != hipSuccess) return e;
    done.fetch_or(bit, std::memory_order_release);
    return hipSuccess;
}

template <int LOGM>
static const gl_t* long_sub(const gl_t* d_sub, bool inv) { return d_sub + long_sub_off<LOGM>() + (inv ? LdePlan<LOGM>::tw_words() : 0); }

template <int LOGA, bool INV>
static hipError_t long_launch_pass1(const gl_t* src, size_t src_stride, gl_t* dst, size_t dst_stride, size_t n_vecs, unsigned n_z, unsigned log_b,
                                    const gl_t* pre, const gl_t* d_sub, hipStream_t st) {
    constexpr int LOG_W = long_log_w(LOGA);
    constexpr size_t lds_bytes = ((size_t)((1 << LOGA) + 1) << LOG_W) * sizeof(gl_t);
    static std::atomic<uint64_t> allowed(0);
    if (hipError_t e = long_allow_lds((const void*)lde_long_pass1_kernel<LOGA, INV>, lds_bytes, allowed); e != hipSuccess) return e;
    if (log_b < (unsigned)LOG_W || log_b - LOG_W > 15) return hipErrorInvalidValue;  // tiles are the grid's y: at most 65535
    hipLaunchKernelGGL((lde_long_pass1_kernel<LOGA, INV>), dim3((unsigned)n_vecs, 1u << (log_b - LOG_W), n_z), dim3(1 << (LOGA - 4 + LOG_W)), lds_bytes, st, src, src_stride,
                       dst, dst_stride, log_b, pre, long_sub<LOGA>(d_sub, INV));
    return hipGetLastError();
}
template <int LOGB, bool INV>
static hipError_t long_launch_pass2(const gl_t* src, size_t src_stride, gl_t* dst, size_t dst_stride, size_t n_vecs, unsigned n_z, unsigned log_a,
                                    const gl_t* tw, const gl_t* post, const gl_t* d_sub, hipStream_t st) {
    constexpr int LOG_W = long_log_w(LOGB);
    constexpr size_t lds_bytes = ((size_t)1 << (LOGB + LOG_W)) * sizeof(gl_t);
    static std::atomic<uint64_t> allowed(0);
    if (hipError_t e = long_allow_lds((const void*)lde_long_pass2_kernel<LOGB, INV>, lds_bytes, allowed); e != hipSuccess) return e;
    if (log_a < (unsigned)LOG_W || log_a - LOG_W > 15) return hipErrorInvalidValue;
    hipLaunchKernelGGL((lde_long_pass2_kernel<LOGB, INV>), dim3((unsigned)n_vecs, 1u << (log_a - LOG_W), n_z), dim3(1 << (LOGB - 4 + LOG_W)), lds_bytes, st, src, src_stride,
                       dst, dst_stride, log_a, tw, post, long_sub<LOGB>(d_sub, INV));
    return hipGetLastError();
}

// One transform of n_z slices of n_vecs vectors in two launches: src (+ pre[z]) -> mid[z] -> dst[z].  mid must not overlap src; dst may be
// mid (in place) or src.  Slices lie n words apart inside a vector's stride in mid and dst.
static hipError_t long_transform(const gl_t* src, size_t src_stride, gl_t* mid, size_t mid_stride, gl_t* dst, size_t dst_stride, size_t n_vecs,
                                 unsigned n_z, unsigned log_n, bool inverse, const gl_t* pre, const gl_t* post, const LdeLongTables& tb,
                                 hipStream_t st) {
    if (!lde_long_supported(log_n) || n_vecs == 0 || n_vecs > 0x7fffffffu || n_z == 0 || n_z > 65535) return hipErrorInvalidValue;
    const unsigned a = long_log_a(log_n), b = log_n - a;
    if (a < LONG_MIN_SUB || b > LONG_MAX_SUB) return hipErrorInvalidValue;
    const gl_t* tw = inverse ? tb.tw_inv : tb.tw_fwd;
    hipError_t e = hipErrorInvalidValue;
#define P1(L) case L: e = inverse ? long_launch_pass1<L, true>(src, src_stride, mid, mid_stride, n_vecs, n_z, b, pre, tb.sub, st) \
                                  : long_launch_pass1<L, false>(src, src_stride, mid, mid_stride, n_vecs, n_z, b, pre, tb.sub, st); break;
    switch (a) { P1(7) P1(8) P1(9) P1(10) P1(11) P1(12) P1(13) default: break; }
#undef P1
    if (e != hipSuccess) return e;
    e = hipErrorInvalidValue;
#define P2(L) case L: e = inverse ? long_launch_pass2<L, true>(mid, mid_stride, dst, dst_stride, n_vecs, n_z, a, tw, post, tb.sub, st) \
                                  : long_launch_pass2<L, false>(mid, mid_stride, dst, dst_stride, n_vecs, n_z, a, tw, post, tb.sub, st); break;
    switch (b) { P2(7) P2(8) P2(9) P2(10) P2(11) P2(12) P2(13) default: break; }
#undef P2
    return e;
}

hipError_t launch_ntt_long(const gl_t* src, gl_t* mid, gl_t* dst, size_t n_vecs, size_t vec_stride, unsigned log_n, bool inverse, const gl_t* pre_scale,
                           const gl_t* post_scale, const LdeLongTables& tb, hipStream_t st) {
    if (n_vecs == 0) return hipSuccess;
    return long_transform(src, vec_stride, mid, vec_stride, dst, vec_stride, n_vecs, 1, log_n, inverse, pre_scale, post_scale, tb, st);
}

// values [C][n] -> coefficients coeffs [C][n] -> lde [C][2^rate][n], coset-major; from_coeffs: `values` holds the coefficients and `coeffs` is
// not used.  `coeffs` is required otherwise (it is the transforms' own scratch as well: the prover passes its `values` buffer) and may
// be `values` itself; neither may overlap `lde`.  cs[s][j] = (7 w_N^s)^j.  No closed forms for constant / unit-vector columns here.
hipError_t launch_lde_columns_long(const gl_t* values, gl_t* coeffs, gl_t* lde, size_t n_cols, unsigned log_n, unsigned rate_bits, const LdeLongTables& tb,
                                   const gl_t* cs, int from_coeffs, hipStream_t st) {
    if (n_cols == 0) return hipSuccess;
    if (!from_coeffs && !coeffs) return hipErrorInvalidValue;
    const size_t n = (size_t)1 << log_n, N = n << rate_bits;
    if (!from_coeffs) {  // inverse: values -> (coset slot 0 of the column's LDE block) -> coeffs
        hipError_t e = long_transform(values, n, lde, N, coeffs, n, n_cols, 1, log_n, true, nullptr, nullptr, tb, st);
        if (e != hipSuccess) return e;
    }
    return long_transform(from_coeffs ? values : coeffs, n, lde, N, lde, N, n_cols, 1u << rate_bits, log_n, false, cs, nullptr, tb, st);
}

}  // namespace starkhip
