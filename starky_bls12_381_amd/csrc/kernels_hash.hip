// Poseidon-Goldilocks hashing kernels for gfx950: Merkle leaf digests over the coset-major LDE,
// 2-to-1 compression levels, proof-of-work grinding and a raw permutation batch for tests.
// Restates plonky2 MerkleTree::new / hash_or_noop / two_to_one, which the
// reference reaches through prove() at /root/reference/src/aggregate_proof.rs:59.
#include <hip/hip_runtime.h>

#include <mutex>

#include "kernels.h"
#include "poseidon_dev.h"
#include "verify_query.h"

namespace starkhip {

// ---- the host-built tables (poseidon_tables.h), one image per device in constant memory; each symbol with its own upload flags
__constant__ QuadMergedTables QUAD_MERGED;
__constant__ RowMergedTables ROW_MERGED;
static bool quad_uploaded[64], row_uploaded[64], lane_uploaded[64], pair_uploaded[64];

// Leaf digests of a column-major matrix laid out coset-major (see kernels_ntt.hip):
//   element (column c, physical point q) at mat[c * N + q], q = s * n + k  <->  natural index i = k * R + s.
// Leaf position j in the tree holds natural row bitrev_logN(j) (plonky2 reverse_index_bits_in_place),
// so the thread that owns physical point q writes digest slot j = bitrev(i).
// Four lanes (one DPP quad) walk one row; adjacent quads read adjacent k => each load touches whole 128-byte runs.
__device__ __forceinline__ void leaf_hash_body(const gl_t* __restrict__ mat, size_t n_cols, unsigned log_n, unsigned rate_bits,
                                               gl_t* __restrict__ digests) {
    // lane l of the quad owns sponge state elements l, l + 4, l + 8 (poseidon_dev.h)
    __shared__ RcPair rcs[4][96];  // per-lane view of the round constants, split in halves, + 3 zeros ("next round" of the last round)
    for (unsigned idx = threadIdx.x; idx < 4 * 96; idx += blockDim.x) {
        const unsigned ll = idx / 96, w = idx % 96;
        const gl_t c = w < 90 ? POSEIDON_RC_DEV[12 * (w / 3) + ll + 4 * (w % 3)] : 0;
        rcs[ll][w].lo = c & 0xFFFFFFFFull;
        rcs[ll][w].hi = c >> 32;
    }
    __shared__ RcPair tks[2 * QUAD_MERGED_TRIPLES];
    __shared__ RcPair tk3s[4][3 * QUAD_MERGED_TRIPLES];
    for (unsigned idx = threadIdx.x; idx < 2 * QUAD_MERGED_TRIPLES; idx += blockDim.x) tks[idx] = QUAD_MERGED.tk[idx];
    for (unsigned idx = threadIdx.x; idx < 4 * 3 * QUAD_MERGED_TRIPLES; idx += blockDim.x)
        tk3s[idx / (3 * QUAD_MERGED_TRIPLES)][idx % (3 * QUAD_MERGED_TRIPLES)] = QUAD_MERGED.tk3[idx / (3 * QUAD_MERGED_TRIPLES)][idx % (3 * QUAD_MERGED_TRIPLES)];
    __syncthreads();
    const unsigned log_N = log_n + rate_bits;
    const size_t N = (size_t)1 << log_N;
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const unsigned l = (unsigned)tid & 3u;
    const size_t q = tid >> 2;
    if (q >= N) return;  // whole quads drop out together
    const size_t s = q >> log_n, k = q & (((size_t)1 << log_n) - 1);
    const size_t i = (k << rate_bits) + s;
    const size_t j = gl_bitrev((uint32_t)i, log_N);
    const gl_t* col = mat + q;
    if (n_cols <= 4) {  // hash_or_noop: short leaves are copied, zero padded
        digests[4 * j + l] = l < n_cols ? col[(size_t)l * N] : 0;
        return;
    }
    const uint32_t diag0 = l == 0 ? 8u : 0u;
    const RcPair* rc = rcs[l];
    QuadMergedCoef mc;
    {
        const uint32_t* c = QUAD_MERGED.coef[l];
#pragma unroll
        for (int e = 0; e < 36; e++) mc.n3[e / 12][e % 12] = c[e];
#pragma unroll
        for (int e = 0; e < 3; e++) {
            mc.n1[e] = c[36 + e];
            mc.n2[e] = c[39 + e];
            mc.b2[e] = c[43 + e];
            mc.b3[e] = c[46 + e];
        }
        mc.m00 = c[42];
#pragma unroll
        for (int e = 0; e < 12; e++) mc.cf[e] = c[50 + e];
    }
    const RcPair* tk3 = tk3s[l];
    const bool even_lane = (l & 1u) == 0;
    gl_t s0 = 0, s1 = 0, s2 = 0;
    // Overwrite-mode sponge, rate 8: block b overwrites state elements 0 .. 7 = slots 0 and 1 of the four lanes with columns
    // 8 b + l and 8 b + l + 4.  The next block's two cells are requested before the current permutation (about 10 us of
    // arithmetic) so that their latency -- column stride N * 8 bytes, a new page per load -- is never waited for with only two
    // waves per SIMD.  A permutation that is followed by another full block computes only the capacity in its last layer.
    const gl_t* mine = col + (size_t)l * N;
    const size_t n_full = n_cols / 8, rem = n_cols % 8;
    gl_t n0 = 0, n1 = 0;
    if (n_full) {
        n0 = mine[0];
        n1 = mine[4 * N];
    }
    for (size_t b = 0; b < n_full; b++) {
        s0 = n0;
        s1 = n1;
        if (b + 1 < n_full) {
            n0 = mine[(8 * (b + 1)) * N];
            n1 = mine[(8 * (b + 1) + 4) * N];
            poseidon_permute_quad_merged<true>(s0, s1, s2, diag0, rc, mc, tks, tk3, l == 0, even_lane);
        } else {
            poseidon_permute_quad_merged<false>(s0, s1, s2, diag0, rc, mc, tks, tk3, l == 0, even_lane);
        }
    }
    if (rem) {  // the last, partial block overwrites elements 0 .. rem - 1 only
        const size_t off = 8 * n_full;
        if (l < rem) s0 = mine[off * N];
        if (l + 4 < rem) s1 = mine[(off + 4) * N];
        poseidon_permute_quad_merged<false>(s0, s1, s2, diag0, rc, mc, tks, tk3, l == 0, even_lane);
    }
    digests[4 * j + l] = gl_canon(s0);  // digest = state elements 0 .. 3: slot 0 of the four lanes
}

__global__ __launch_bounds__(256) void leaf_hash_kernel(const gl_t* __restrict__ mat, size_t n_cols, unsigned log_n, unsigned rate_bits,
                                                         gl_t* __restrict__ digests) { STARKHIP_PRIO_ENTRY
    leaf_hash_body(mat, n_cols, log_n, rate_bits, digests);
}

// The same over K matrices of ONE shape in one launch (grid.y = matrix): the commitments of K proofs of the same AIR.  A
// 1024-row AIR has 2048 .. 4096 leaves, i.e. 128 .. 256 waves of up to 12 167 sequential permutations each -- a latency chain
// that leaves 7/8 of the chip idle; K of them side by side fill it (scheduler.hip gathers them).
__global__ __launch_bounds__(256) void leaf_hash_multi_kernel(LeafHashBatch B, size_t n_cols, unsigned log_n, unsigned rate_bits) { STARKHIP_PRIO_ENTRY
    leaf_hash_body(B.mat[blockIdx.y], n_cols, log_n, rate_bits, B.digests[blockIdx.y]);
}

// [lane of the row][entry]: entries 0 .. 31 the round constants (zero beyond round 29), 32 + 3 t + {0, 1, 2} the merged triples' k1, k2
// (lane 0 only) and k3; everything zero on lanes 12 .. 15.  Filled by the whole block; the caller synchronises.
__device__ __forceinline__ void row_rcs_fill(RcPair (*rcs)[64]) {
    for (unsigned idx = threadIdx.x; idx < 16 * 64; idx += blockDim.x) {
        const unsigned e = idx / 64, r = idx % 64;
        RcPair c = {0, 0};
        if (e < 12 && r < 30) {
            const gl_t v = POSEIDON_RC_DEV[12 * r + e];
            c.lo = v & 0xFFFFFFFFull;
            c.hi = v >> 32;
        } else if (e < 12 && r >= 32 && r < 32 + 3 * 7) {
            const unsigned t = (r - 32) / 3, w = (r - 32) % 3;
            if (w == 2) c = ROW_MERGED.k3[t][e];
            else if (e == 0) c = w == 0 ? ROW_MERGED.k1[t] : ROW_MERGED.k2[t];
        }
        rcs[e][r] = c;
    }
}

// ---- the row form (poseidon_dev.h): 16 lanes per leaf, for commitments whose quad launch would leave most of the chip idle.
// Same digests as leaf_hash_kernel.  Lane e < 8 of a row absorbs column 8 b + e of block b (the rate), lanes 8 .. 11 carry the
// capacity, lanes 12 .. 15 idle as mirrors.  One wave = 4 leaves; adjacent rows read adjacent points of a column.
__global__ __launch_bounds__(256) void leaf_hash_row_kernel(const gl_t* __restrict__ mat, size_t n_cols, unsigned log_n, unsigned rate_bits,
                                                             gl_t* __restrict__ digests) { STARKHIP_PRIO_ENTRY
    __shared__ RcPair rcs[16][64];
    row_rcs_fill(rcs);
    __syncthreads();
    const unsigned log_N = log_n + rate_bits;
    const size_t N = (size_t)1 << log_N;
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const unsigned e = (unsigned)tid & 15u;
    const size_t q = tid >> 4;
    if (q >= N) return;  // whole rows drop out together
    const size_t sidx = q >> log_n, k = q & (((size_t)1 << log_n) - 1);
    const size_t i = (k << rate_bits) + sidx;
    const size_t j = gl_bitrev((uint32_t)i, log_N);
    const gl_t* col = mat + q;
    if (n_cols <= 4) {  // hash_or_noop: short leaves are copied, zero padded
        if (e < 4) digests[4 * j + e] = e < n_cols ? col[(size_t)e * N] : 0;
        return;
    }
#ifdef STARKHIP_ROW_CPP_ROUNDS  // the C++ rounds (poseidon_permute_row): what hipcc schedules by itself, kept for comparison
    const uint32_t c0 = e == 0 ? 17u + 8u : 17u;  // CIRC[0] + MDS_MATRIX_DIAG[0] on lane 0
#define STARKHIP_ROW_PERMUTE(s) poseidon_permute_row(s, rc, c0, e == 0)
#else
    RowConsts K;
    row_consts_init(K, e, ROW_MERGED.coef[e]);
#ifdef STARKHIP_ROW_PLAIN_ROUNDS  // asm rounds without the merged triples
#define STARKHIP_ROW_PERMUTE(s) poseidon_permute_row_asm(s, rc, K)
#else
#define STARKHIP_ROW_PERMUTE(s) poseidon_permute_row_merged_asm(s, rc, K)
#endif
#endif
    const RcPair* rc = rcs[e];
    const bool absorbs = e < 8;
    gl_t s = 0;
    const gl_t* mine = col + (size_t)(absorbs ? e : 0) * N;  // lanes 8 .. 15 never load
    const size_t n_full = n_cols / 8, rem = n_cols % 8;
    gl_t nx = 0;
    if (n_full && absorbs) nx = mine[0];
    for (size_t b = 0; b < n_full; b++) {
        if (absorbs) s = nx;
        if (b + 1 < n_full && absorbs) nx = mine[(8 * (b + 1)) * N];  // requested one permutation ahead
        s = STARKHIP_ROW_PERMUTE(s);
    }
    if (rem) {  // the last, partial block overwrites elements 0 .. rem - 1 only
        if (e < rem) s = mine[(8 * n_full) * N];
        s = STARKHIP_ROW_PERMUTE(s);
    }
    if (e < 4) digests[4 * j + e] = gl_canon(s);
#undef STARKHIP_ROW_PERMUTE
}

// ---- the device verifier's leaf digests (verifier_device.cpp): opened leaves of query rounds, contiguous words in the proof, one
// descriptor each (verify_query.h: VQLeaf), hashed in the row form -- the shortest chain per permutation, and a batch has only a few
// thousand long chains.  Lane e < 8 of a row absorbs word 8 b + e of block b, one block ahead; the host sorts the descriptors longest
// first, so the longest chains start first and the waves hold chains of like length.
__global__ __launch_bounds__(256) void verify_leaf_digest_kernel(const gl_t* __restrict__ words, const VQLeaf* __restrict__ leaves, size_t n_leaves,
                                                                  gl_t* __restrict__ digests) { STARKHIP_PRIO_ENTRY
    __shared__ RcPair rcs[16][64];
    row_rcs_fill(rcs);
    __syncthreads();
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const unsigned e = (unsigned)tid & 15u;
    const size_t q = tid >> 4;
    if (q >= n_leaves) return;  // whole rows drop out together
    const VQLeaf lf = leaves[q];
    if (lf.hasher != STARKHIP_HASHER_POSEIDON) return;  // another hasher's leaf: its own kernel takes it (kernels_keccak.hip)
    const gl_t* in = words + lf.off;
    gl_t* out = digests + 4 * (size_t)lf.slot;
    if (lf.len <= 4) {  // hash_or_noop: short leaves are copied, zero padded
        if (e < 4) out[e] = e < lf.len ? in[e] : 0;
        return;
    }
    RowConsts K;
    row_consts_init(K, e, ROW_MERGED.coef[e]);
    const RcPair* rc = rcs[e];
    const bool absorbs = e < 8;
    const gl_t* mine = in + (absorbs ? e : 0);  // lanes 8 .. 15 never load
    const size_t n_full = lf.len / 8, rem = lf.len % 8;
    gl_t s = 0, nx = 0;
    if (n_full && absorbs) nx = mine[0];
    for (size_t b = 0; b < n_full; b++) {
        if (absorbs) s = nx;
        if (b + 1 < n_full && absorbs) nx = mine[8 * (b + 1)];  // requested one permutation ahead
        s = poseidon_permute_row_merged_asm(s, rc, K);
    }
    if (rem) {  // the last, partial block overwrites elements 0 .. rem - 1 only
        if (e < rem) s = mine[8 * n_full];
        s = poseidon_permute_row_merged_asm(s, rc, K);
    }
    if (e < 4) out[e] = gl_canon(s);
}

// ---- the lane form (poseidon_dev.h): one lane per leaf, for big commitments when several are in flight (the pool picks).
// Same digests as leaf_hash_kernel.  64 adjacent points of a column per wave: every load is one 512-byte run.
__constant__ LaneTables LANE_TABLES;
// The first block a leaf absorbs: n / 8 where this commitment may start from the saved state past its identity prefix, else 0.  Uniform
// over the launch's segment: the counter is one word read through a uniform pointer.
__device__ __forceinline__ size_t leaf_prefix_blocks(const unsigned* count, const gl_t* cap, size_t n_cols, unsigned log_n) {
    const size_t n = (size_t)1 << log_n;
    if (count == nullptr || cap == nullptr || n_cols < n + 8) return 0;
    return __builtin_amdgcn_readfirstlane(*count) == (unsigned)n ? n / 8 : 0;
}
// grid.y = commitment (LeafHashBatch, as leaf_hash_multi_kernel): the lane-form group of a proof pool is ONE grid -- four launches on four
// streams occupy four hardware queues for 350 ms each, and with HIP's default of four queues every other stream of the process then waits
// behind one of them (tools/experiments/hw_queue_probe.hip).  The segment's two pointers are looked up once, from the kernel arguments.
__global__ __launch_bounds__(256, 2) void leaf_hash_lane_kernel(LeafHashBatch B, size_t n_cols, unsigned log_n, unsigned rate_bits) {
    const gl_t* __restrict__ mat = B.mat[blockIdx.y];
    gl_t* __restrict__ digests = B.digests[blockIdx.y];
    __shared__ LaneTables T;
    {
        const uint32_t* src = (const uint32_t*)&LANE_TABLES;
        uint32_t* dst = (uint32_t*)&T;
        for (unsigned idx = threadIdx.x; idx < sizeof(LaneTables) / 4; idx += blockDim.x) dst[idx] = src[idx];
    }
    __syncthreads();
    const unsigned log_N = log_n + rate_bits;
    const size_t N = (size_t)1 << log_N;
    // Every lane of a wave stays active to the end: the matrix-pipe rounds read the operand registers of all 64 lanes whatever EXEC
    // says (a lane that left early would feed garbage weights into its partner half's sums).  Lanes beyond the last leaf shadow it.
    const size_t q_raw = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const bool live = q_raw < N;
    const size_t q = live ? q_raw : N - 1;
    const size_t sidx = q >> log_n, k = q & (((size_t)1 << log_n) - 1);
    const size_t i = (k << rate_bits) + sidx;
    const size_t j = gl_bitrev((uint32_t)i, log_N);
    const gl_t* col = mat + q;
    if (n_cols <= 4) {
        if (live)
            for (unsigned e = 0; e < 4; e++) digests[4 * j + e] = e < n_cols ? col[(size_t)e * N] : 0;
        return;
    }
    const size_t n_full = n_cols / 8, rem = n_cols % 8;
    // The saved state past an identity prefix (kernels.h: LeafPrefix): one uniform load decides for the whole grid segment.  With it the
    // leaves start at block n / 8 from the table's capacity; the rate is zero and the first block absorbed overwrites all of it.
    const size_t b0 = leaf_prefix_blocks(B.prefix_count[blockIdx.y], B.prefix_cap[blockIdx.y], n_cols, log_n);
    gl_t nx[8];
    if (n_full) {
#pragma unroll
        for (int e = 0; e < 8; e++) nx[e] = col[(8 * b0 + e) * N];
    }
    LaneZeros Z;
    lane_zeros_init(Z);
    LaneMfma M;
    const unsigned lane = threadIdx.x & 63u;
    lane_mfma_init(M, lane);
    LaneState st;
#pragma unroll
    for (int w = 0; w < 8; w++) st.t0[w] = st.t1[w] = st.t2[w] = 0;
    if (b0) {
        const gl_t* cap = B.prefix_cap[blockIdx.y] + q;
#pragma unroll
        for (int e = 0; e < 4; e++) lane_set(st.t2, e, cap[(size_t)e * N]);
    }
    for (size_t b = b0; b < n_full; b++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            lane_set(st.t0, e, nx[e]);
            lane_set(st.t1, e, nx[4 + e]);
        }
        if (b + 1 < n_full) {
#pragma unroll
            for (int e = 0; e < 8; e++) nx[e] = col[(8 * (b + 1) + e) * N];  // requested one permutation ahead
            poseidon_permute_lane_asm<true>(st, &T, Z, M, lane);
        } else {
            poseidon_permute_lane_asm<false>(st, &T, Z, M, lane);
        }
    }
    if (rem) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if ((size_t)e < rem) lane_set(st.t0, e, col[(8 * n_full + e) * N]);
            if ((size_t)(4 + e) < rem) lane_set(st.t1, e, col[(8 * n_full + 4 + e) * N]);
        }
        poseidon_permute_lane_asm<false>(st, &T, Z, M, lane);
    }
    if (live) {
#pragma unroll
        for (int e = 0; e < 4; e++) digests[4 * j + e] = gl_canon(lane_get(st.t0, e));
    }
}

// ---- the pair form (poseidon_dev.h): two lanes per leaf, for a LONE commitment of >= 32 768 leaves (1 024 waves: one per SIMD).
// Same digests as leaf_hash_kernel.  Lane l < 32 of a wave absorbs columns 8 b .. 8 b + 5 of block b at point 32 w + l, lane l + 32
// columns 8 b + 6, 8 b + 7 of the same point and carries the capacity: every load is a 256-byte run.
__constant__ PairTables PAIR_TABLES;
__global__ __launch_bounds__(256, 2) void leaf_hash_pair_kernel(const gl_t* __restrict__ mat, size_t n_cols, unsigned log_n, unsigned rate_bits,
                                                              gl_t* __restrict__ digests, const unsigned* prefix_count, const gl_t* __restrict__ prefix_cap) {
    __shared__ PairTables T;
    {
        const uint32_t* src = (const uint32_t*)&PAIR_TABLES;
        uint32_t* dst = (uint32_t*)&T;
        for (unsigned idx = threadIdx.x; idx < sizeof(PairTables) / 4; idx += blockDim.x) dst[idx] = src[idx];
    }
    __syncthreads();
    const unsigned log_N = log_n + rate_bits;
    const size_t N = (size_t)1 << log_N;
    const unsigned lane = threadIdx.x & 63u, half = lane >> 5;
    // every lane stays active to the end (the matrix-pipe rounds read all 64 lanes' operand registers); pairs beyond the last leaf shadow it
    const size_t q_raw = (blockIdx.x * (size_t)(blockDim.x >> 6) + (threadIdx.x >> 6)) * 32u + (lane & 31u);
    const bool live = q_raw < N;
    const size_t q = live ? q_raw : N - 1;
    const size_t sidx = q >> log_n, k = q & (((size_t)1 << log_n) - 1);
    const size_t i = (k << rate_bits) + sidx;
    const size_t j = gl_bitrev((uint32_t)i, log_N);
    if (n_cols <= 4) {
        if (live && half == 0)
            for (unsigned e = 0; e < 4; e++) digests[4 * j + e] = e < n_cols ? mat[q + (size_t)e * N] : 0;
        return;
    }
    const size_t n_full = n_cols / 8, rem = n_cols % 8;
    const unsigned first = half ? 6u : 0u;            // this lane's columns inside a block of eight: first .. first + cnt - 1
    const gl_t* col = mat + q + (size_t)first * N;
    const size_t b0 = leaf_prefix_blocks(prefix_count, prefix_cap, n_cols, log_n);  // as in leaf_hash_lane_kernel
    gl_t nx[6];
    if (n_full) {
        const gl_t* nc = col + 8 * b0 * N;
        nx[0] = nc[0];
        nx[1] = nc[N];
        if (half == 0) {
#pragma unroll
            for (int e = 2; e < 6; e++) nx[e] = nc[(size_t)e * N];
        }
    }
    LaneZeros Z;
    lane_zeros_init(Z);
    PairMfma M;
    pair_mfma_init(M, lane);
    uint64_t mask_lo = 0xFFFFFFFFull;
    asm volatile("" : "+s"(mask_lo));
    PairState st;
#pragma unroll
    for (int w = 0; w < 4; w++) st.t0[w] = st.t1[w] = st.t2[w] = 0;
    if (b0 && half) {  // the capacity: the upper lane's elements 2 .. 5
        const gl_t* cap = prefix_cap + q;
        pair_set(st.t1, 0, cap[0]);
        pair_set(st.t1, 1, cap[N]);
        pair_set(st.t2, 0, cap[2 * N]);
        pair_set(st.t2, 1, cap[3 * N]);
    }
    for (size_t b = b0; b < n_full; b++) {
        pair_set(st.t0, 0, nx[0]);
        pair_set(st.t0, 1, nx[1]);
        if (half == 0) {   // the upper lane's elements 2 .. 5 are the capacity
            pair_set(st.t1, 0, nx[2]);
            pair_set(st.t1, 1, nx[3]);
            pair_set(st.t2, 0, nx[4]);
            pair_set(st.t2, 1, nx[5]);
        }
        if (b + 1 < n_full) {
            const gl_t* nc = col + 8 * (b + 1) * N;   // requested one permutation ahead
            nx[0] = nc[0];
            nx[1] = nc[N];
            if (half == 0) {
#pragma unroll
                for (int e = 2; e < 6; e++) nx[e] = nc[(size_t)e * N];
            }
            poseidon_permute_pair_asm<true>(st, &T, Z, M, lane, mask_lo);
        } else {
            poseidon_permute_pair_asm<false>(st, &T, Z, M, lane, mask_lo);
        }
    }
    if (rem) {
        const gl_t* nc = col + 8 * n_full * N;
        const unsigned cnt = half ? 2u : 6u;
#pragma unroll
        for (unsigned e = 0; e < 6; e++) {
            if (e < cnt && first + e < rem) {
                const gl_t x = nc[(size_t)e * N];
                if (e < 2) pair_set(st.t0, e, x);
                else if (e < 4) pair_set(st.t1, e - 2, x);
                else pair_set(st.t2, e - 4, x);
            }
        }
        poseidon_permute_pair_asm<false>(st, &T, Z, M, lane, mask_lo);
    }
    if (live && half == 0) {
        digests[4 * j + 0] = gl_canon(pair_get(st.t0, 0));
        digests[4 * j + 1] = gl_canon(pair_get(st.t0, 1));
        digests[4 * j + 2] = gl_canon(pair_get(st.t1, 0));
        digests[4 * j + 3] = gl_canon(pair_get(st.t1, 1));
    }
}

// Leaves stored row-major and already in tree order: leaf j = rows[j][0..width)
__global__ __launch_bounds__(64) void leaf_hash_rows_kernel(const gl_t* __restrict__ rows, size_t width, size_t n_leaves,
                                                             gl_t* __restrict__ digests) { STARKHIP_PRIO_ENTRY
    size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n_leaves) return;
    gl_t out[4];
    poseidon_hash_or_noop_dev(rows + j * width, width, 1, out);
#pragma unroll
    for (int e = 0; e < 4; e++) digests[4 * j + e] = out[e];
}

__global__ __launch_bounds__(64) void merkle_level_kernel(const gl_t* __restrict__ child, gl_t* __restrict__ parent, size_t n_parent) { STARKHIP_PRIO_ENTRY
    size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n_parent) return;
    gl_t out[4];
    poseidon_two_to_one_dev(child + 8 * j, child + 8 * j + 4, out);
#pragma unroll
    for (int e = 0; e < 4; e++) parent[4 * j + e] = out[e];
}

__global__ void permute_batch_kernel(gl_t* states, size_t n) { STARKHIP_PRIO_ENTRY
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    gl_t s[12];
#pragma unroll
    for (int e = 0; e < 12; e++) s[e] = states[12 * i + e];
    poseidon_permute_dev(s);
#pragma unroll
    for (int e = 0; e < 12; e++) states[12 * i + e] = s[e];
}

// ---- test entry points (starkhip_poseidon_permute_batch_form): the permutation of each leaf-hash form on WHOLE 12-word states, so that a
// test can place any value at any round of it (a sponge fixes the capacity of its first block).  Each kernel takes its leaf kernel's launch
// bounds and table staging, loads state q into the form's register layout, calls the function the leaf kernel calls and writes the canonical
// words to out + 12 q.  Every lane stays active to the end; lanes beyond the last state shadow it (as leaf_hash_lane_kernel does) and write
// nothing.  CAP_ONLY variants compute only part of the state in their last round: the words they are not specified to produce are written
// as the INPUT words, and a test compares the others.
//
// (The quad form's entry point is kernels_hash_quad_form.hip: see there why it is a translation unit of its own.)
//
// Row form: lane e < 12 of a row of 16 holds word e, lanes 12 .. 15 start from zero as in the leaf kernel (mirrors, never read).
__global__ __launch_bounds__(256) void permute_row_form_kernel(const gl_t* __restrict__ in, gl_t* __restrict__ out, size_t n) { STARKHIP_PRIO_ENTRY
    __shared__ RcPair rcs[16][64];
    row_rcs_fill(rcs);
    __syncthreads();
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const unsigned e = (unsigned)tid & 15u;
    const bool live = (tid >> 4) < n;
    const size_t q = live ? tid >> 4 : n - 1;
    RowConsts K;
    row_consts_init(K, e, ROW_MERGED.coef[e]);
    gl_t s = e < 12 ? in[12 * q + e] : 0;
    s = poseidon_permute_row_merged_asm(s, rcs[e], K);
    if (live && e < 12) out[12 * q + e] = gl_canon(s);
}

// Lane form: one lane per state, words 0 .. 3 / 4 .. 7 / 8 .. 11 in the three tuples.  CAP_ONLY specifies words 8 .. 11 (st.t2).
template <bool CAP_ONLY>
__global__ __launch_bounds__(256, 2) void permute_lane_form_kernel(const gl_t* __restrict__ in, gl_t* __restrict__ out, size_t n) {
    __shared__ LaneTables T;
    {
        const uint32_t* src = (const uint32_t*)&LANE_TABLES;
        uint32_t* dst = (uint32_t*)&T;
        for (unsigned idx = threadIdx.x; idx < sizeof(LaneTables) / 4; idx += blockDim.x) dst[idx] = src[idx];
    }
    __syncthreads();
    const size_t q_raw = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const bool live = q_raw < n;
    const gl_t* mine = in + 12 * (live ? q_raw : n - 1);
    LaneZeros Z;
    lane_zeros_init(Z);
    LaneMfma M;
    const unsigned lane = threadIdx.x & 63u;
    lane_mfma_init(M, lane);
    LaneState st;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        lane_set(st.t0, e, mine[e]);
        lane_set(st.t1, e, mine[4 + e]);
        lane_set(st.t2, e, mine[8 + e]);
    }
    poseidon_permute_lane_asm<CAP_ONLY>(st, &T, Z, M, lane);
    if (!live) return;
    gl_t* o = out + 12 * q_raw;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        o[e] = CAP_ONLY ? mine[e] : gl_canon(lane_get(st.t0, e));
        o[4 + e] = CAP_ONLY ? mine[4 + e] : gl_canon(lane_get(st.t1, e));
        o[8 + e] = gl_canon(lane_get(st.t2, e));
    }
}

// Pair form: lane l < 32 of a wave holds words 0 .. 5 of state 32 w + l, lane l + 32 its words 6 .. 11.  CAP_ONLY specifies each lane's
// elements 2 .. 5: words 2 .. 5 and 8 .. 11.
template <bool CAP_ONLY>
__global__ __launch_bounds__(256, 2) void permute_pair_form_kernel(const gl_t* __restrict__ in, gl_t* __restrict__ out, size_t n) {
    __shared__ PairTables T;
    {
        const uint32_t* src = (const uint32_t*)&PAIR_TABLES;
        uint32_t* dst = (uint32_t*)&T;
        for (unsigned idx = threadIdx.x; idx < sizeof(PairTables) / 4; idx += blockDim.x) dst[idx] = src[idx];
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u, half = lane >> 5;
    const size_t q_raw = (blockIdx.x * (size_t)(blockDim.x >> 6) + (threadIdx.x >> 6)) * 32u + (lane & 31u);
    const bool live = q_raw < n;
    const gl_t* mine = in + 12 * (live ? q_raw : n - 1) + 6 * half;
    LaneZeros Z;
    lane_zeros_init(Z);
    PairMfma M;
    pair_mfma_init(M, lane);
    uint64_t mask_lo = 0xFFFFFFFFull;
    asm volatile("" : "+s"(mask_lo));
    PairState st;
#pragma unroll
    for (int e = 0; e < 2; e++) {
        pair_set(st.t0, e, mine[e]);
        pair_set(st.t1, e, mine[2 + e]);
        pair_set(st.t2, e, mine[4 + e]);
    }
    poseidon_permute_pair_asm<CAP_ONLY>(st, &T, Z, M, lane, mask_lo);
    if (!live) return;
    gl_t* o = out + 12 * q_raw + 6 * half;
#pragma unroll
    for (int e = 0; e < 2; e++) {
        o[e] = CAP_ONLY ? mine[e] : gl_canon(pair_get(st.t0, e));
        o[2 + e] = gl_canon(pair_get(st.t1, e));
        o[4 + e] = gl_canon(pair_get(st.t2, e));
    }
}

// Proof-of-work grinding (plonky2 fri_proof_of_work, App. A.8): the challenger's sponge state with its
// pending inputs already written in; candidate nonce goes to lane `pos`; the response is state[7]
// after one permutation.  Keeps the MINIMUM valid nonce in *best (initialised to UINT64_MAX).
__global__ void pow_grind_kernel(const gl_t* __restrict__ base_state, int pos, unsigned pow_bits, uint64_t start, uint64_t count,
                                 unsigned long long* best) { STARKHIP_PRIO_ENTRY
    uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= count) return;
    uint64_t w = start + t;
    gl_t s[12];
#pragma unroll
    for (int e = 0; e < 12; e++) s[e] = base_state[e];
    s[pos] = w;
    poseidon_permute_dev(s);
    if ((s[7] >> (64 - pow_bits)) == 0) atomicMin(best, (unsigned long long)w);
}

// The table of LeafPrefix (kernels.h): the sponge of leaf q = s n + k over the n columns e_0 .. e_{n-1}, whose LDE at that point is the
// LDE of e_0 rotated -- column c reads e0[s][(k - c) mod n] -- so no matrix is ever formed.  One lane per leaf, the generic permutation:
// it runs once per context and shape.
__global__ __launch_bounds__(64) void leaf_prefix_build_kernel(const gl_t* __restrict__ oh, unsigned log_n, unsigned rate_bits, gl_t* __restrict__ cap) { STARKHIP_PRIO_ENTRY
    const size_t n = (size_t)1 << log_n, N = n << rate_bits;
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q >= N) return;
    const size_t sidx = q >> log_n;
    const unsigned k = (unsigned)(q & (n - 1)), mask = (unsigned)(n - 1);
    const gl_t* e0 = oh + n + sidx * n;
    gl_t s[12];
#pragma unroll
    for (int e = 0; e < 12; e++) s[e] = 0;
#pragma unroll 1
    for (unsigned c = 0; c < (unsigned)n; c += 8) {
#pragma unroll
        for (unsigned e = 0; e < 8; e++) s[e] = e0[(k - c - e) & mask];
        poseidon_permute_dev(s);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) cap[(size_t)e * N + q] = gl_canon(s[8 + e]);
}

static inline unsigned nblocks(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

size_t leaf_prefix_words(unsigned log_n, unsigned rate_bits) { return lde_v2_oh_words(log_n, rate_bits) ? (size_t)4 << (log_n + rate_bits) : 0; }
hipError_t launch_leaf_prefix_build(const gl_t* oh, unsigned log_n, unsigned rate_bits, gl_t* cap, hipStream_t st) {
    if (!leaf_prefix_words(log_n, rate_bits) || !oh || !cap) return hipErrorInvalidValue;
    const size_t N = (size_t)1 << (log_n + rate_bits);
    hipLaunchKernelGGL(leaf_prefix_build_kernel, dim3(nblocks(N, 64)), dim3(64), 0, st, oh, log_n, rate_bits, cap);
    return hipGetLastError();
}

hipError_t upload_table_once(const void* symbol, const void* image, size_t bytes, bool (&done)[64]) {
    static std::mutex mu;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(mu);
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (done[dev]) return hipSuccess;
    if (!image) return hipErrorInvalidValue;
    e = hipMemcpyToSymbol(symbol, image, bytes);
    if (e == hipSuccess) done[dev] = true;
    return e;
}
static hipError_t ensure_quad_merged_tables() { return upload_table_once(&QUAD_MERGED, quad_merged_tables_host(), sizeof QUAD_MERGED, quad_uploaded); }
static hipError_t ensure_row_merged_tables() { return upload_table_once(&ROW_MERGED, row_merged_tables_host(), sizeof ROW_MERGED, row_uploaded); }
static hipError_t ensure_lane_tables() { return upload_table_once(&LANE_TABLES, lane_tables_host(), sizeof LANE_TABLES, lane_uploaded); }
static hipError_t ensure_pair_tables() { return upload_table_once(&PAIR_TABLES, pair_tables_host(), sizeof PAIR_TABLES, pair_uploaded); }

hipError_t launch_leaf_hash_form(LeafHashForm form, const gl_t* mat, size_t n_cols, unsigned log_n, unsigned rate_bits, gl_t* digests, hipStream_t st,
                                 LeafPrefix prefix) {
    const size_t N = (size_t)1 << (log_n + rate_bits);
    switch (form) {
        case FORM_QUAD:
            if (hipError_t e = ensure_quad_merged_tables(); e != hipSuccess) return e;
            hipLaunchKernelGGL(leaf_hash_kernel, dim3(nblocks(4 * N, 256)), dim3(256), 0, st, mat, n_cols, log_n, rate_bits, digests);
            break;
        case FORM_ROW:
            if (hipError_t e = ensure_row_merged_tables(); e != hipSuccess) return e;
            hipLaunchKernelGGL(leaf_hash_row_kernel, dim3(nblocks(16 * N, 256)), dim3(256), 0, st, mat, n_cols, log_n, rate_bits, digests);
            break;
        case FORM_LANE:
            if (hipError_t e = ensure_lane_tables(); e != hipSuccess) return e;
            {
                LeafHashBatch B = {};
                B.mat[0] = mat;
                B.digests[0] = digests;
                B.prefix_count[0] = prefix.count;
                B.prefix_cap[0] = prefix.cap;
                hipLaunchKernelGGL(leaf_hash_lane_kernel, dim3(nblocks(N, 256)), dim3(256), 0, st, B, n_cols, log_n, rate_bits);
            }
            break;
        case FORM_PAIR:
            if (hipError_t e = ensure_pair_tables(); e != hipSuccess) return e;
            hipLaunchKernelGGL(leaf_hash_pair_kernel, dim3(nblocks(N, 128)), dim3(256), 0, st, mat, n_cols, log_n, rate_bits, digests, prefix.count, prefix.cap);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
hipError_t launch_verify_leaf_digests(const gl_t* words, const VQLeaf* leaves, size_t n_leaves, gl_t* digests, unsigned hashers, hipStream_t st) {
    if (!n_leaves) return hipSuccess;
    if (hashers & (1u << STARKHIP_HASHER_POSEIDON)) {
        if (hipError_t e = ensure_row_merged_tables(); e != hipSuccess) return e;
        hipLaunchKernelGGL(verify_leaf_digest_kernel, dim3(nblocks(16 * n_leaves, 256)), dim3(256), 0, st, words, leaves, n_leaves, digests);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (hashers & (1u << STARKHIP_HASHER_KECCAK)) return launch_verify_leaf_digests_keccak(words, leaves, n_leaves, digests, st);
    return hipSuccess;
}
hipError_t launch_leaf_hash_multi(const LeafHashBatch& B, unsigned count, size_t n_cols, unsigned log_n, unsigned rate_bits, hipStream_t st) {
    if (count == 0 || count > LEAF_HASH_MAX_BATCH) return hipErrorInvalidValue;
    size_t N = (size_t)1 << (log_n + rate_bits);
    if (hipError_t e = ensure_quad_merged_tables(); e != hipSuccess) return e;
    if (count == 1) hipLaunchKernelGGL(leaf_hash_kernel, dim3(nblocks(4 * N, 256)), dim3(256), 0, st, B.mat[0], n_cols, log_n, rate_bits, B.digests[0]);
    else hipLaunchKernelGGL(leaf_hash_multi_kernel, dim3(nblocks(4 * N, 256), count), dim3(256), 0, st, B, n_cols, log_n, rate_bits);
    return hipGetLastError();
}
hipError_t launch_leaf_hash_lane_group(const LeafHashBatch& B, unsigned count, size_t n_cols, unsigned log_n, unsigned rate_bits, hipStream_t st) {
    if (count == 0 || count > LEAF_HASH_MAX_BATCH) return hipErrorInvalidValue;
    const size_t N = (size_t)1 << (log_n + rate_bits);
    if (hipError_t e = ensure_lane_tables(); e != hipSuccess) return e;
    hipLaunchKernelGGL(leaf_hash_lane_kernel, dim3(nblocks(N, 256), count), dim3(256), 0, st, B, n_cols, log_n, rate_bits);
    return hipGetLastError();
}
hipError_t launch_leaf_hash_rows(const gl_t* rows, size_t width, size_t n_leaves, gl_t* digests, hipStream_t st) {
    hipLaunchKernelGGL(leaf_hash_rows_kernel, dim3(nblocks(n_leaves, 64)), dim3(64), 0, st, rows, width, n_leaves, digests);
    return hipGetLastError();
}
// levels: digests buffer holds level 0 (n_leaves * 4) followed by level 1 (n_leaves/2 * 4) ... down to the cap level.
hipError_t launch_merkle_levels(gl_t* digests, unsigned log_leaves, unsigned cap_h, hipStream_t st) {
    gl_t* child = digests;
    for (unsigned lv = log_leaves; lv > cap_h; lv--) {
        size_t n_parent = (size_t)1 << (lv - 1);
        gl_t* parent = child + ((size_t)4 << lv);
        hipLaunchKernelGGL(merkle_level_kernel, dim3(nblocks(n_parent, 64)), dim3(64), 0, st, child, parent, n_parent);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        child = parent;
    }
    return hipSuccess;
}
hipError_t launch_permute_batch(gl_t* states, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(permute_batch_kernel, dim3(nblocks(n, 64)), dim3(64), 0, st, states, n);
    return hipGetLastError();
}
// form: a LeafHashForm, FORM_AUTO = the generic loop; variant 1 = the form's capacity-only last round (quad, lane, pair).  The caller has
// checked both (permute_form_variants) and n >= 1; `in` and `out` do not overlap.
hipError_t launch_permute_batch_form(int form, int variant, const gl_t* in, gl_t* out, size_t n, hipStream_t st) {
    if (variant < 0 || (unsigned)variant >= permute_form_variants(form) || n == 0) return hipErrorInvalidValue;
    switch (form) {
        case FORM_AUTO:
            if (hipError_t e = hipMemcpyAsync(out, in, n * 96, hipMemcpyDeviceToDevice, st); e != hipSuccess) return e;
            return launch_permute_batch(out, n, st);
        case FORM_QUAD: return launch_permute_quad_form(variant != 0, in, out, n, st);
        case FORM_ROW:
            if (hipError_t e = ensure_row_merged_tables(); e != hipSuccess) return e;
            hipLaunchKernelGGL(permute_row_form_kernel, dim3(nblocks(16 * n, 256)), dim3(256), 0, st, in, out, n);
            break;
        case FORM_LANE:
            if (hipError_t e = ensure_lane_tables(); e != hipSuccess) return e;
            if (variant) hipLaunchKernelGGL(permute_lane_form_kernel<true>, dim3(nblocks(n, 256)), dim3(256), 0, st, in, out, n);
            else hipLaunchKernelGGL(permute_lane_form_kernel<false>, dim3(nblocks(n, 256)), dim3(256), 0, st, in, out, n);
            break;
        default:  // FORM_PAIR
            if (hipError_t e = ensure_pair_tables(); e != hipSuccess) return e;
            if (variant) hipLaunchKernelGGL(permute_pair_form_kernel<true>, dim3(nblocks(n, 128)), dim3(256), 0, st, in, out, n);
            else hipLaunchKernelGGL(permute_pair_form_kernel<false>, dim3(nblocks(n, 128)), dim3(256), 0, st, in, out, n);
    }
    return hipGetLastError();
}
hipError_t launch_pow_grind(const gl_t* base_state, int pos, unsigned pow_bits, uint64_t start, uint64_t count, unsigned long long* best,
                            hipStream_t st) {
    hipLaunchKernelGGL(pow_grind_kernel, dim3(nblocks(count, 256)), dim3(256), 0, st, base_state, pos, pow_bits, start, count, best);
    return hipGetLastError();
}

}  // namespace starkhip
