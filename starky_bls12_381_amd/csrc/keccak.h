// Keccak-f[1600] and plonky2 0.1.4's KeccakHash<25> / KeccakGoldilocksConfig conventions (COMPAT.md K1 - K8) for host and gfx950 device
// code: keccak256 with the original 0x01 .. 0x80 padding, digests of 25 bytes carried as four field elements of 7, 7, 7 and 4 bytes,
// hash_or_noop with its threshold of 3 elements, two_to_one over 50 bytes, and the challenger's permutation with its word filter.
// The state is 25 uint64_t in registers: every index below is a compile-time constant once the loops are unrolled, the rotation amounts
// are template arguments, and the only table is the 24 round constants (immediates after the unrolling).
#pragma once
#include "../../include/starkhip.h"
#include "gl.h"

namespace starkhip {

#define KECCAK_RATE_WORDS 17  // 136 bytes
#define KECCAK_PAD_LAST 0x8000000000000000ULL  // 0x80 in byte 135 = the top byte of lane 16

#define STARKHIP_HASHER_COUNT 2  // STARKHIP_HASHER_POSEIDON, STARKHIP_HASHER_KECCAK (starkhip.h)

// On the device a 64-bit rotation by a constant is two funnel shifts of the 32-bit halves (v_alignbit_b32), after a swap of the halves
// for amounts of 32 and more; written on 64 bits the compiler makes it two 64-bit shifts and two ORs.
template <int N>
GL_HD uint64_t keccak_rotl(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (N == 0) return x;
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    const uint32_t a = N < 32 ? lo : hi, b = N < 32 ? hi : lo;  // the value rotated by 0 or 32 is b:a
    constexpr int M = N & 31;
    if (M == 0) return ((uint64_t)b << 32) | a;
    const uint32_t nlo = (a << M) | (b >> ((32 - M) & 31)), nhi = (b << M) | (a >> ((32 - M) & 31));
    return ((uint64_t)nhi << 32) | nlo;
#else
    return N == 0 ? x : (x << (N & 63)) | (x >> ((64 - N) & 63));
#endif
}

GL_HD void keccak_round(uint64_t* a, uint64_t rc) {
    uint64_t c[5], d[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ keccak_rotl<1>(c[(x + 1) % 5]);
    // rho and pi: b[y + 5 ((2 x + 3 y) mod 5)] = rotl(a[x + 5 y] ^ d[x], r[x][y])
    b[0] = a[0] ^ d[0];
    b[1] = keccak_rotl<44>(a[6] ^ d[1]);
    b[2] = keccak_rotl<43>(a[12] ^ d[2]);
    b[3] = keccak_rotl<21>(a[18] ^ d[3]);
    b[4] = keccak_rotl<14>(a[24] ^ d[4]);
    b[5] = keccak_rotl<28>(a[3] ^ d[3]);
    b[6] = keccak_rotl<20>(a[9] ^ d[4]);
    b[7] = keccak_rotl<3>(a[10] ^ d[0]);
    b[8] = keccak_rotl<45>(a[16] ^ d[1]);
    b[9] = keccak_rotl<61>(a[22] ^ d[2]);
    b[10] = keccak_rotl<1>(a[1] ^ d[1]);
    b[11] = keccak_rotl<6>(a[7] ^ d[2]);
    b[12] = keccak_rotl<25>(a[13] ^ d[3]);
    b[13] = keccak_rotl<8>(a[19] ^ d[4]);
    b[14] = keccak_rotl<18>(a[20] ^ d[0]);
    b[15] = keccak_rotl<27>(a[4] ^ d[4]);
    b[16] = keccak_rotl<36>(a[5] ^ d[0]);
    b[17] = keccak_rotl<10>(a[11] ^ d[1]);
    b[18] = keccak_rotl<15>(a[17] ^ d[2]);
    b[19] = keccak_rotl<56>(a[23] ^ d[3]);
    b[20] = keccak_rotl<62>(a[2] ^ d[2]);
    b[21] = keccak_rotl<55>(a[8] ^ d[3]);
    b[22] = keccak_rotl<39>(a[14] ^ d[4]);
    b[23] = keccak_rotl<41>(a[15] ^ d[0]);
    b[24] = keccak_rotl<2>(a[21] ^ d[1]);
    // chi (and-not), then iota
#pragma unroll
    for (int y = 0; y < 25; y += 5) {
#pragma unroll
        for (int x = 0; x < 5; x++) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
    }
    a[0] ^= rc;
}

GL_HD void keccak_f1600(uint64_t* a) {
    keccak_round(a, 0x0000000000000001ULL); keccak_round(a, 0x0000000000008082ULL); keccak_round(a, 0x800000000000808AULL);
    keccak_round(a, 0x8000000080008000ULL); keccak_round(a, 0x000000000000808BULL); keccak_round(a, 0x0000000080000001ULL);
    keccak_round(a, 0x8000000080008081ULL); keccak_round(a, 0x8000000000008009ULL); keccak_round(a, 0x000000000000008AULL);
    keccak_round(a, 0x0000000000000088ULL); keccak_round(a, 0x0000000080008009ULL); keccak_round(a, 0x000000008000000AULL);
    keccak_round(a, 0x000000008000808BULL); keccak_round(a, 0x800000000000008BULL); keccak_round(a, 0x8000000000008089ULL);
    keccak_round(a, 0x8000000000008003ULL); keccak_round(a, 0x8000000000008002ULL); keccak_round(a, 0x8000000000000080ULL);
    keccak_round(a, 0x000000000000800AULL); keccak_round(a, 0x800000008000000AULL); keccak_round(a, 0x8000000080008081ULL);
    keccak_round(a, 0x8000000000008080ULL); keccak_round(a, 0x0000000080000001ULL); keccak_round(a, 0x8000000080008008ULL);
}

// K6: the first 25 bytes of a hash output (lanes o[0 .. 3], little-endian) as four field elements of 7, 7, 7 and 4 bytes
GL_HD void keccak_digest_words(uint64_t o0, uint64_t o1, uint64_t o2, uint64_t o3, gl_t* w) {
    w[0] = o0 & 0x00FFFFFFFFFFFFFFULL;
    w[1] = (o0 >> 56) | ((o1 & 0x0000FFFFFFFFFFFFULL) << 8);
    w[2] = (o1 >> 48) | ((o2 & 0x000000FFFFFFFFFFULL) << 16);
    w[3] = (o2 >> 40) | ((o3 & 0xFFULL) << 24);
}
// ... and back: the 25 bytes as lanes l[0 .. 2] and the one byte l[3]
GL_HD void keccak_digest_lanes(const gl_t* w, uint64_t* l) {
    l[0] = w[0] | (w[1] << 56);
    l[1] = (w[1] >> 8) | (w[2] << 48);
    l[2] = (w[2] >> 16) | (w[3] << 40);
    l[3] = w[3] >> 24;
}
// the ranges K6 leaves a digest's words in; a proof word outside them is no digest
GL_HD bool keccak_digest_in_range(const gl_t* w) { return ((w[0] | w[1] | w[2]) >> 56) == 0 && (w[3] >> 32) == 0; }

// K5: keccak256 over l ++ r (50 bytes), truncated
GL_HD void keccak_two_to_one(const gl_t* l, const gl_t* r, gl_t* out) {
    uint64_t L[4], R[4], a[25];
    keccak_digest_lanes(l, L);
    keccak_digest_lanes(r, R);
    a[0] = L[0]; a[1] = L[1]; a[2] = L[2];
    a[3] = L[3] | (R[0] << 8);
    a[4] = (R[0] >> 56) | (R[1] << 8);
    a[5] = (R[1] >> 56) | (R[2] << 8);
    a[6] = (R[2] >> 56) | (R[3] << 8) | (0x01ULL << 16);  // bytes 48, 49 and the first padding byte
#pragma unroll
    for (int i = 7; i < 25; i++) a[i] = 0;
    a[16] = KECCAK_PAD_LAST;
    keccak_f1600(a);
    keccak_digest_words(a[0], a[1], a[2], a[3], out);
}

// K3 / K4 over a strided sequence (element i at in[i * stride]), canonical elements as 8 little-endian bytes each: leaves of at most
// 3 elements are copied (zero padded to 25 bytes), longer ones hashed.  One call site of the permutation: the last block is the
// partial one (possibly empty: the extra padding block of a length that is a multiple of 17).
GL_HD void keccak_hash_or_noop(const gl_t* in, size_t len, size_t stride, gl_t* out) {
    if (len <= 3) {
        keccak_digest_words(len > 0 ? in[0] : 0, len > 1 ? in[stride] : 0, len > 2 ? in[2 * stride] : 0, 0, out);
        return;
    }
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
    const size_t n_blocks = len / KECCAK_RATE_WORDS + 1;
    for (size_t b = 0; b < n_blocks; b++) {
        const size_t off = b * KECCAK_RATE_WORDS, rem = len - off < KECCAK_RATE_WORDS ? len - off : KECCAK_RATE_WORDS;
#pragma unroll
        for (int e = 0; e < KECCAK_RATE_WORDS; e++) {
            if ((size_t)e < rem) a[e] ^= in[(off + e) * stride];
        }
        if (b + 1 == n_blocks) {  // rem < 17 here
#pragma unroll
            for (int e = 0; e < KECCAK_RATE_WORDS; e++) {
                if ((size_t)e == rem) a[e] ^= 0x01ULL;
            }
            a[16] ^= KECCAK_PAD_LAST;
        }
        keccak_f1600(a);
    }
    keccak_digest_words(a[0], a[1], a[2], a[3], out);
}

// K7's word filter: the words below p of words[0 .. n) go to state[have], state[have + 1], ... until the state has 12; returns the new
// count and adds the words it read to *used.  The state is written with constant indices (a device caller keeps it in registers).
GL_HD int keccak_take_words(const uint64_t* words, int n, gl_t* state, int have, int* used) {
    for (int k = 0; k < n && have < 12; k++) {
        const uint64_t w = words[k];
        (*used)++;
        if (w >= GL_P) continue;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            if (i == have) state[i] = w;
        }
        have++;
    }
    return have;
}

// K7: the challenger's permutation.  keccak256 of the state's 96 bytes, then of each 32-byte output in turn; the outputs' words below p
// are the new state.
GL_HD void keccak_permute(gl_t* s) {
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 12; i++) a[i] = s[i];
    a[12] = 0x01ULL;
#pragma unroll
    for (int i = 13; i < 25; i++) a[i] = 0;
    a[16] = KECCAK_PAD_LAST;
    int have = 0, used = 0;
    for (;;) {
        keccak_f1600(a);
        uint64_t h[4] = {a[0], a[1], a[2], a[3]};
        have = keccak_take_words(h, 4, s, have, &used);
        if (have >= 12) break;
        a[4] = 0x01ULL;
#pragma unroll
        for (int i = 5; i < 25; i++) a[i] = 0;
        a[16] = KECCAK_PAD_LAST;
    }
}

// host code (keccak_host.cpp)
void keccak256_host(const uint8_t* bytes, size_t len, uint8_t out[32]);
void keccak_permute_host(gl_t* s);

}  // namespace starkhip
