// The host-built tables of the leaf-hash forms (poseidon_dev.h): plain data that poseidon_tables.cpp fills on the CPU and the kernels of
// kernels_hash.hip read from constant memory.  No HIP header here: the builders are host code of the host-only builds too (Makefile: asan,
// tsan-test), and starkhip_hash_table_image hands the images to a CPU test (tests/golden/hash_table_images.json).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gl.h"

namespace starkhip {

// Round constants as the kernels stage them in LDS: per constant two 64-bit words (low half, high half), so each
// is directly the 64-bit addend of the first multiply-add of its accumulator.
struct RcPair {
    uint64_t lo, hi;
};

static const int QUAD_MERGED_TRIPLES = 7;  // = POSEIDON_MERGED_TRIPLES (poseidon_merged.h): partial rounds 0..20; the 22nd stays a plain round

// The host-built image of the per-lane tables (poseidon_tables.cpp: build_quad_merged_tables), uploaded to constant memory once per device
struct QuadMergedTables {
    uint32_t coef[4][64];  // per lane: n3[3][12], n1[3], n2[3], m00 (lane 0 only), b2[3], b3[3], pad to 50, cf[12] at 50, pad
    RcPair tk[2 * QUAD_MERGED_TRIPLES];       // k1, k2 per triple
    RcPair tk3[4][3 * QUAD_MERGED_TRIPLES];   // per lane: k3[mo] per triple
};

// Per-lane coefficient rows of the merged triples, built on the host once per device (poseidon_tables.cpp)
struct RowMergedTables {
    uint32_t coef[16][20];                       // [lane]: n3k[12], then misc0[4], misc1[4]
    RcPair k1[7], k2[7], k3[7][12];              // POSEIDON_MERGED_TRIPLES = 7
};

struct LaneTables {
    RcPair rc[31][12];         // round constants in halves; rc[30] = 0 (the "next round" of the last one)
    RcPair kf[5][3];           // k1, k2, k3 of the merged fours (poseidon_merged.h)
    RcPair k4[5][12];
    uint32_t row[12][16];      // per output row of the dense layer: N4[r][0 .. 11], N3[r][0], N2[r][0], M[r][0], -
    uint32_t m0[12], n20[12];  // row 0 of M and of N2 (the first two intermediate dot products) ...
    uint32_t n30[16];          // ... and of N3, then N2[0][0] (the third)
    // The rounds whose circulant layer runs on the matrix pipe (full rounds 0 .. 3 and 26 .. 28, the plain partial rounds 24 and 25;
    // lane_round_asm.inc, tools/gen_lane_round_asm.py): per round, byte plane and LANE the fourth dword of the weight tile -- the constant
    // bytes that ride in the spare K-values (poseidon_tables.cpp: build_lane_tables)
    uint32_t rcb[9][8][64];
    gl_t rc0[12];              // the first round's constants as whole words (added to the state at the start of every permutation)
};

constexpr int PAIR_MFMA_ROUNDS = 10;   // full rounds 0 .. 3, the plain partial rounds 24 and 25, full rounds 26 .. 29
struct PairTables {
    gl_t rc0[2][6];                 // [half]: the first round's constants of the half's elements
    RcPair kf[5][2][3];             // [merged four][half]: k1, k2, k3 -- in the lower half only (the sums are added across the pair), zero in the upper
    RcPair k4[5][2][6];             // [merged four][half][local output]
    // per half, 480 bytes: rows 0 of M, N2 and N3 against the half's own six elements (8 dwords each; N2[0][0] in dword 6 of the third),
    // then per local output r (g = 6 half + r) sixteen dwords: N4[g][own six], N4[g][the partner's six, neighbours crossed], N3[g][0],
    // N2[g][0], M[g][0], 0
    uint32_t coef[2][120];
    uint32_t rcb[PAIR_MFMA_ROUNDS][4][64];   // per matrix-pipe round, instruction and LANE: dword 3 of the weight tile (the constants' bytes)
};

// What the spare K-values of the matrix-pipe rounds add to every byte plane (tools/gen_lane_round_asm.py: K_OFFSET; poseidon_dev.h
// asserts that lane_round_asm.inc's STARKHIP_LANE_K_OFFSET is this)
constexpr uint32_t LANE_K_OFFSET = 34818;

// The kernels copy the images to LDS dword by dword, and the scheduled blocks address them by byte offset
static_assert(sizeof(QuadMergedTables) == 2592 && sizeof(RowMergedTables) == 2848, "leaf-hash table layout");
static_assert(sizeof(LaneTables) == 26608 && sizeof(PairTables) == 12736, "leaf-hash table layout");
// tools/gen_lane_round_asm.py: ROW_OFF, M0_OFF, N20_OFF, N30_OFF, relative to LaneTables::row
static_assert(offsetof(LaneTables, m0) - offsetof(LaneTables, row) == 12 * 64, "M0_OFF");
static_assert(offsetof(LaneTables, n20) - offsetof(LaneTables, row) == 12 * 64 + 48, "N20_OFF");
static_assert(offsetof(LaneTables, n30) - offsetof(LaneTables, row) == 12 * 64 + 96, "N30_OFF");

// ---- poseidon_tables.cpp: each image is built once; null when the four-round merge's sums would not fit (poseidon_merged.h: sums_fit)
const QuadMergedTables* quad_merged_tables_host();
const RowMergedTables* row_merged_tables_host();
const LaneTables* lane_tables_host();
const PairTables* pair_tables_host();
// CPU replay of the quad form's merged-partial-round tables against the plain permutation; mismatching states out of n
int quad_merged_tables_selfcheck(unsigned n);
int merged_fours_selfcheck(unsigned n);   // poseidon_host.cpp: the same for the four-round merges of the lane and pair forms

}  // namespace starkhip
