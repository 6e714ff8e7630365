// The leaf-hash forms' tables (poseidon_tables.h), built on the host from poseidon_merged.h's matrices and constants: what the kernels of
// kernels_hash.hip find in constant memory, and what starkhip_hash_table_image shows a CPU test byte for byte.
#include "poseidon_tables.h"

#include <string.h>

#include <mutex>

#include "poseidon_merged.h"

namespace starkhip {

static RcPair split(gl_t v) { return RcPair{v & 0xFFFFFFFFull, v >> 32}; }

// Lane l owns state elements l, l + 4, l + 8 (slots 0, 1, 2); its rotated operand (r, m) is element ((l + r) & 3) + 4 m.
static inline int quad_elem(int l, int m) { return l + 4 * m; }
static inline int quad_col(int l, int r, int m) { return ((l + r) & 3) + 4 * m; }

// The per-lane views of poseidon_merged.h's tables and of the circulant MDS matrix.
static bool build_quad_merged_tables(QuadMergedTables& T) {
    static PoseidonMergedTables P;
    build_poseidon_merged_tables(P);
    for (int l = 0; l < 4; l++) {
        uint32_t* c = T.coef[l];
        for (int r = 0; r < 4; r++)
            for (int m = 0; m < 3; m++) {
                const int col = quad_col(l, r, m);
                for (int mo = 0; mo < 3; mo++) c[12 * mo + 3 * r + m] = (uint32_t)P.N3[quad_elem(l, mo)][col];
            }
        for (int m = 0; m < 3; m++) {
            c[36 + m] = (uint32_t)P.M[0][quad_elem(l, m)];   // the lane's own columns of row 0
            c[39 + m] = (uint32_t)P.N2[0][quad_elem(l, m)];
        }
        c[42] = l == 0 ? (uint32_t)P.M[0][0] : 0;
        for (int mo = 0; mo < 3; mo++) {
            c[43 + mo] = (uint32_t)P.N2[quad_elem(l, mo)][0];
            c[46 + mo] = (uint32_t)P.M[quad_elem(l, mo)][0];
        }
        c[49] = 0;
        // cf[3 r + d]: coefficient of the operand (r, m') for the output slot m with (m' - m) mod 3 = d:
        // CIRC[(col - out) mod 12] with col - out = ((l + r) & 3) - l + 4 d
        for (int r = 0; r < 4; r++)
            for (int d = 0; d < 3; d++) c[50 + 3 * r + d] = POSEIDON_MDS_CIRC[((((l + r) & 3) - l + 4 * d) % 12 + 12) % 12];
        c[62] = c[63] = 0;
    }
    // every lane seeds its partial sum of y1 / y2 with a quarter of the constant (4^-1 = (3p + 1) / 4 mod p)
    const gl_t quarter = (gl_t)((((unsigned __int128)3 * GL_P) + 1) / 4);
    for (int t = 0; t < QUAD_MERGED_TRIPLES; t++) {
        T.tk[2 * t] = split(gl_mul(P.k1[t], quarter));
        T.tk[2 * t + 1] = split(gl_mul(P.k2[t], quarter));
        for (int l = 0; l < 4; l++)
            for (int mo = 0; mo < 3; mo++) T.tk3[l][3 * t + mo] = split(P.k3[t][quad_elem(l, mo)]);
    }
    return true;
}

// ---- the row form's merged triples: per-lane coefficient rows and constants
static bool build_row_merged_tables(RowMergedTables& T) {
    static PoseidonMergedTables P;
    build_poseidon_merged_tables(P);
    for (int e = 0; e < 16; e++) {
        uint32_t* c = T.coef[e];
        for (int k = 0; k < 20; k++) c[k] = 0;
        if (e >= 12) continue;
        for (int k = 0; k < 12; k++) c[k] = (uint32_t)P.N3[e][(e + k) % 12];
        c[12] = (uint32_t)P.M[0][e];
        c[13] = (uint32_t)P.N2[0][e];
        c[14] = (uint32_t)P.N2[e][0];
        c[15] = (uint32_t)P.M[e][0];
        c[16] = (uint32_t)P.N3[e][0];
        c[17] = e == 0 ? (uint32_t)P.M[0][0] : 0;
        c[18] = e == 0 ? (uint32_t)P.N2[0][0] : 0;
    }
    for (int t = 0; t < POSEIDON_MERGED_TRIPLES; t++) {
        T.k1[t] = split(P.k1[t]);
        T.k2[t] = split(P.k2[t]);
        for (int e = 0; e < 12; e++) T.k3[t][e] = split(P.k3[t][e]);
    }
    return true;
}

// The matrix-pipe rounds of the lane and pair forms (poseidon_dev.h: poseidon_permute_lane_asm, poseidon_permute_pair_asm): the layer of
// such a round is seeded with the constants of round `next` (none beyond round 29).  The products see signed bytes (byte - 128) and the
// spare K-values add LANE_K_OFFSET to every plane, so the 64-bit constant whose bytes ride in the weight tile of output g is
// RC[g] = rc[g] - (34 818 - 128 rowsum[g]) * 0x0101010101010101  mod p  (a row sums twelve signed bytes in both forms).  Writes the
// weight-tile dwords of its byte planes first, first + step, .. (count of them) to dst[0], dst[64], ..: one lane's column of rcb.
static void pack_rcb(uint32_t* dst, int next, unsigned g, unsigned first, unsigned step, unsigned count) {
    uint64_t rowsum = 0;
    for (int j = 0; j < 12; j++) rowsum += (uint64_t)POSEIDON_MDS_CIRC[(j + 12 - (int)g) % 12] + ((g == 0 && j == 0) ? 8u : 0u);
    const gl_t off = gl_mul((gl_t)(LANE_K_OFFSET - 128 * rowsum), 0x0101010101010101ull % GL_P);
    const gl_t RC = gl_sub(next < 30 ? POSEIDON_RC_HOST[12 * next + g] : 0, off);
    for (unsigned k = 0; k < count; k++) {
        const uint32_t byte = (uint32_t)(RC >> (8 * (first + step * k))) & 0xFFu;
        dst[64 * k] = (byte & 0x7Fu) | ((2u * (byte >> 7) + 40u) << 8) | (127u << 16) | (127u << 24);
    }
}

static bool build_lane_tables(LaneTables& T) {
    static PoseidonMergedFours P;
    build_poseidon_merged_fours(P);
    if (!P.sums_fit) return false;   // (a property of the MDS matrix, checked where the tables are made: the accumulators' 64 bits)
    memset(&T, 0, sizeof T);
    for (int r = 0; r < 30; r++)
        for (int e = 0; e < 12; e++) T.rc[r][e] = split(POSEIDON_RC_HOST[12 * r + e]);
    for (int e = 0; e < 12; e++) T.rc0[e] = POSEIDON_RC_HOST[e];
    for (int t = 0; t < POSEIDON_MERGED_FOURS; t++) {
        T.kf[t][0] = split(P.k1[t]);
        T.kf[t][1] = split(P.k2[t]);
        T.kf[t][2] = split(P.k3[t]);
        for (int e = 0; e < 12; e++) T.k4[t][e] = split(P.k4[t][e]);
    }
    for (int r = 0; r < 12; r++) {
        for (int c = 0; c < 12; c++) T.row[r][c] = (uint32_t)P.N4[r][c];
        T.row[r][12] = (uint32_t)P.N3[r][0];
        T.row[r][13] = (uint32_t)P.N2[r][0];
        T.row[r][14] = (uint32_t)P.M[r][0];
        T.m0[r] = (uint32_t)P.M[0][r];
        T.n20[r] = (uint32_t)P.N2[0][r];
        T.n30[r] = (uint32_t)P.N3[0][r];
    }
    T.n30[12] = (uint32_t)P.N2[0][0];
    // table m serves the round whose layer is seeded with rc[NEXT_ROUND[m]]; the tile row of a lane holds output g, all eight byte planes
    static const int NEXT_ROUND[9] = {1, 2, 3, 4, 25, 26, 27, 28, 29};
    for (int m = 0; m < 9; m++)
        for (unsigned lane = 0; lane < 64; lane++) {
            const unsigned row = lane & 31u, half = lane >> 5, g = (row & 3u) + 4u * (row >> 3);
            if (((row >> 2) & 1u) == half && g < 12u) pack_rcb(&T.rcb[m][0][lane], NEXT_ROUND[m], g, 0, 1, 8);
        }
    return true;
}

static bool build_pair_tables(PairTables& T) {
    static PoseidonMergedFours P;
    build_poseidon_merged_fours(P);
    if (!P.sums_fit) return false;
    memset(&T, 0, sizeof T);
    for (unsigned h = 0; h < 2; h++) {
        for (unsigned e = 0; e < 6; e++) T.rc0[h][e] = POSEIDON_RC_HOST[6 * h + e];
        for (int t = 0; t < POSEIDON_MERGED_FOURS; t++)
            for (unsigned r = 0; r < 6; r++) T.k4[t][h][r] = split(P.k4[t][6 * h + r]);
        uint32_t* c = T.coef[h];
        for (unsigned e = 0; e < 6; e++) {
            c[e] = (uint32_t)P.M[0][6 * h + e];
            c[8 + e] = (uint32_t)P.N2[0][6 * h + e];
            c[16 + e] = (uint32_t)P.N3[0][6 * h + e];
        }
        c[16 + 6] = (uint32_t)P.N2[0][0];
        for (unsigned r = 0; r < 6; r++) {
            const unsigned g = 6 * h + r;
            uint32_t* row = c + 24 + 16 * r;
            for (unsigned jj = 0; jj < 12; jj++) row[jj] = (uint32_t)P.N4[g][(6 * h + jj) % 12];   // own six, then the partner's
            row[12] = (uint32_t)P.N3[g][0];
            row[13] = (uint32_t)P.N2[g][0];
            row[14] = (uint32_t)P.M[g][0];
        }
    }
    for (int t = 0; t < POSEIDON_MERGED_FOURS; t++) {   // the constants of the three dot products enter once: through the lower half
        T.kf[t][0][0] = split(P.k1[t]);
        T.kf[t][0][1] = split(P.k2[t]);
        T.kf[t][0][2] = split(P.k3[t]);
    }
    // the tile row of a lane of the lower K-half holds output g against byte planes pp, pp + 2, pp + 4, pp + 6: one per instruction
    static const int NEXT_ROUND[PAIR_MFMA_ROUNDS] = {1, 2, 3, 4, 25, 26, 27, 28, 29, 30};
    for (int m = 0; m < PAIR_MFMA_ROUNDS; m++)
        for (unsigned lane = 0; lane < 32; lane++) {
            const unsigned i = (lane & 3u) + 4u * (lane >> 3), out_half = (lane >> 2) & 1u;
            if (i < 12u) pack_rcb(&T.rcb[m][0][lane], NEXT_ROUND[m], 6u * out_half + i % 6u, i / 6u, 2, 4);
        }
    return true;
}

// ---- the images, built once each
// false from a builder: the four-round merge's sums would not fit (poseidon_merged.h: sums_fit); the image is null then
template <class T>
static const T* built_once(bool (*build)(T&)) {
    static T image;  // zero-initialised; one per table type
    static std::once_flag once;
    static bool ok = false;
    std::call_once(once, [&] { ok = build(image); });
    return ok ? &image : nullptr;
}
const QuadMergedTables* quad_merged_tables_host() { return built_once<QuadMergedTables>(build_quad_merged_tables); }
const RowMergedTables* row_merged_tables_host() { return built_once<RowMergedTables>(build_row_merged_tables); }
const LaneTables* lane_tables_host() { return built_once<LaneTables>(build_lane_tables); }
const PairTables* pair_tables_host() { return built_once<PairTables>(build_pair_tables); }

// Host replay of the quad formulation with exactly the tables the kernel gets (per-lane coefficient views included), against
// the plain host permutation: a CPU-side check of build_quad_merged_tables (tests/test_field_hash_cpu.py).  Returns the
// number of mismatching states out of `n`.
int quad_merged_tables_selfcheck(unsigned n) {
    const QuadMergedTables& T = *quad_merged_tables_host();
    auto join = [](const RcPair& c) { return (gl_t)(c.lo | (c.hi << 32)); };
    // the plain layer as the kernel computes it: per lane, twelve coefficients by rotation and slot difference
    auto mds_lanes = [&](gl_t* s) {
        gl_t out[12];
        for (int l = 0; l < 4; l++)
            for (int mo = 0; mo < 3; mo++) {
                gl_t acc = 0;
                for (int r = 0; r < 4; r++)
                    for (int m = 0; m < 3; m++) acc = gl_add(acc, gl_mul(s[quad_col(l, r, m)], T.coef[l][50 + 3 * r + (m - mo + 3) % 3]));
                if (l == 0 && mo == 0) acc = gl_add(acc, gl_mul(s[0], 8));
                out[quad_elem(l, mo)] = acc;
            }
        for (int i = 0; i < 12; i++) s[i] = out[i];
    };
    int bad = 0;
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (unsigned it = 0; it < n; it++) {
        gl_t s[12], want[12];
        for (int i = 0; i < 12; i++) {
            seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
            s[i] = it == 0 ? 0 : it == 1 ? GL_P - 1 : seed % GL_P;
            want[i] = s[i];
        }
        poseidon_permute(want);
        const uint64_t* RC = POSEIDON_RC_HOST;
        int r = 0;
        for (; r < 4; r++) {
            for (int i = 0; i < 12; i++) s[i] = poseidon_sbox(gl_add(s[i], RC[12 * r + i]));
            mds_lanes(s);
        }
        for (int i = 0; i < 12; i++) s[i] = gl_add(s[i], RC[12 * r + i]);
        for (int t = 0; t < QUAD_MERGED_TRIPLES; t++, r += 3) {
            gl_t u[12];
            for (int i = 0; i < 12; i++) u[i] = s[i];
            u[0] = poseidon_sbox(u[0]);
            // y1, y2: per-lane partial sums with the quartered constants, exactly as the kernel adds them up
            gl_t y1 = 0, y2p = 0;
            for (int l = 0; l < 4; l++) {
                const uint32_t* c = T.coef[l];
                gl_t a = join(T.tk[2 * t]), b = join(T.tk[2 * t + 1]);
                for (int m = 0; m < 3; m++) {
                    a = gl_add(a, gl_mul(u[quad_elem(l, m)], c[36 + m]));
                    b = gl_add(b, gl_mul(u[quad_elem(l, m)], c[39 + m]));
                }
                y1 = gl_add(y1, a);
                y2p = gl_add(y2p, b);
            }
            const gl_t x2 = poseidon_sbox(y1);
            gl_t y2 = y2p;
            for (int l = 0; l < 4; l++) y2 = gl_add(y2, gl_mul(x2, T.coef[l][42]));
            const gl_t x3 = poseidon_sbox(y2);
            for (int l = 0; l < 4; l++) {
                const uint32_t* c = T.coef[l];
                for (int mo = 0; mo < 3; mo++) {
                    gl_t acc = join(T.tk3[l][3 * t + mo]);
                    for (int rr = 0; rr < 4; rr++)
                        for (int m = 0; m < 3; m++) acc = gl_add(acc, gl_mul(u[quad_col(l, rr, m)], c[12 * mo + 3 * rr + m]));
                    acc = gl_add(acc, gl_mul(x2, c[43 + mo]));
                    acc = gl_add(acc, gl_mul(x3, c[46 + mo]));
                    s[quad_elem(l, mo)] = acc;
                }
            }
        }
        s[0] = poseidon_sbox(s[0]);  // round 25, plain
        mds_lanes(s);
        r++;
        for (int i = 0; i < 12; i++) s[i] = gl_add(s[i], RC[12 * r + i]);
        for (; r < 30; r++) {
            for (int i = 0; i < 12; i++) s[i] = poseidon_sbox(s[i]);
            mds_lanes(s);
            if (r + 1 < 30)
                for (int i = 0; i < 12; i++) s[i] = gl_add(s[i], RC[12 * (r + 1) + i]);
        }
        for (int i = 0; i < 12; i++)
            if (s[i] != want[i]) {
                bad++;
                break;
            }
    }
    return bad;
}

}  // namespace starkhip
