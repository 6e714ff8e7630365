// Stand-alone program for the sanitizer run of the LogUp host code (make asan-logup-test): the validator over fuzzed sections (whatever
// it accepts is registered and its descriptors are built and walked), AirBuilder::logup against the parsed program, the host replay of
// the auxiliary polynomials on traces of 2 .. 1024 rows in both layouts with output buffers of exactly the size the header states (an
// over-write is the sanitizer's to find), a trace whose frequencies are off, a zero denominator, logup_eval_folded through
// starkhip_air_eval_frame_logup on frames of exactly nA openings, and the refusals.  Exit status 0 = consistent.
#include <stdio.h>

#include <vector>

#include "../include/starkhip.h"
#include "../starky_bls12_381_amd/csrc/air_ir.h"
#include "../starky_bls12_381_amd/csrc/air_validate.h"
#include "../starky_bls12_381_amd/csrc/logup.h"

using namespace starkhip;

static uint64_t rnd(uint64_t& s) {  // splitmix64
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// the test AIR: column 0 squared in column 1, column 2 the table, then per lookup m columns and a frequencies column
static AirProgram make_air(uint32_t degree, uint32_t m, uint32_t n_lookups) {
    AirBuilder b(3 + n_lookups * (m + 1), 0, degree);
    b.constraint(b.L(1) - b.L(0) * b.L(0));
    for (uint32_t l = 0; l < n_lookups; l++) {
        std::vector<uint32_t> cols;
        for (uint32_t c = 0; c < m; c++) cols.push_back(3 + l * (m + 1) + c);
        b.logup(cols, 2, 3 + l * (m + 1) + m);
    }
    return b.finish();
}

int main() {
    int bad = 0;
    uint64_t s = 1;
    // ---- the validator over fuzzed sections
    {
        AirBuilder b(7, 0, 3);
        b.constraint(b.L(1) - b.L(0) * b.L(0));
        b.logup({0, 3, 5}, 1, 2);
        b.logup({6}, 0, 4);
        b.logup({1, 4}, 6, 6);
        const std::vector<uint64_t> blob = b.finish().serialize();
        const size_t at = blob.size() - (2 + 5 + 3 + 4);
        bad += blob[at] != AIR_LOGUP_MAGIC;
        const uint64_t interesting[] = {0, 1, 2, 3, 6, 7, 63, 64, 65, 1ull << 32, 7ull << 32, (6ull << 32) | 6, (7ull << 32) | 6, ~0ull, AIR_LOGUP_MAGIC, AIR_PERM_MAGIC};
        size_t passed = 0;
        for (int trial = 0; trial < 4000; trial++) {
            std::vector<uint64_t> t = blob;
            if (trial % 5 == 4) t.resize(at + rnd(s) % (blob.size() - at + 2));  // a section cut short, or with a word too many
            for (int k = 0; k < 1 + trial % 2 && t.size() > at; k++)
                t[at + rnd(s) % (t.size() - at)] = trial % 3 ? interesting[rnd(s) % 16] : rnd(s) >> (rnd(s) % 64);
            std::vector<uint64_t> exact(t);  // exactly the blob's words on the heap
            AirProgram P;
            std::string why;
            if (!air_parse_checked(exact.data(), exact.size(), &P, &why)) {
                bad += why.empty();
                continue;
            }
            passed++;
            bad += !P.perm_pairs.empty() && !P.logups.empty();
            bad += P.logups.size() > STARKHIP_AIR_MAX_LOGUP_LOOKUPS || P.logup_polys() > STARKHIP_AIR_MAX_LOGUP_POLYS;
            for (const auto& lk : P.logups) {
                bad += lk.cols.empty() || lk.cols.size() > STARKHIP_AIR_MAX_LOGUP_COLUMNS || lk.table >= 7 || lk.freq >= 7;
                for (uint32_t c : lk.cols) bad += c >= 7;
            }
            bad += P.serialize() != exact;
            const std::vector<uint32_t> cols = logup_columns(P), d0 = logup_descriptor(P, false), d1 = logup_descriptor(P, true), zp = logup_z_polys(P);
            bad += d0.size() != d1.size() || zp.size() != 2 * P.logups.size();
            for (uint32_t z : zp) bad += z >= P.logup_polys();
            if (!P.logups.empty()) {
                uint32_t w = LOGUP_DESC_HEAD;
                for (size_t l = 0; l < P.logups.size(); l++) {
                    const uint32_t m = d1[w + 1];
                    for (uint32_t k = 2; k < LOGUP_DESC_LOOKUP + m; k++) bad += d1[w + k] >= cols.size() || cols[d1[w + k]] != d0[w + k];
                    w += LOGUP_DESC_LOOKUP + m;
                }
                bad += w != d1.size();
            }
        }
        bad += passed < 50;
    }
    // ---- the replay and the fold
    for (uint32_t degree : {2u, 3u, 5u})
        for (uint32_t m : {1u, degree - 1, degree, 16u}) {
            const uint32_t NL = 2;
            const AirProgram prog = make_air(degree, m, NL);
            const std::vector<uint64_t> blob = prog.serialize();
            starkhip_air_t air = (starkhip_air_t)0;
            if (starkhip_air_register(blob.data(), blob.size(), "AsanLogup", 0, &air) != STARKHIP_OK) return 3;
            const size_t C = prog.n_cols, nA = prog.logup_polys();
            bad += starkhip_air_logups(air) != (int)NL || starkhip_air_logup_polys(air) != (int)nA || nA != 2 * NL * ((m + degree - 2) / (degree - 1) + 1);
            for (size_t n : {(size_t)2, (size_t)4, (size_t)64, (size_t)1024}) {
                std::vector<uint64_t> rows(n * C, 0);
                for (size_t r = 0; r < n; r++) rows[r * C + 2] = 11 + 5 * r + (r % 3 == 0 ? GL_P : 0);  // the table; some cells written as value + p
                for (uint32_t l = 0; l < NL; l++)
                    for (size_t r = 0; r < n; r++)
                        for (uint32_t c = 0; c < m; c++) {
                            const size_t pick = rnd(s) % n;
                            rows[r * C + 3 + l * (m + 1) + c] = 11 + 5 * pick;
                            rows[pick * C + 3 + l * (m + 1) + m]++;
                        }
                std::vector<uint64_t> cols(n * C);
                for (size_t r = 0; r < n; r++)
                    for (size_t c = 0; c < C; c++) cols[c * n + r] = rows[r * C + c];
                const uint64_t ch[2] = {rnd(s) % GL_P, rnd(s) % GL_P};
                std::vector<uint64_t> polys(nA * n), polys2(nA * n), closing(2 * NL), closing2(2 * NL);  // exactly the sizes the header states
                uint64_t zeros = 7, zeros2 = 7;
                if (starkhip_logup_polys_replay(air, rows.data(), n, C, 0, ch, polys.data(), closing.data(), &zeros) != STARKHIP_OK) return 4;
                if (starkhip_logup_polys_replay(air, cols.data(), n, C, 1, ch, polys2.data(), closing2.data(), &zeros2) != STARKHIP_OK) return 5;
                bad += polys != polys2 || closing != closing2 || zeros != 0 || zeros2 != 0;
                for (uint64_t v : closing) bad += v != 0;
                for (uint64_t v : polys) bad += v >= GL_P;
                // every row satisfies the constraints: the fold over the frame (row, next row) with the row's masks is 0 + the AIR's own
                if (n <= 64) {
                    for (size_t r = 0; r < n; r++) {
                        std::vector<uint64_t> local(2 * C, 0), next(2 * C, 0), aux(2 * nA, 0), auxn(2 * nA, 0);  // exactly nA openings
                        for (size_t c = 0; c < C; c++) local[2 * c] = rows[r * C + c], next[2 * c] = rows[((r + 1) % n) * C + c];
                        for (size_t a = 0; a < nA; a++) aux[2 * a] = polys[a * n + r], auxn[2 * a] = polys[a * n + (r + 1) % n];
                        const uint64_t masks[8] = {1, 0, r + 1 < n, 0, r == 0, 0, r + 1 == n, 0};
                        const uint64_t alphas[4] = {rnd(s) % GL_P, rnd(s) % GL_P, rnd(s) % GL_P, rnd(s) % GL_P};
                        uint64_t acc[4], own[4];
                        if (starkhip_air_eval_frame_logup(air, local.data(), next.data(), nullptr, masks, alphas, 2, aux.data(), auxn.data(), ch, acc) != STARKHIP_OK) return 6;
                        if (starkhip_air_eval_frame(air, local.data(), next.data(), nullptr, masks, alphas, 2, own) != STARKHIP_OK) return 7;
                        for (int j = 0; j < 4; j++) bad += acc[j] != 0 || own[j] != 0;  // columns 0 and 1 are zero: the AIR's own constraint holds
                    }
                }
                // frequencies off by one in one row: the second lookup does not close, the first does
                std::vector<uint64_t> off = rows;
                off[(n / 2) * C + 3 + (m + 1) + m]++;
                if (starkhip_logup_polys_replay(air, off.data(), n, C, 0, ch, polys2.data(), closing2.data(), &zeros2) != STARKHIP_OK) return 8;
                bad += closing2[0] != 0 || closing2[NL] != 0 || closing2[1] == 0 || closing2[NL + 1] == 0 || zeros2 != 0;
                // a challenge that meets a cell: counted, and the inverse is 0
                const uint64_t meet[2] = {GL_P - rows[1 * C + 3] % GL_P, ch[1]};
                if (starkhip_logup_polys_replay(air, rows.data(), n, C, 0, meet, polys2.data(), closing2.data(), &zeros2) != STARKHIP_OK) return 9;
                bad += zeros2 < 1 || (degree == 2 && polys2[1] != 0);  // at degree 2 a helper is one inverse: row 1's first helper under chi_0
            }
            // refusals: none of them writes
            uint64_t t2[4] = {0}, out[1] = {5};
            const uint64_t ch[2] = {1, 2}, high[2] = {GL_P, 2};
            bad += starkhip_logup_polys_replay(air, t2, 3, C, 0, ch, out, out, out) != STARKHIP_ERR_BAD_SHAPE;
            bad += starkhip_logup_polys_replay(air, t2, 2, C + 1, 0, ch, out, out, out) != STARKHIP_ERR_BAD_SHAPE;
            bad += starkhip_logup_polys_replay(air, t2, 2, C, 0, high, out, out, out) != STARKHIP_ERR_BAD_SHAPE;
            bad += starkhip_logup_polys_replay(air, nullptr, 2, C, 0, ch, out, out, out) != STARKHIP_ERR_BAD_SHAPE;
            bad += starkhip_logup_polys_replay(air, t2, 2, C, 0, ch, out, out, nullptr) != STARKHIP_ERR_BAD_SHAPE;
            bad += starkhip_logup_polys_replay(STARKHIP_AIR_TEST_FIBONACCI, t2, 2, 2, 0, ch, out, out, out) != STARKHIP_ERR_BAD_AIR;
            bad += starkhip_logup_polys(nullptr, air, t2, 2, C, 0, 0, ch, out, out, out) != STARKHIP_ERR_NO_DEVICE;
            bad += out[0] != 5;
        }
    printf(bad ? "asan_logup: %d inconsistencies\n" : "asan_logup: ok\n", bad);
    return bad ? 1 : 0;
}
