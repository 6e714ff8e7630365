// Stand-alone program for the sanitizer run of starkhip_check_trace_permutations' host driver and replay (make asan-perm-check-test):
// an AIR with a three-entry and two one-entry pairs on traces of 2 .. 1024 rows, both layouts, satisfying and with changed cells, with
// per_pair, masks and list buffers of exactly the size the header states (an over-write is the sanitizer's to find), every cap from 0
// to past the number of flagged rows, and the refusals.  Exit status 0 = consistent.
#include <stdio.h>

#include <vector>

#include "../include/starkhip.h"
#include "../starky_bls12_381_amd/csrc/air_ir.h"

using namespace starkhip;

static uint64_t rnd(uint64_t& s) {  // splitmix64
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

int main() {
    int bad = 0;
    AirBuilder b(6, 0, 3);
    b.constraint(b.L(0) - b.L(0));
    b.permutation_pair({{0, 3}, {1, 4}, {2, 5}});
    b.permutation_pair({{0, 3}});
    b.permutation_pair({{1, 4}});
    const std::vector<uint64_t> blob = b.finish().serialize();
    starkhip_air_t air = (starkhip_air_t)0;
    if (starkhip_air_register(blob.data(), blob.size(), "AsanPermCheck", 0, &air) != STARKHIP_OK) return 2;
    const size_t C = 6, NP = 3;
    uint64_t s = 1;
    for (size_t n : {(size_t)2, (size_t)4, (size_t)64, (size_t)1024}) {
        const size_t W = (n + 63) / 64;
        std::vector<uint64_t> rows(n * C);
        for (size_t r = 0; r < n; r++)
            for (size_t c = 0; c < 3; c++) rows[r * C + c] = rnd(s) % 97;  // few values: long runs of equal keys
        for (size_t r = 0; r < n; r++)  // the rhs: the lhs rows rotated, some cells written as value + p
            for (size_t c = 0; c < 3; c++) rows[r * C + 3 + c] = rows[((r + n / 2 + 1) % n) * C + c] + (r % 3 == 0 ? 0xFFFFFFFF00000001ULL : 0);
        for (int broken = 0; broken < 2; broken++) {
            if (broken) rows[(n - 1) * C + 4] += 1000, rows[3] += 1000;
            std::vector<uint64_t> cols(n * C);
            for (size_t r = 0; r < n; r++)
                for (size_t c = 0; c < C; c++) cols[c * n + r] = rows[r * C + c];
            starkhip_perm_check_t full = {}, rep = {};
            std::vector<uint32_t> per(NP), per2(NP);
            std::vector<uint64_t> masks(NP * 2 * W), masks2(NP * 2 * W);
            if (starkhip_check_trace_permutations_replay(air, rows.data(), n, C, 0, 12345, per.data(), masks.data(), nullptr, 0, &full) != STARKHIP_OK) return 3;
            bad += full.pairs != NP || full.pairs_undecided != 0 || (full.unmatched != 0) != (broken != 0) || full.unmatched % 2;
            uint64_t bits = 0;
            for (uint64_t w : masks) bits += (uint64_t)__builtin_popcountll(w);
            bad += bits != full.unmatched;
            for (size_t cap = 0; cap <= full.unmatched + 2; cap++) {
                std::vector<uint64_t> list(3 * cap);  // exactly cap entries
                if (starkhip_check_trace_permutations_replay(air, cols.data(), n, C, 1, 2 + cap, per2.data(), masks2.data(), cap ? list.data() : nullptr, cap, &rep) != STARKHIP_OK)
                    return 4;
                bad += rep.listed != (cap < full.unmatched ? cap : full.unmatched) || rep.unmatched != full.unmatched || per2 != per || masks2 != masks;
                for (size_t i = 0; i < rep.listed; i++) {
                    const uint64_t q = list[3 * i], side = list[3 * i + 1], row = list[3 * i + 2];
                    bad += q >= NP || side > 1 || row >= n || !((masks[(q * 2 + side) * W + (row >> 6)] >> (row & 63)) & 1);
                }
            }
        }
    }
    // refusals: none of them reads the trace
    uint64_t t2[12] = {0}, seeds[STARKHIP_PERM_CHECK_ATTEMPTS];
    starkhip_perm_check_t rep = {};
    bad += starkhip_check_trace_permutations_replay(air, t2, 3, 6, 0, 5, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_check_trace_permutations_replay(air, t2, 2, 6, 0, 1, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_check_trace_permutations_replay(air, t2, 2, 6, 0, 5, nullptr, nullptr, nullptr, 1, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_check_trace_permutations_replay(air, t2, 2, 6, 0, 5, nullptr, nullptr, nullptr, 0, nullptr) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_check_trace_permutations_replay(STARKHIP_AIR_TEST_FIBONACCI, t2, 2, 2, 0, 5, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_AIR;
    bad += starkhip_check_trace_permutations(nullptr, air, t2, 2, 6, 0, 0, 5, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_NO_DEVICE;
    bad += starkhip_perm_check_seeds(2, seeds) != STARKHIP_OK || seeds[0] != 2 || seeds[1] != 15;
    bad += starkhip_perm_check_seeds(1, seeds) != STARKHIP_ERR_BAD_SHAPE;
    printf(bad ? "asan_perm_check: %d inconsistencies\n" : "asan_perm_check: ok\n", bad);
    return bad ? 1 : 0;
}
