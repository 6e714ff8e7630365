// Stand-alone program for the sanitizer run of starkhip_lookup_columns' host driver and replay (make asan-lookup-test): two inputs
// looked up in one shared table on traces of 2 .. 1024 rows, both layouts, holding and failing, with per_lookup, masks and list buffers
// of exactly the size the header states (an over-write is the sanitizer's to find), every cap from 0 to past the number of missing
// rows, every optional pointer NULL, AirBuilder::lookup, and the refusals.  The filled columns are checked for what a lookup witness
// must have.  Exit status 0 = consistent.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../include/starkhip.h"
#include "../starky_bls12_381_amd/csrc/air_ir.h"

using namespace starkhip;

static const uint64_t GLP = 0xFFFFFFFF00000001ULL;

static uint64_t rnd(uint64_t& s) {  // splitmix64
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// columns pi, pt of the row-major trace are a witness for the lookup of column a in column t
static int witness_faults(const std::vector<uint64_t>& rows, size_t n, size_t C, const starkhip_lookup_t& lk) {
    std::vector<uint64_t> a(n), t(n), pi(n), pt(n);
    for (size_t r = 0; r < n; r++) {
        a[r] = rows[r * C + lk.input] % GLP, t[r] = rows[r * C + lk.table] % GLP;
        pi[r] = rows[r * C + lk.permuted_input], pt[r] = rows[r * C + lk.permuted_table];
    }
    int bad = 0;
    for (size_t r = 0; r < n; r++) bad += pi[(r + 1) % n] != pi[r] && pi[(r + 1) % n] != pt[(r + 1) % n];
    bad += pi[0] != pt[0] || !std::is_sorted(pi.begin(), pi.end());
    std::sort(a.begin(), a.end()), std::sort(t.begin(), t.end()), std::sort(pt.begin(), pt.end());
    return bad + (a != pi) + (t != pt);
}

int main() {
    int bad = 0;
    const size_t C = 8, NL = 2;
    const starkhip_lookup_t lookups[NL] = {{0, 2, 3, 4}, {1, 2, 5, 6}};
    uint64_t s = 1;
    for (size_t n : {(size_t)2, (size_t)4, (size_t)64, (size_t)1024}) {
        const size_t W = (n + 63) / 64, m = n < 256 ? n : 256;
        std::vector<uint64_t> rows(n * C);
        for (size_t r = 0; r < n; r++) {
            for (size_t c = 0; c < C; c++) rows[r * C + c] = rnd(s);
            rows[r * C + 0] = rnd(s) % m + (r % 3 == 0 ? GLP : 0);  // some cells written as value + p
            rows[r * C + 1] = rnd(s) % m;
            rows[r * C + 2] = r % m;
        }
        for (int broken = 0; broken < 2; broken++) {
            if (broken) rows[0] = m + 5, rows[(n - 1) * C] = GLP - 1;  // two rows of lookup 0 the table lacks
            const size_t missing = broken ? 2 : 0;
            std::vector<uint64_t> cols(n * C);
            for (size_t r = 0; r < n; r++)
                for (size_t c = 0; c < C; c++) cols[c * n + r] = rows[r * C + c];
            starkhip_lookup_report_t full = {}, rep = {};
            std::vector<uint32_t> per(NL), per2(NL);
            std::vector<uint64_t> masks(NL * W), masks2(NL * W), filled = rows;
            if (starkhip_lookup_columns_replay(filled.data(), n, C, 0, lookups, NL, per.data(), masks.data(), nullptr, 0, &full) != STARKHIP_OK) return 3;
            bad += full.lookups != NL || full.lookups_failed != (broken ? 1u : 0u) || full.missing_rows != missing || full.listed != 0;
            bad += per[0] != missing || per[1] != 0;
            uint64_t bits = 0;
            for (uint64_t w : masks) bits += (uint64_t)__builtin_popcountll(w);
            bad += bits != missing;
            for (size_t r = 0; r < n; r++)  // nothing but the output columns of the lookups that hold
                for (size_t c = 0; c < C; c++) bad += (c < (broken ? 5u : 3u) || c == 7) && filled[r * C + c] != rows[r * C + c];
            if (!broken) bad += witness_faults(filled, n, C, lookups[0]);
            bad += witness_faults(filled, n, C, lookups[1]);
            for (size_t cap = 0; cap <= missing + 2; cap++) {
                std::vector<uint64_t> list(2 * cap), fc = cols;  // exactly cap entries
                if (starkhip_lookup_columns_replay(fc.data(), n, C, 1, lookups, NL, per2.data(), masks2.data(), cap ? list.data() : nullptr, cap, &rep) != STARKHIP_OK)
                    return 4;
                bad += rep.listed != (cap < missing ? cap : missing) || rep.missing_rows != missing || per2 != per || masks2 != masks;
                for (size_t i = 0; i < rep.listed; i++) bad += list[2 * i] != 0 || list[2 * i + 1] != (i ? n - 1 : 0);
                for (size_t r = 0; r < n; r++)
                    for (size_t c = 0; c < C; c++) bad += fc[c * n + r] != filled[r * C + c];  // both layouts, the same columns
            }
            std::vector<uint64_t> again = rows;  // every optional pointer NULL
            if (starkhip_lookup_columns_replay(again.data(), n, C, 0, lookups, NL, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_OK) return 5;
            bad += again != filled || rep.missing_rows != missing;
        }
    }
    // AirBuilder::lookup: two constraints and two pairs per lookup, and a program the registry takes
    AirBuilder b(7, 0, 3);
    b.lookup(0, 2, 3, 4);
    b.lookup(1, 2, 5, 6);
    bad += b.count() != 4 || b.lookups().size() != 2 || b.lookups()[1].permuted_table != 6;
    const AirProgram prog = b.finish();
    bad += prog.perm_pairs.size() != 4 || prog.perm_pairs[1][0] != (2ull | 4ull << 32);
    const std::vector<uint64_t> blob = prog.serialize();
    starkhip_air_t air = (starkhip_air_t)0;
    bad += starkhip_air_register(blob.data(), blob.size(), "AsanLookup", 0, &air) != STARKHIP_OK;
    std::vector<uint64_t> from_c(blob.size());
    size_t words = 0;
    bad += starkhip_lookup_air_blob(7, 3, lookups, NL, from_c.data(), from_c.size(), &words) != STARKHIP_OK || words != blob.size() || from_c != blob;
    bad += starkhip_lookup_air_blob(7, 3, lookups, NL, from_c.data(), from_c.size() - 1, &words) != STARKHIP_ERR_BAD_SHAPE;
    // refusals: none of them reads or writes the trace
    uint64_t t2[16] = {0};
    starkhip_lookup_report_t rep = {};
    const starkhip_lookup_t high = {0, 2, 3, 8}, own = {0, 2, 0, 4}, twin = {0, 2, 3, 3}, clash[2] = {{0, 2, 3, 4}, {1, 2, 5, 3}};
    bad += starkhip_lookup_columns_replay(t2, 3, 5, 0, lookups, 1, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 2, lookups, NL, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 0, lookups, 0, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 0, lookups, STARKHIP_LOOKUPS_MAX + 1, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 0, nullptr, 1, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(nullptr, 2, 8, 0, lookups, NL, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 0, &high, 1, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 0, &own, 1, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 0, &twin, 1, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 0, clash, 2, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 0, lookups, NL, nullptr, nullptr, nullptr, 1, &rep) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns_replay(t2, 2, 8, 0, lookups, NL, nullptr, nullptr, nullptr, 0, nullptr) != STARKHIP_ERR_BAD_SHAPE;
    bad += starkhip_lookup_columns(nullptr, t2, 2, 8, 0, 0, lookups, NL, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_NO_DEVICE;
    for (uint64_t w : t2) bad += w != 0;
    printf(bad ? "asan_lookup: %d inconsistencies\n" : "asan_lookup: ok\n", bad);
    return bad ? 1 : 0;
}
