// Stand-alone program for the sanitizer run of what "fill_lookups" adds to the host code (make asan-lookup-fill-test): the check of a
// lookup list against a program and the registry keyed by (blob, list); the host driver of the lookups in uneven batches over the
// replay steps -- five lookups as 2, 2, 1, as 3, 2, one by one and all at once, with per_lookup, masks and list buffers of exactly the
// size the header states -- which must not depend on the batch; the lookup blob's builder and parser on blobs of exactly their
// length.  Exit status 0 = consistent.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/starkhip.h"
#include "../starky_bls12_381_amd/csrc/air_ir.h"
#include "../starky_bls12_381_amd/csrc/lookup_columns.h"

using namespace starkhip;

static uint64_t rnd(uint64_t& s) {  // splitmix64
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static const size_t C = 17, NL = 5;

static std::vector<starkhip_lookup_t> five() {
    std::vector<starkhip_lookup_t> l;
    for (uint32_t q = 0; q < NL; q++) l.push_back({q, q < 3 ? 5u : 6u, 7 + 2 * q, 8 + 2 * q});
    return l;
}

static std::vector<uint64_t> program(const std::vector<starkhip_lookup_t>& lookups, std::vector<starkhip_lookup_t>* from_builder) {
    AirBuilder b(C, 0, 5);
    for (const starkhip_lookup_t& lk : lookups) b.lookup(lk.input, lk.table, lk.permuted_input, lk.permuted_table);
    const std::vector<uint64_t> blob = b.finish().serialize();
    if (from_builder)
        for (const AirBuilder::Lookup& lk : b.lookups()) from_builder->push_back({lk.input, lk.table, lk.permuted_input, lk.permuted_table});
    return blob;
}

static int refused(const std::vector<uint64_t>& blob, const std::vector<starkhip_lookup_t>& l, size_t n, const char* word) {
    char why[200];  // exactly the length passed on
    memset(why, 'x', sizeof why);
    const int rc = starkhip_air_check_lookups(blob.data(), blob.size(), l.data(), n, why, sizeof why);
    starkhip_air_t id = (starkhip_air_t)0;
    const int rc2 = starkhip_air_register_lookups(blob.data(), blob.size(), "AsanRefused", 0, l.data(), n, &id);
    return (rc != STARKHIP_ERR_BAD_AIR) + (rc2 != STARKHIP_ERR_BAD_AIR) + (strstr(why, word) == nullptr);
}

int main() {
    int bad = 0;
    // ---- registration
    std::vector<starkhip_lookup_t> lookups = five(), built;
    const std::vector<uint64_t> blob = program(lookups, &built);
    bad += built.size() != NL || memcmp(built.data(), lookups.data(), NL * sizeof(starkhip_lookup_t)) != 0;
    char tiny[4];
    bad += starkhip_air_check_lookups(blob.data(), blob.size(), lookups.data(), NL, nullptr, 0) != STARKHIP_OK;
    bad += starkhip_air_check_lookups(blob.data(), blob.size(), lookups.data(), 0, tiny, sizeof tiny) != STARKHIP_ERR_BAD_AIR || strlen(tiny) != 3;  // cut to fit
    {
        std::vector<starkhip_lookup_t> l = lookups;
        l[1].table = C;
        bad += refused(blob, l, NL, "out of range");
        l = lookups, l[4].permuted_input = l[0].input;
        bad += refused(blob, l, NL, "is the input of lookup 0");
        l = lookups, l[2].permuted_table = 6;
        bad += refused(blob, l, NL, "is the table of lookup 3");
        l = lookups, l[3].permuted_table = l[1].permuted_input;
        bad += refused(blob, l, NL, "also an output");
        l = lookups, l[0].permuted_table = l[0].permuted_input;
        bad += refused(blob, l, NL, "are both column");
        l.assign(STARKHIP_LOOKUPS_MAX + 1, lookups[0]);
        bad += refused(blob, l, l.size(), "at most");
        bad += refused(blob, lookups, 0, "no lookups");
        // a program that binds four of the five lookups: the fifth's pairs are not declared
        const std::vector<uint64_t> four = program(std::vector<starkhip_lookup_t>(lookups.begin(), lookups.begin() + 4), nullptr);
        bad += refused(four, lookups, NL, "declares no permutation pair [(4, 15)]");
        bad += starkhip_air_check_lookups(four.data(), four.size(), lookups.data(), 4, nullptr, 0) != STARKHIP_OK;
        bad += refused(std::vector<uint64_t>(blob.begin(), blob.end() - 1), lookups, NL, "");  // a truncated program
    }
    starkhip_air_t a = (starkhip_air_t)0, again = (starkhip_air_t)0, plain = (starkhip_air_t)0, part = (starkhip_air_t)0;
    bad += starkhip_air_register_lookups(blob.data(), blob.size(), "AsanFill", 64, lookups.data(), NL, &a) != STARKHIP_OK;
    bad += starkhip_air_register_lookups(blob.data(), blob.size(), nullptr, 0, lookups.data(), NL, &again) != STARKHIP_OK || again != a;
    bad += starkhip_air_register(blob.data(), blob.size(), nullptr, 0, &plain) != STARKHIP_OK || plain == a;
    bad += starkhip_air_register_lookups(blob.data(), blob.size(), nullptr, 0, lookups.data(), 2, &part) != STARKHIP_OK || part == a || part == plain;
    bad += starkhip_air_register_lookups(blob.data(), blob.size(), nullptr, 0, lookups.data(), NL, nullptr) != STARKHIP_ERR_BAD_SHAPE;
    {
        std::vector<starkhip_lookup_t> out(NL);  // exactly the entries asked for
        bad += starkhip_air_lookups(a, out.data(), NL) != NL || memcmp(out.data(), lookups.data(), NL * sizeof(starkhip_lookup_t)) != 0;
        std::vector<starkhip_lookup_t> two(2);
        bad += starkhip_air_lookups(a, two.data(), 2) != NL || two[1].permuted_table != lookups[1].permuted_table;
        bad += starkhip_air_lookups(a, nullptr, 0) != NL || starkhip_air_lookups(part, two.data(), 2) != 2;
        bad += starkhip_air_lookups(plain, out.data(), NL) != 0 || starkhip_air_lookups(STARKHIP_AIR_FP12_MUL, out.data(), NL) != 0;
        bad += starkhip_air_lookups((starkhip_air_t)99999, nullptr, 0) != 0;
    }
    // ---- the host driver in uneven batches over the replay steps
    uint64_t s = 7;
    for (size_t n : {(size_t)2, (size_t)64, (size_t)512}) {
        const size_t W = (n + 63) / 64, m = n < 256 ? n : 256;
        std::vector<uint64_t> rows(n * C);
        for (size_t r = 0; r < n; r++) {
            for (size_t c = 0; c < C; c++) rows[r * C + c] = rnd(s) | 1;
            for (size_t c = 0; c < 5; c++) rows[r * C + c] = rnd(s) % m;
            rows[r * C + 5] = r % m, rows[r * C + 6] = (n - 1 - r) % m;
        }
        for (int broken = 0; broken < 2; broken++) {
            if (broken) rows[1] = m + 3, rows[(n - 1) * C + 1] = m + 4, rows[3] = m + 9;  // lookup 1 misses rows 0 and n - 1, lookup 3 row 0
            const size_t missing = broken ? 3 : 0;
            std::vector<uint64_t> want;
            std::vector<uint32_t> want_per;
            std::vector<uint64_t> want_masks, want_list;
            for (size_t batch : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)64}) {
                for (size_t cap : {(size_t)0, (size_t)2, (size_t)4}) {
                    std::vector<uint64_t> filled = rows, masks(NL * W), list(2 * cap);
                    std::vector<uint32_t> per(NL);
                    starkhip_lookup_report_t rep = {};
                    const TraceInput mine = TraceInput::dense(filled.data(), n, C, 0, 0);
                    if (lookup_columns_replay(mine, filled.data(), lookups.data(), NL, per.data(), masks.data(), cap ? list.data() : nullptr, cap, &rep, batch) != STARKHIP_OK)
                        return 3;
                    bad += rep.lookups != NL || rep.lookups_failed != (broken ? 2u : 0u) || rep.missing_rows != missing || rep.listed != (cap < missing ? cap : missing);
                    if (want.empty()) want = filled, want_per = per, want_masks = masks;
                    bad += filled != want || per != want_per || masks != want_masks;  // whatever the batch and the cap
                    if (cap == 4) {
                        if (want_list.empty()) want_list = list;
                        bad += list != want_list;
                        if (broken) bad += list[0] != 1 || list[1] != 0 || list[2] != 1 || list[3] != n - 1 || list[4] != 3 || list[5] != 0;
                    }
                    for (size_t r = 0; r < n && broken; r++)  // the failed lookups keep their columns, in the middle of a batch too
                        for (uint32_t c : {9u, 10u, 13u, 14u}) bad += filled[r * C + c] != rows[r * C + c];
                }
            }
            // ---- the blob of this trace: builder, parser, and the replay that prove() must match
            for (size_t cap : {(size_t)0, (size_t)1, (size_t)16}) {
                uint64_t* lb = nullptr;
                size_t words = 1;
                const std::vector<uint64_t> before = rows;
                const int rc = starkhip_lookup_blob_replay(a, rows.data(), n, C, 0, cap, &lb, &words);
                bad += rows != before;
                if (!broken) {
                    bad += rc != STARKHIP_OK || lb != nullptr || words != 0;
                    continue;
                }
                const size_t listed = cap < missing ? cap : missing;
                if (rc != STARKHIP_ERR_TRACE || !lb || words != 8 + 2 * listed) return 4;
                std::vector<uint64_t> exact(lb, lb + words);  // a copy of exactly its length: the parser reads no further
                starkhip_free(lb);
                starkhip_lookup_report_t rep = {};
                const uint64_t* list = nullptr;
                bad += starkhip_lookup_blob_layout(exact.data(), exact.size(), &rep, &list) != STARKHIP_OK;
                bad += exact[0] != STARKHIP_LOOKUP_MAGIC || exact[1] != (uint64_t)a || exact[2] != n || exact[7] != 0;
                bad += rep.lookups != NL || rep.lookups_failed != 2 || rep.missing_rows != 3 || rep.listed != listed;
                bad += (list != nullptr) != (listed != 0) || (list && (list != exact.data() + 8 || list[0] != 1 || list[1] != 0));
                bad += starkhip_lookup_blob_layout(exact.data(), exact.size(), &rep, nullptr) != STARKHIP_OK;
                bad += starkhip_lookup_blob_layout(exact.data(), exact.size() - 1, &rep, &list) != STARKHIP_ERR_BAD_SHAPE;
                bad += starkhip_lookup_blob_layout(exact.data(), 7, &rep, &list) != STARKHIP_ERR_BAD_SHAPE;
                bad += starkhip_lookup_blob_layout(exact.data(), exact.size(), nullptr, &list) != STARKHIP_ERR_BAD_SHAPE;
                bad += starkhip_lookup_blob_layout(nullptr, 8, &rep, &list) != STARKHIP_ERR_BAD_SHAPE;
                starkhip_check_report_t crep = {};
                bad += starkhip_check_blob_layout(exact.data(), exact.size(), &crep, nullptr) != STARKHIP_ERR_BAD_SHAPE;
                std::vector<uint64_t> wrong = exact;
                wrong[6] += 1;  // listed disagrees with the length
                bad += starkhip_lookup_blob_layout(wrong.data(), wrong.size(), &rep, &list) != STARKHIP_ERR_BAD_SHAPE;
                wrong = exact, wrong[0] = STARKHIP_CHECK_MAGIC;
                bad += starkhip_lookup_blob_layout(wrong.data(), wrong.size(), &rep, &list) != STARKHIP_ERR_BAD_SHAPE;
                wrong = exact, wrong[0] = STARKHIP_PROOF_MAGIC;
                bad += starkhip_lookup_blob_layout(wrong.data(), wrong.size(), &rep, &list) != STARKHIP_ERR_BAD_SHAPE;
            }
            uint64_t* lb = nullptr;
            size_t words = 0;
            bad += starkhip_lookup_blob_replay(plain, rows.data(), n, C, 0, 16, &lb, &words) != STARKHIP_OK || lb != nullptr;  // no list: nothing to refuse
            bad += starkhip_lookup_blob_replay(a, rows.data(), n, C + 1, 0, 16, &lb, &words) != STARKHIP_ERR_BAD_SHAPE;
            bad += starkhip_lookup_blob_replay(a, rows.data(), n, C, 0, 16, nullptr, &words) != STARKHIP_ERR_BAD_SHAPE;
            bad += starkhip_lookup_blob_replay((starkhip_air_t)99999, rows.data(), n, C, 0, 16, &lb, &words) != STARKHIP_ERR_BAD_AIR;
        }
    }
    // the batch rule: all lookups inside the budget, never none, the limit on top
    bad += lookup_batch_size(1024, 64, 0) != 64 || lookup_batch_size((size_t)1 << 20, 8, 0) != 2 || lookup_batch_size((size_t)1 << 16, 64, 0) != 32;
    bad += lookup_batch_size((size_t)1 << 16, 32, 0) != 32 || lookup_batch_size((size_t)1 << 20, 1, 0) != 1 || lookup_batch_size(512, 5, 2) != 2;
    bad += lookup_batch_size((size_t)1 << 20, 8, 64) != 2;
    printf(bad ? "asan_lookup_fill: %d inconsistencies\n" : "asan_lookup_fill: ok\n", bad);
    return bad ? 1 : 0;
}
