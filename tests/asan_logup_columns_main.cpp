// Stand-alone program for the sanitizer run of the host code of LogUp lookups over Columns and Filters (make asan-logup-columns-test):
// the validator over a general section cut at every word, with a word too many, with oversized counts and with fuzzed words (whatever it
// accepts goes back to the same words, and its descriptors are built and walked to their last word); the replay of the auxiliary
// polynomials, the replay of the frequencies fill and the blob replay at 2 and 64 rows in both layouts, with output buffers of exactly
// the size the header states (an over-write is the sanitizer's to find); the fold over every row's frame.  Exit status 0 = consistent.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../include/starkhip.h"
#include "../starky_bls12_381_amd/csrc/air_ir.h"
#include "../starky_bls12_381_amd/csrc/air_validate.h"
#include "../starky_bls12_381_amd/csrc/logup.h"
#include "../starky_bls12_381_amd/csrc/logup_frequencies.h"

using namespace starkhip;
typedef AirProgram::Column Col;

static uint64_t rnd(uint64_t& s) {  // splitmix64
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// 12 columns: 0, 1 the AIR's own (0 squared in 1, both zero in the traces); table lo + 2^16 hi over columns 2, 3; selector 4; a product
// filter over 5 (zeros) and 4; values: column 6 under the selector, 7 + 3 next[8] - local[9] unfiltered, the constant 9 under the
// product filter; frequencies column 10; a second, plain lookup of column 11 in column 2 with frequencies in column 9 would read a
// value's column, so it has column 6's: lookup 1 looks column 6 up in the same table Column, frequencies 11
static AirProgram make_air() {
    AirBuilder b(12, 0, 3);
    b.constraint(b.L(1) - b.L(0) * b.L(0));
    const Col table = AirBuilder::column_of(0, {{2, 1}, {3, 1ull << 16}});
    b.logup_columns({{Col(6), AirBuilder::filter_of({}, {Col(4)})},
                     {AirBuilder::column_of(7, {{9, GL_P - 1}}, {{8, 3}}), AirProgram::Filter()},
                     {AirBuilder::column_of(9, {}), AirBuilder::filter_of({{Col(5), Col(4)}})}},
                    table, Col(10));
    b.logup_columns({{Col(6), AirBuilder::filter_of({}, {Col(4)})}}, table, Col(11));
    return b.finish();
}

static void walk_descriptor(const AirProgram& P, const std::vector<uint32_t>& d, size_t n_refs, int& bad) {
    uint32_t at = LOGUP_DESC_HEAD;
    auto cell = [&](uint32_t ref, bool) { bad += ref >= n_refs; return (gl_t)1; };
    for (size_t l = 0; l < P.logups.size(); l++) {
        const uint32_t m = d[at + 1], H = P.logup_helpers(l);
        const uint32_t* w = d.data() + at + LOGUP_DESC_LOOKUP_GENERAL + H;
        logup_desc_column(w, cell);
        logup_desc_column(w, cell);
        for (uint32_t c = 0; c < m; c++) {
            if (c % P.logup_batch_size() == 0) bad += d[at + LOGUP_DESC_LOOKUP_GENERAL + c / P.logup_batch_size()] != (uint32_t)(w - d.data());
            const uint32_t* skip = w;
            logup_desc_column(w, cell);
            logup_desc_filter(w, cell);
            logup_desc_skip_column(skip);
            logup_desc_skip_filter(skip);
            bad += skip != w;
        }
        bad += (uint32_t)(w - d.data()) != d[at + 2];
        at = d[at + 2];
    }
    bad += at != d.size();
}

int main() {
    int bad = 0;
    uint64_t s = 1;
    const AirProgram prog = make_air();
    const std::vector<uint64_t> blob = prog.serialize();
    size_t at = 0;
    while (blob[at] != AIR_LOGUP2_MAGIC) at++;
    // ---- the validator: every truncation, a word too many, oversized counts, fuzzed words
    {
        size_t passed = 0;
        auto check = [&](const std::vector<uint64_t>& t) {
            std::vector<uint64_t> exact(t);  // exactly the blob's words on the heap
            AirProgram P;
            std::string why;
            if (!air_parse_checked(exact.data(), exact.size(), &P, &why)) {
                bad += why.empty();
                return false;
            }
            passed++;
            bad += P.serialize() != exact;
            bad += P.logups.size() > STARKHIP_AIR_MAX_LOGUP_LOOKUPS || P.logup_polys() > STARKHIP_AIR_MAX_LOGUP_POLYS;
            if (P.logups.empty()) return true;
            const std::vector<uint32_t> cols = logup_columns(P);
            for (uint32_t c : cols) bad += c >= P.n_cols;
            for (const auto& lk : P.logups) {
                bad += lk.cols.empty() || lk.cols.size() > STARKHIP_AIR_MAX_LOGUP_COLUMNS || lk.cols.size() != lk.filters.size();
                for (const auto& f : lk.filters) bad += f.n_products > 4 || f.cols.size() - 2 * f.n_products > 4;
            }
            walk_descriptor(P, logup_descriptor(P, false, true), P.n_cols, bad);
            walk_descriptor(P, logup_descriptor(P, true, true), cols.size(), bad);
            std::string w2;
            if (logup_fillable(P, &w2)) {
                const LogupFreqPlan plan(P);
                bad += plan.L != P.logups.size() || plan.named.empty();
            } else {
                bad += w2.empty();
            }
            return true;
        };
        bad += !check(blob);
        for (size_t cut = at; cut < blob.size(); cut++) bad += cut > at && check(std::vector<uint64_t>(blob.begin(), blob.begin() + cut));
        std::vector<uint64_t> more = blob;
        more.push_back(0);
        bad += check(more);
        for (uint64_t big : {65ull, 1ull << 20, 1ull << 32, ~0ull, 17ull, 17ull << 32, 5ull, 5ull << 32})
            for (size_t i = at + 1; i < blob.size(); i++) {
                std::vector<uint64_t> t = blob;
                t[i] = big;
                check(t);
            }
        const uint64_t interesting[] = {0, 1, 2, 3, 4, 11, 12, 16, 1ull << 32, 4ull << 32, (1ull << 32) | 1, GL_P - 1, GL_P, ~0ull, AIR_LOGUP2_MAGIC, AIR_LOGUP_MAGIC};
        for (int trial = 0; trial < 4000; trial++) {
            std::vector<uint64_t> t = blob;
            if (trial % 5 == 4) t.resize(at + rnd(s) % (blob.size() - at + 2));
            for (int k = 0; k < 1 + trial % 2 && t.size() > at; k++)
                t[at + rnd(s) % (t.size() - at)] = trial % 3 ? interesting[rnd(s) % 16] : rnd(s) >> (rnd(s) % 64);
            check(t);
        }
        bad += passed < 50;
    }
    if (bad) return printf("validator: %d\n", bad), 1;

    // ---- the replays
    starkhip_air_t air = (starkhip_air_t)0;
    if (starkhip_air_register(blob.data(), blob.size(), "AsanLogupColumns", 0, &air) != STARKHIP_OK) return 3;
    const size_t C = prog.n_cols, nA = prog.logup_polys(), NL = 2, NC = 4;
    bad += starkhip_air_logup_general(air) != 1 || starkhip_air_logup_fillable(air) != 1 || starkhip_air_logup_columns(air) != (int)NC || nA != 10;
    bad += starkhip_air_logup_general(STARKHIP_AIR_TEST_FIBONACCI) != 0 || starkhip_air_logup_general((starkhip_air_t)123456) != STARKHIP_ERR_BAD_AIR;
    for (size_t n : {(size_t)2, (size_t)64}) {
        const size_t W = (n + 63) / 64;
        std::vector<uint64_t> rows(n * C, 0);
        for (size_t r = 0; r < n; r++) {
            rows[r * C + 2] = rnd(s) % 7 + (r % 3 == 0 ? GL_P : 0);  // some cells written as value + p; the table has duplicates
            rows[r * C + 3] = rnd(s) % 3;
            rows[r * C + 4] = rnd(s) & 1;
            rows[r * C + 8] = rnd(s) % 100;
        }
        auto tv = [&](size_t r) { return rows[r * C + 2] % GL_P + (rows[r * C + 3] << 16); };
        for (size_t r = 0; r < n; r++) {
            rows[r * C + 6] = tv(rnd(s) % n);
            // 7 + 3 next[8] - local[9] = a table value
            rows[r * C + 9] = gl_sub(gl_add(7, gl_mul(3, rows[((r + 1) % n) * C + 8])), tv(rnd(s) % n));
            rows[r * C + 10] = rows[r * C + 11] = 12345;  // to be filled
        }
        for (int layout = 0; layout < 2; layout++) {
            std::vector<uint64_t> t(n * C);
            for (size_t r = 0; r < n; r++)
                for (size_t c = 0; c < C; c++) t[layout ? c * n + r : r * C + c] = rows[r * C + c];
            const std::vector<uint64_t> before = t;
            std::vector<uint32_t> per_lookup(NL), per_column(NC);  // exactly the sizes the header states
            std::vector<uint64_t> masks(NL * W), list(2 * 4);
            starkhip_logup_report_t rep;
            if (starkhip_logup_frequencies_replay(air, t.data(), n, C, layout, per_lookup.data(), per_column.data(), masks.data(), list.data(), 4, &rep) != STARKHIP_OK) return 4;
            bad += rep.lookups != NL || rep.lookups_failed != 0 || rep.missing_cells != 0;
            uint64_t total0 = 0, total1 = 0, on = 0;
            for (size_t r = 0; r < n; r++) {
                total0 += t[layout ? 10 * n + r : r * C + 10], total1 += t[layout ? 11 * n + r : r * C + 11], on += rows[r * C + 4];
                for (size_t c = 0; c < 10; c++) bad += t[layout ? c * n + r : r * C + c] != before[layout ? c * n + r : r * C + c];
            }
            bad += total0 != n + on || total1 != on;  // the unfiltered value on every row, column 6 where the selector is on; the constant never
            uint64_t* blob_out = (uint64_t*)1;
            size_t blob_words = 7;
            bad += starkhip_logup_blob_replay(air, before.data(), n, C, layout, 4, &blob_out, &blob_words) != STARKHIP_OK || blob_out || blob_words;
            // the filled trace closes, and every row's frame satisfies every constraint
            const uint64_t ch[2] = {rnd(s) % GL_P, rnd(s) % GL_P};
            std::vector<uint64_t> polys(nA * n), closing(2 * NL);
            uint64_t zeros = 7;
            if (starkhip_logup_polys_replay(air, t.data(), n, C, layout, ch, polys.data(), closing.data(), &zeros) != STARKHIP_OK) return 5;
            for (uint64_t v : closing) bad += v != 0;
            bad += zeros != 0;
            for (size_t r = 0; r < n && !layout; r++) {
                std::vector<uint64_t> local(2 * C, 0), next(2 * C, 0), aux(2 * nA, 0), auxn(2 * nA, 0);  // exactly nA openings
                for (size_t c = 0; c < C; c++) local[2 * c] = t[r * C + c], next[2 * c] = t[((r + 1) % n) * C + c];
                for (size_t a = 0; a < nA; a++) aux[2 * a] = polys[a * n + r], auxn[2 * a] = polys[a * n + (r + 1) % n];
                const uint64_t masks8[8] = {1, 0, r + 1 < n, 0, r == 0, 0, r + 1 == n, 0};
                const uint64_t alphas[4] = {rnd(s) % GL_P, rnd(s) % GL_P, rnd(s) % GL_P, rnd(s) % GL_P};
                uint64_t acc[4];
                if (starkhip_air_eval_frame_logup(air, local.data(), next.data(), nullptr, masks8, alphas, 2, aux.data(), auxn.data(), ch, acc) != STARKHIP_OK) return 6;
                for (int j = 0; j < 4; j++) bad += acc[j] != 0;
            }
            // a filter-on cell outside the table and a filter of 2: both lookups fail on those rows, nothing is written, the blob says so
            std::vector<uint64_t> broken = before;
            size_t r_on = 0;
            while (r_on < n && !rows[r_on * C + 4]) r_on++;
            if (r_on == n) continue;
            const size_t r_two = (r_on + 1) % n;
            broken[layout ? 6 * n + r_on : r_on * C + 6] = 1ull << 40;
            broken[layout ? 4 * n + r_two : r_two * C + 4] = 2;
            std::vector<uint64_t> t2 = broken;
            if (starkhip_logup_frequencies_replay(air, t2.data(), n, C, layout, per_lookup.data(), per_column.data(), masks.data(), list.data(), 4, &rep) != STARKHIP_OK) return 7;
            bad += rep.lookups_failed != 2 || rep.missing_cells != 4 || rep.missing_rows != 4 || rep.listed != 4 || t2 != broken;
            bad += per_lookup[0] != 2 || per_lookup[1] != 2 || per_column[0] != 2 || per_column[1] != 0 || per_column[2] != 0 || per_column[3] != 2;
            if (starkhip_logup_blob_replay(air, broken.data(), n, C, layout, 4, &blob_out, &blob_words) != STARKHIP_ERR_TRACE || !blob_out) return 8;
            starkhip_logup_report_t rep2;
            const uint64_t* lst = nullptr;
            bad += starkhip_logup_blob_layout(blob_out, blob_words, &rep2, &lst) != STARKHIP_OK || rep2.missing_cells != 4 || rep2.listed != 4;
            free(blob_out);
        }
    }
    printf(bad ? "asan_logup_columns: %d inconsistencies\n" : "asan_logup_columns: ok\n", bad);
    return bad ? 1 : 0;
}
