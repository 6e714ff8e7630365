// Stand-alone program for the sanitizer run of the host code of starkhip_logup_frequencies (make asan-logup-freq-test): the fillable
// test, the host driver over the replay steps in both layouts with per_lookup, per_column, masks and list buffers of exactly the size
// the header states, against a count written here; a failing lookup beside ones that hold; the LogUp blob's builder, parser and
// replay on blobs of exactly their length; every refusal of the entries.  Exit status 0 = consistent.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/starkhip.h"
#include "../starky_bls12_381_amd/csrc/air_ir.h"
#include "../starky_bls12_381_amd/csrc/gl.h"
#include "../starky_bls12_381_amd/csrc/logup_frequencies.h"

using namespace starkhip;

static uint64_t rnd(uint64_t& s) {  // splitmix64
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

struct Lk { std::vector<uint32_t> cols; uint32_t table, freq; };

// columns: 0 the program's own, 1 and 2 tables; lookup 0 = {3, 4} in 1 -> 5, lookup 1 = {6} in 2 -> 7, lookup 2 = {8, 9, 10} in 1 -> 11
static const size_t C = 12;
static std::vector<Lk> three() { return {{{3, 4}, 1, 5}, {{6}, 2, 7}, {{8, 9, 10}, 1, 11}}; }

static int register_air(const std::vector<Lk>& lks, size_t n_cols, starkhip_air_t* id) {
    AirBuilder b((uint32_t)n_cols, 1, 3);
    b.transition(b.N(0) - b.L(0) - (uint64_t)1);
    b.first_row(b.L(0) - b.PI(0));
    for (const Lk& l : lks) b.logup(l.cols, l.table, l.freq);
    const std::vector<uint64_t> blob = b.finish().serialize();
    return starkhip_air_register(blob.data(), blob.size(), nullptr, 0, id);
}

// row-major [n][C]: tables with duplicates (some written as v + p), every looked-up cell from its table, frequencies junk
static std::vector<uint64_t> make_trace(size_t n, uint64_t seed) {
    std::vector<uint64_t> t(n * C);
    for (size_t r = 0; r < n; r++) {
        t[r * C] = r + 1;
        for (size_t c : {1, 2}) t[r * C + c] = 5 + 3 * (rnd(seed) % (n / 2 + 1)) + (rnd(seed) % 3 == 0 ? GL_P : 0);
    }
    for (const Lk& l : three())
        for (size_t r = 0; r < n; r++) {
            for (uint32_t c : l.cols) t[r * C + c] = t[(rnd(seed) % n) * C + l.table] % GL_P + (rnd(seed) % 4 == 0 ? GL_P : 0);
            t[r * C + l.freq] = rnd(seed);
        }
    return t;
}

static std::vector<uint64_t> transposed(const std::vector<uint64_t>& t, size_t n) {
    std::vector<uint64_t> o(t.size());
    for (size_t r = 0; r < n; r++)
        for (size_t c = 0; c < C; c++) o[c * n + r] = t[r * C + c];
    return o;
}

// the rule, written out: f of lookup l for the row-major trace t, or false when a cell is missing
static bool expect(const std::vector<uint64_t>& t, size_t n, const Lk& l, std::vector<uint64_t>* f) {
    f->assign(n, 0);
    for (size_t r = 0; r < n; r++)
        for (uint32_t c : l.cols) {
            const uint64_t v = t[r * C + c] % GL_P;
            size_t first = n;
            for (size_t k = 0; k < n && first == n; k++)
                if (t[k * C + l.table] % GL_P == v) first = k;
            if (first == n) return false;
            (*f)[first]++;
        }
    return true;
}

int main() {
    int bad = 0;
    starkhip_air_t air = (starkhip_air_t)0, plain = (starkhip_air_t)0, unfillable = (starkhip_air_t)0;
    bad += register_air(three(), C, &air) != STARKHIP_OK;
    bad += register_air({}, C, &plain) != STARKHIP_OK;
    {
        std::vector<Lk> l = three();
        l[1].cols[0] = 5;  // lookup 1 looks lookup 0's frequencies up
        bad += register_air(l, C, &unfillable) != STARKHIP_OK;
    }
    bad += starkhip_air_logup_fillable(air) != 1 || starkhip_air_logup_fillable(unfillable) != 0;
    bad += starkhip_air_logup_fillable(plain) != STARKHIP_ERR_BAD_AIR || starkhip_air_logup_fillable((starkhip_air_t)123456) != STARKHIP_ERR_BAD_AIR;
    {
        AirBuilder b(C, 1, 3);
        b.logup({3, 4}, 1, 5);
        b.logup({6}, 5, 7);
        std::string why;
        bad += logup_fillable(b.finish(), &why) || why.find("table column of lookup 1") == std::string::npos;
    }
    if (bad) return printf("registration: %d\n", bad), 1;

    // ---- the driver over the replay steps, exact buffers
    const size_t NL = 3, NC = 6;
    for (size_t n : {2, 4, 64, 256}) {
        const size_t W = (n + 63) / 64;
        for (int layout = 0; layout < 2; layout++)
            for (int fail = 0; fail < 2; fail++) {
                std::vector<uint64_t> rows = make_trace(n, 11 * n + fail);
                if (fail) {  // lookup 2: two cells of row n - 1 and one of row 0 miss table 1; the others hold
                    rows[(n - 1) * C + 8] = 1, rows[(n - 1) * C + 10] = 2 + GL_P, rows[0 * C + 9] = 4;
                }
                std::vector<uint64_t> t = layout ? transposed(rows, n) : rows;
                const std::vector<uint64_t> before = t;
                std::vector<uint32_t> per_lookup(NL, 7), per_column(NC, 7);
                std::vector<uint64_t> masks(NL * W, ~0ull);
                for (size_t cap : {(size_t)0, (size_t)1, (size_t)8}) {
                    std::vector<uint64_t> list(2 * cap, ~0ull);
                    starkhip_logup_report_t rep;
                    t = before;
                    const int rc = starkhip_logup_frequencies_replay(air, t.data(), n, C, layout, per_lookup.data(), per_column.data(), masks.data(),
                                                                     cap ? list.data() : nullptr, cap, &rep);
                    bad += rc != STARKHIP_OK;
                    const uint64_t rows_missing = fail ? 2 : 0;  // rows 0 and n - 1
                    bad += rep.lookups != NL || rep.lookups_failed != (uint64_t)fail || rep.missing_cells != (fail ? 3u : 0u) || rep.missing_rows != rows_missing;
                    bad += rep.listed != (cap < rows_missing ? cap : rows_missing);
                    bad += per_lookup[0] != 0 || per_lookup[1] != 0 || per_lookup[2] != (fail ? 3u : 0u);
                    bad += per_column[3] != (uint32_t)fail || per_column[4] != (uint32_t)fail || per_column[5] != (uint32_t)fail || per_column[0] + per_column[1] + per_column[2] != 0;
                    if (fail && cap >= 1) bad += list[0] != 2 || list[1] != 0;
                    if (fail && cap >= 2) bad += list[2] != 2 || list[3] != n - 1;
                    const std::vector<Lk> lks = three();
                    for (size_t q = 0; q < NL; q++) {
                        std::vector<uint64_t> f;
                        const bool holds = expect(rows, n, lks[q], &f);
                        bad += holds != !(fail && q == 2);
                        for (size_t r = 0; r < n; r++) {
                            const size_t at = layout ? lks[q].freq * n + r : r * C + lks[q].freq;
                            bad += t[at] != (holds ? f[r] : before[at]);
                            bad += ((masks[q * W + (r >> 6)] >> (r & 63)) & 1) != (uint64_t)(!holds && (r == 0 || r == n - 1));
                        }
                    }
                    for (size_t i = 0; i < t.size(); i++) {  // nothing but the frequencies columns is written
                        const size_t c = layout ? i / n : i % C;
                        if (c != 5 && c != 7 && c != 11) bad += t[i] != before[i];
                    }
                    // ---- the blob of the same trace
                    uint64_t* blob = nullptr;
                    size_t words = 99;
                    const int brc = starkhip_logup_blob_replay(air, before.data(), n, C, layout, cap, &blob, &words);
                    if (!fail) bad += brc != STARKHIP_OK || blob != nullptr || words != 0;
                    else {
                        bad += brc != STARKHIP_ERR_TRACE || !blob || words != LOGUP_BLOB_HEADER + 2 * rep.listed;
                        if (blob) {
                            std::vector<uint64_t> exact(blob, blob + words);  // a copy of exactly its length: reads past it are seen
                            starkhip_free(blob);
                            starkhip_logup_report_t got;
                            const uint64_t* lst = nullptr;
                            bad += starkhip_logup_blob_layout(exact.data(), exact.size(), &got, &lst) != STARKHIP_OK;
                            bad += memcmp(&got, &rep, sizeof rep) != 0 || (rep.listed ? lst != exact.data() + LOGUP_BLOB_HEADER : lst != nullptr);
                            bad += exact[0] != STARKHIP_LOGUP_MAGIC || exact[2] != n || exact[7] != 3;
                            if (rep.listed) bad += memcmp(lst, list.data(), 2 * rep.listed * 8) != 0;
                            starkhip_lookup_report_t other;
                            bad += starkhip_lookup_blob_layout(exact.data(), exact.size(), &other, nullptr) != STARKHIP_ERR_BAD_SHAPE;
                            for (size_t cut = 0; cut < exact.size(); cut++) {  // every truncation
                                std::vector<uint64_t> part(exact.begin(), exact.begin() + cut);
                                bad += starkhip_logup_blob_layout(part.data(), part.size(), &got, nullptr) != STARKHIP_ERR_BAD_SHAPE;
                            }
                            exact[0] = STARKHIP_LOOKUP_MAGIC;
                            bad += starkhip_logup_blob_layout(exact.data(), exact.size(), &got, nullptr) != STARKHIP_ERR_BAD_SHAPE;
                        }
                    }
                }
            }
        if (bad) return printf("driver at %zu rows: %d\n", n, bad), 1;
    }

    // ---- refusals
    {
        std::vector<uint64_t> t = make_trace(64, 5);
        starkhip_logup_report_t rep;
        uint64_t list[2];
        uint64_t* blob = nullptr;
        size_t words = 0;
        bad += starkhip_logup_frequencies(nullptr, air, t.data(), 64, C, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_NO_DEVICE;
        bad += starkhip_logup_frequency_timings(nullptr, nullptr) != STARKHIP_ERR_NO_DEVICE;
        bad += starkhip_logup_frequencies_replay(plain, t.data(), 64, C, 0, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_AIR;
        bad += starkhip_logup_frequencies_replay((starkhip_air_t)123456, t.data(), 64, C, 0, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_AIR;
        bad += starkhip_logup_frequencies_replay(unfillable, t.data(), 64, C, 0, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_blob_replay(unfillable, t.data(), 64, C, 0, 4, &blob, &words) != STARKHIP_ERR_BAD_AIR;
        bad += starkhip_logup_blob_replay(plain, t.data(), 64, C, 0, 4, &blob, &words) != STARKHIP_ERR_BAD_AIR;
        bad += starkhip_logup_blob_replay(air, t.data(), 64, C, 0, 4, nullptr, &words) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, nullptr, 64, C, 0, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, t.data(), 64, C, 2, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, t.data(), 64, C + 1, 0, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, t.data(), 48, C, 0, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, t.data(), 1, C, 0, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, t.data(), (size_t)1 << (STARKHIP_MAX_LOG_ROWS + 1), C, 0, nullptr, nullptr, nullptr, nullptr, 0, &rep) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, t.data(), 64, C, 0, nullptr, nullptr, nullptr, list, (size_t)STARKHIP_CHECK_LIST_MAX + 1, &rep) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, t.data(), 64, C, 0, nullptr, nullptr, nullptr, nullptr, 1, &rep) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, t.data(), 64, C, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr) != STARKHIP_ERR_BAD_SHAPE;
        bad += starkhip_logup_frequencies_replay(air, t.data(), 64, C, 0, nullptr, nullptr, nullptr, list, 1, &rep) != STARKHIP_OK || rep.lookups_failed != 0;
        bad += starkhip_logup_blob_layout(nullptr, 8, &rep, nullptr) != STARKHIP_ERR_BAD_SHAPE;
    }
    if (bad) return printf("refusals: %d\n", bad), 1;
    printf("asan logup frequencies ok\n");
    return 0;
}
