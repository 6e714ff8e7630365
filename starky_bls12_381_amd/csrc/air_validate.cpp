// Validation of a caller's constraint program (air_validate.h).
#include "air_validate.h"

#include <algorithm>

namespace starkhip {

namespace {
bool refuse(std::string* why, const std::string& msg) {
    if (why) *why = msg;
    return false;
}
// one COLUMN of the general LogUp section (air_ir.h) at sec[*at], of a program of n_cols columns; *at moves past it
bool read_column(const uint64_t* sec, uint64_t sec_words, uint64_t* at_io, uint64_t n_cols, AirProgram::Column* c, std::string* msg) {
    uint64_t at = *at_io;
    if (sec_words < at || sec_words - at < 2) return *msg = "runs past the blob", false;
    const uint64_t nl = sec[at] & 0xFFFFFFFFu, nn = sec[at] >> 32, constant = sec[at + 1];
    at += 2;
    if (nl + nn > AIR_LOGUP_MAX_TERMS) return *msg = "Column of " + std::to_string(nl + nn) + " terms (at most " + std::to_string(AIR_LOGUP_MAX_TERMS) + ")", false;
    if (constant >= GL_P) return *msg = "Column constant is not canonical", false;
    if ((sec_words - at) / 2 < nl + nn) return *msg = "Column terms run past the blob", false;
    c->n_local = (uint32_t)nl;
    c->constant = constant;
    for (uint64_t k = 0; k < nl + nn; k++, at += 2) {
        if (sec[at] >= n_cols) return *msg = "column " + std::to_string(sec[at]) + " out of range", false;
        if (sec[at + 1] == 0) return *msg = "Column coefficient is zero", false;
        if (sec[at + 1] >= GL_P) return *msg = "Column coefficient is not canonical", false;
        c->terms.push_back({(uint32_t)sec[at], sec[at + 1]});
    }
    *at_io = at;
    return true;
}
}  // namespace

// A system blob (ctl.h): SYSTEM_MAGIC, T, the T table ids, K, then per CTL: width, L, and its 1 + L endpoints, the looked one first:
//   table, width (again), width COLUMNs, FILTER      (COLUMN and FILTER as in the general LogUp section, air_ir.h)
bool system_parse_checked(const uint64_t* blob, size_t words, const std::function<const AirProgram*(int)>& air_of, SystemProgram* out, std::string* why) {
    if (!blob || words < 3) return refuse(why, "system blob shorter than its header");
    if (blob[0] != SYSTEM_MAGIC) return refuse(why, "bad magic (not a SYSCTL01 system)");
    const uint64_t T = blob[1], W = words;
    if (T < 2 || T > SYSTEM_MAX_TABLES) return refuse(why, "a system of " + std::to_string(T) + " tables (2.." + std::to_string(SYSTEM_MAX_TABLES) + ")");
    if (W < 3 + T) return refuse(why, "table ids run past the blob");
    SystemProgram S;
    std::vector<const AirProgram*> progs;
    for (uint64_t t = 0; t < T; t++) {
        const std::string att = "table " + std::to_string(t) + ": ";
        const AirProgram* P = blob[2 + t] <= 0x7FFFFFFFu ? air_of((int)blob[2 + t]) : nullptr;
        if (!P) return refuse(why, att + "table id " + std::to_string(blob[2 + t]) + " is not a registered AIR");
        if (!P->perm_pairs.empty()) return refuse(why, att + "an AIR with permutation pairs cannot be a table of a system (its Zs take the middle matrix)");
        if (P->degree < 2) return refuse(why, att + "cross-table lookups need degree >= 2 (h c - filter has degree 2)");
        S.airs.push_back((int)blob[2 + t]);
        progs.push_back(P);
    }
    uint64_t at = 2 + T;
    const uint64_t K = blob[at++];
    if (K > SYSTEM_MAX_CTLS) return refuse(why, "a system of " + std::to_string(K) + " CTLs (at most " + std::to_string(SYSTEM_MAX_CTLS) + ")");
    std::vector<uint64_t> eps_of(T, 0);
    std::string msg;
    for (uint64_t k = 0; k < K; k++) {
        const std::string atk = "CTL " + std::to_string(k) + ": ";
        if (W < at || W - at < 2) return refuse(why, atk + "runs past the blob");
        const uint64_t width = blob[at], L = blob[at + 1];
        at += 2;
        if (width < 1 || width > CTL_MAX_WIDTH) return refuse(why, atk + "width " + std::to_string(width) + " outside 1.." + std::to_string(CTL_MAX_WIDTH));
        if (L < 1 || L > SYSTEM_MAX_LOOKING) return refuse(why, atk + std::to_string(L) + " looking endpoints (1.." + std::to_string(SYSTEM_MAX_LOOKING) + ")");
        Ctl ctl;
        ctl.width = (uint32_t)width;
        for (uint64_t e = 0; e <= L; e++) {
            const std::string ate = atk + (e == 0 ? std::string("looked endpoint: ") : "looking endpoint " + std::to_string(e - 1) + ": ");
            if (W < at || W - at < 2) return refuse(why, ate + "runs past the blob");
            const uint64_t table = blob[at], w_e = blob[at + 1];
            at += 2;
            if (table >= T) return refuse(why, ate + "table " + std::to_string(table) + " out of range (the system has " + std::to_string(T) + ")");
            if (w_e != width) return refuse(why, ate + "width mismatch: " + std::to_string(w_e) + " columns, the CTL has " + std::to_string(width));
            CtlEndpoint ep;
            ep.table = (uint32_t)table;
            ep.ctl = (uint32_t)k;
            ep.looked = e == 0;
            const uint64_t n_cols = progs[table]->n_cols;
            for (uint64_t j = 0; j < width; j++) {
                AirProgram::Column c;
                if (!read_column(blob, W, &at, n_cols, &c, &msg)) return refuse(why, ate + "column " + std::to_string(j) + ": " + msg);
                ep.cols.push_back(std::move(c));
            }
            if (at >= W) return refuse(why, ate + "filter runs past the blob");
            const uint64_t np = blob[at] & 0xFFFFFFFFu, ns = blob[at] >> 32;
            at++;
            if (np > AIR_LOGUP_MAX_FILTER_PRODUCTS) return refuse(why, ate + "filter of " + std::to_string(np) + " products (at most " + std::to_string(AIR_LOGUP_MAX_FILTER_PRODUCTS) + ")");
            if (ns > AIR_LOGUP_MAX_FILTER_SUMS) return refuse(why, ate + "filter of " + std::to_string(ns) + " sums (at most " + std::to_string(AIR_LOGUP_MAX_FILTER_SUMS) + ")");
            ep.filter.n_products = (uint32_t)np;
            for (uint64_t j = 0; j < 2 * np + ns; j++) {
                AirProgram::Column fc;
                if (!read_column(blob, W, &at, n_cols, &fc, &msg)) return refuse(why, ate + "filter: " + msg);
                ep.filter.cols.push_back(std::move(fc));
            }
            eps_of[table]++;
            if (e == 0) ctl.looked = std::move(ep);
            else ctl.looking.push_back(std::move(ep));
        }
        S.ctls.push_back(std::move(ctl));
    }
    if (at != W) return refuse(why, "trailing words after the last CTL");
    for (uint64_t t = 0; t < T; t++)
        if (progs[t]->logup_polys() + 4 * eps_of[t] > STARKHIP_AIR_MAX_LOGUP_POLYS)
            return refuse(why, "table " + std::to_string(t) + ": " + std::to_string(progs[t]->logup_polys()) + " LogUp and " + std::to_string(4 * eps_of[t]) +
                                   " CTL polynomials, nA + nC above " + std::to_string(STARKHIP_AIR_MAX_LOGUP_POLYS));
    if (out) *out = std::move(S);
    return true;
}

bool air_parse_checked(const uint64_t* blob, size_t words, AirProgram* out, std::string* why) {
    if (!blob || words < 8) return refuse(why, "blob shorter than its 8-word header");
    if (blob[0] != AIR_MAGIC) return refuse(why, "bad magic (not a SAIR_IR1 program)");
    const uint64_t n_cols = blob[1], n_pis = blob[2], degree = blob[3], n_constraints = blob[4], n_consts = blob[5], n_code = blob[6],
                   n_groups = blob[7];
    if (n_cols < 1 || n_cols > STARKHIP_AIR_MAX_COLUMNS) return refuse(why, "n_cols " + std::to_string(n_cols) + " outside 1.." + std::to_string(STARKHIP_AIR_MAX_COLUMNS));
    if (n_pis > STARKHIP_AIR_MAX_PUBLIC_INPUTS) return refuse(why, "n_pis " + std::to_string(n_pis) + " above " + std::to_string(STARKHIP_AIR_MAX_PUBLIC_INPUTS));
    if (degree < 1 || degree > STARKHIP_AIR_MAX_DEGREE) return refuse(why, "degree " + std::to_string(degree) + " outside 1.." + std::to_string(STARKHIP_AIR_MAX_DEGREE));
    if (n_code < 2 || n_code > STARKHIP_AIR_MAX_CODE_WORDS) return refuse(why, "code size " + std::to_string(n_code) + " outside 2.." + std::to_string(STARKHIP_AIR_MAX_CODE_WORDS));
    if (n_consts > n_code) return refuse(why, "more constants than code words");
    if (n_constraints < 1 || n_constraints > n_code) return refuse(why, "n_constraints " + std::to_string(n_constraints) + " not in 1..code size");
    if (n_groups < 1 || n_groups > n_code) return refuse(why, "n_groups " + std::to_string(n_groups) + " not in 1..code size");
    const uint64_t code_u64 = (n_code + 1) / 2;
    const uint64_t base_words = 8 + n_consts + code_u64 + n_groups;  // every count is below 2^27 here: no overflow
    // what follows the group table is the section of permutation pairs or of LogUp lookups, or nothing (a word that is neither section's magic is a wrong length)
    if ((uint64_t)words < base_words || ((uint64_t)words > base_words && blob[base_words] != AIR_PERM_MAGIC && blob[base_words] != AIR_LOGUP_MAGIC && blob[base_words] != AIR_LOGUP2_MAGIC))
        return refuse(why, "blob length " + std::to_string(words) + " differs from the " + std::to_string(base_words) + " words its header implies");
    const uint64_t* consts = blob + 8;
    const uint64_t* code64 = consts + n_consts;
    const uint64_t* groups = code64 + code_u64;
    for (uint64_t i = 0; i < n_consts; i++)
        if (consts[i] >= GL_P) return refuse(why, "constant " + std::to_string(i) + " is not canonical");
    if ((n_code & 1) && (code64[code_u64 - 1] >> 32) != 0) return refuse(why, "nonzero padding after the last code word");

    AirProgram P;
    P.n_cols = (uint32_t)n_cols;
    P.n_pis = (uint32_t)n_pis;
    P.degree = (uint32_t)degree;
    P.n_constraints = (uint32_t)n_constraints;
    P.consts.assign(consts, consts + n_consts);
    P.code.resize(n_code);
    for (uint64_t i = 0; i < n_code; i++) P.code[i] = (uint32_t)(code64[i / 2] >> (32 * (i & 1)));
    P.group_off.resize(n_groups);
    P.group_k0.resize(n_groups);
    for (uint64_t g = 0; g < n_groups; g++) {
        P.group_off[g] = (uint32_t)groups[g];
        P.group_k0[g] = (uint32_t)(groups[g] >> 32);
    }

    auto cellref_ok = [&](uint32_t ref, bool gate, std::string* msg) {
        if (ref & ~(REF_COL_MASK | REF_NEXT | REF_COMPL)) return *msg = "cell reference with unknown flag bits", false;
        if (!gate && (ref & REF_COMPL)) return *msg = "REF_COMPL on a term factor (gates only)", false;
        if ((ref & REF_COL_MASK) >= n_cols) return *msg = "column " + std::to_string(ref & REF_COL_MASK) + " out of range", false;
        return true;
    };
    const std::vector<uint32_t>& code = P.code;
    size_t i = 0;
    uint64_t k = 0, g = 0;
    std::string msg;
    for (;;) {
        if (i >= n_code) return refuse(why, "code ends without its END word");
        const uint32_t gw = code[i];
        if (gw == 0) {
            if (i + 1 != n_code) return refuse(why, "trailing words after END");
            break;
        }
        const std::string at = "group " + std::to_string(g) + " (code word " + std::to_string(i) + "): ";
        const GroupWord grp = GroupWord::decode(gw);
        if (grp.encode() != gw) return refuse(why, at + "not a GROUP word");  // another tag, or a reserved bit
        const uint32_t kind = grp.kind, ng = grp.n_gates, m = grp.m;
        if (m < 1 || m > AIR_MAX_GROUP) return refuse(why, at + "m = " + std::to_string(m) + " outside 1.." + std::to_string(AIR_MAX_GROUP));
        if (ng > 4) return refuse(why, at + std::to_string(ng) + " gates (at most 4)");
        if (g >= n_groups) return refuse(why, at + "more groups than the group table holds");
        if (P.group_off[g] != i || P.group_k0[g] != k) return refuse(why, at + "group table entry differs from the code");
        g++;
        i++;
        if (n_code - i < ng) return refuse(why, at + "gates run past the code");
        for (uint32_t j = 0; j < ng; j++, i++)
            if (!cellref_ok(code[i], true, &msg)) return refuse(why, at + "gate: " + msg);
        for (uint32_t c = 0; c < m; c++, k++) {
            const std::string atk = "constraint " + std::to_string(k) + ": ";
            uint32_t maxf = 0;
            for (;;) {
                if (i >= n_code) return refuse(why, atk + "terms run past the code");
                const TermWord tw = TermWord::decode(code[i++]);
                const uint32_t nf = tw.nf, ck = tw.ck, idx = tw.idx;
                if (ck > CK_NEG_PI) return refuse(why, atk + "coefficient kind " + std::to_string(ck) + " (at most 4)");
                if (ck == CK_CONST && idx >= n_consts) return refuse(why, atk + "const index " + std::to_string(idx) + " out of range");
                if ((ck == CK_PI || ck == CK_NEG_PI) && idx >= n_pis) return refuse(why, atk + "public input index " + std::to_string(idx) + " out of range");
                if ((ck == CK_PLUS || ck == CK_MINUS) && idx != 0) return refuse(why, atk + "index on a +-1 term");
                if (n_code - i < nf) return refuse(why, atk + "factors run past the code");
                for (uint32_t f = 0; f < nf; f++, i++)
                    if (!cellref_ok(code[i], false, &msg)) return refuse(why, atk + msg);
                maxf = std::max(maxf, nf);
                if (tw.last) break;
            }
            const uint32_t deg = ng + maxf + ((kind == KIND_FIRST || kind == KIND_LAST) ? 1u : 0u);
            if (deg > degree) return refuse(why, atk + "degree " + std::to_string(deg) + " above the declared " + std::to_string(degree));
        }
    }
    if (g != n_groups) return refuse(why, "group table has " + std::to_string(n_groups) + " entries, the code " + std::to_string(g) + " groups");
    if (k != n_constraints) return refuse(why, "n_constraints " + std::to_string(n_constraints) + " but the code has " + std::to_string(k));

    // ---- permutation pairs: every column a kernel will read is < n_cols, every count within what the proof header and the kernels carry
    if ((uint64_t)words > base_words && blob[base_words] == AIR_PERM_MAGIC) {
        const uint64_t* sec = blob + base_words;
        const uint64_t sec_words = (uint64_t)words - base_words;
        if (sec_words < 2) return refuse(why, "permutation section shorter than its 2-word header");
        const uint64_t n_pairs = sec[1];
        if (n_pairs < 1 || n_pairs > STARKHIP_AIR_MAX_PERMUTATION_PAIRS)
            return refuse(why, "permutation section with " + std::to_string(n_pairs) + " pairs (1.." + std::to_string(STARKHIP_AIR_MAX_PERMUTATION_PAIRS) + ")");
        if (degree < 2) return refuse(why, "permutation pairs need degree >= 2 (a Z constraint has degree 1 + the pairs of its batch)");
        const uint64_t B = degree - 1, n_batches = (n_pairs + B - 1) / B;
        if (n_batches > B)  // upstream draws B challenge sets and zips the batches with them: the batches beyond B would go unchecked
            return refuse(why, std::to_string(n_pairs) + " permutation pairs make " + std::to_string(n_batches) + " batches, more than the " + std::to_string(B) + " challenge sets of degree " + std::to_string(degree));
        uint64_t at = 2;
        for (uint64_t p = 0; p < n_pairs; p++) {
            const std::string atp = "permutation pair " + std::to_string(p) + ": ";
            if (at >= sec_words) return refuse(why, atp + "runs past the blob");
            const uint64_t ne = sec[at++];
            if (ne < 1) return refuse(why, atp + "empty pair");
            if (ne > STARKHIP_AIR_MAX_PERMUTATION_ENTRIES) return refuse(why, atp + std::to_string(ne) + " entries (at most " + std::to_string(STARKHIP_AIR_MAX_PERMUTATION_ENTRIES) + ")");
            if (sec_words - at < ne) return refuse(why, atp + "entries run past the blob");
            for (uint64_t e = 0; e < ne; e++) {
                const uint64_t lhs = sec[at + e] & 0xFFFFFFFFu, rhs = sec[at + e] >> 32;
                if (lhs >= n_cols || rhs >= n_cols) return refuse(why, atp + "column " + std::to_string(lhs >= n_cols ? lhs : rhs) + " out of range");
            }
            P.perm_pairs.emplace_back(sec + at, sec + at + ne);
            at += ne;
        }
        if (at < sec_words && (sec[at] == AIR_LOGUP_MAGIC || sec[at] == AIR_LOGUP2_MAGIC))
            return refuse(why, "permutation pairs and LogUp lookups together (the two share the middle matrix of a proof)");
        if (at != sec_words) return refuse(why, "trailing words after the permutation section");
    }
    // ---- LogUp lookups: the same for the other section
    if ((uint64_t)words > base_words && blob[base_words] == AIR_LOGUP_MAGIC) {
        const uint64_t* sec = blob + base_words;
        const uint64_t sec_words = (uint64_t)words - base_words;
        if (sec_words < 2) return refuse(why, "LogUp section shorter than its 2-word header");
        const uint64_t n_lookups = sec[1];
        if (n_lookups < 1 || n_lookups > STARKHIP_AIR_MAX_LOGUP_LOOKUPS)
            return refuse(why, "LogUp section with " + std::to_string(n_lookups) + " lookups (1.." + std::to_string(STARKHIP_AIR_MAX_LOGUP_LOOKUPS) + ")");
        if (degree < 2) return refuse(why, "LogUp lookups need degree >= 2 (a helper constraint has degree 1 + the columns of its batch)");
        uint64_t at = 2;
        for (uint64_t l = 0; l < n_lookups; l++) {
            const std::string atl = "LogUp lookup " + std::to_string(l) + ": ";
            if (sec_words - at < 2) return refuse(why, atl + "runs past the blob");
            const uint64_t m = sec[at], table = sec[at + 1] & 0xFFFFFFFFu, freq = sec[at + 1] >> 32;
            at += 2;
            if (m < 1) return refuse(why, atl + "empty lookup");
            if (m > STARKHIP_AIR_MAX_LOGUP_COLUMNS) return refuse(why, atl + std::to_string(m) + " columns (at most " + std::to_string(STARKHIP_AIR_MAX_LOGUP_COLUMNS) + ")");
            if (table >= n_cols || freq >= n_cols) return refuse(why, atl + "column " + std::to_string(table >= n_cols ? table : freq) + " out of range");
            if (sec_words - at < m) return refuse(why, atl + "columns run past the blob");
            AirProgram::Logup lk;
            lk.table = AirProgram::Column((uint32_t)table);
            lk.freq = AirProgram::Column((uint32_t)freq);
            for (uint64_t e = 0; e < m; e++) {
                if (sec[at + e] >= n_cols) return refuse(why, atl + "column " + std::to_string(sec[at + e]) + " out of range");
                lk.cols.push_back(AirProgram::Column((uint32_t)sec[at + e]));
            }
            lk.filters.resize(m);
            P.logups.push_back(std::move(lk));
            at += m;
        }
        if (at < sec_words && sec[at] == AIR_PERM_MAGIC)
            return refuse(why, "permutation pairs and LogUp lookups together (the two share the middle matrix of a proof)");
        if (at < sec_words && sec[at] == AIR_LOGUP2_MAGIC) return refuse(why, "LogUp sections of both versions together (declare every lookup in the general one)");
        if (at != sec_words) return refuse(why, "trailing words after the LogUp section");
        if (P.logup_polys() > STARKHIP_AIR_MAX_LOGUP_POLYS)
            return refuse(why, "LogUp lookups make " + std::to_string(P.logup_polys()) + " auxiliary polynomials (at most " + std::to_string(STARKHIP_AIR_MAX_LOGUP_POLYS) + ")");
    }
    // ---- LogUp lookups over Columns and Filters: the general section, by the same rules
    if ((uint64_t)words > base_words && blob[base_words] == AIR_LOGUP2_MAGIC) {
        const uint64_t* sec = blob + base_words;
        const uint64_t sec_words = (uint64_t)words - base_words;
        if (sec_words < 2) return refuse(why, "LogUp section shorter than its 2-word header");
        const uint64_t n_lookups = sec[1];
        if (n_lookups < 1 || n_lookups > STARKHIP_AIR_MAX_LOGUP_LOOKUPS)
            return refuse(why, "LogUp section with " + std::to_string(n_lookups) + " lookups (1.." + std::to_string(STARKHIP_AIR_MAX_LOGUP_LOOKUPS) + ")");
        if (degree < 2) return refuse(why, "LogUp lookups need degree >= 2 (a helper constraint has degree 1 + the columns of its batch)");
        uint64_t at = 2;
        std::string msg2;
        auto column = [&](AirProgram::Column* c) { return read_column(sec, sec_words, &at, n_cols, c, &msg2); };  // one COLUMN at sec[at]
        for (uint64_t l = 0; l < n_lookups; l++) {
            const std::string atl = "LogUp lookup " + std::to_string(l) + ": ";
            if (at >= sec_words) return refuse(why, atl + "runs past the blob");
            const uint64_t m = sec[at++];
            if (m < 1) return refuse(why, atl + "empty lookup");
            if (m > STARKHIP_AIR_MAX_LOGUP_COLUMNS) return refuse(why, atl + std::to_string(m) + " columns (at most " + std::to_string(STARKHIP_AIR_MAX_LOGUP_COLUMNS) + ")");
            AirProgram::Logup lk;
            if (!column(&lk.table)) return refuse(why, atl + "table: " + msg2);
            if (!column(&lk.freq)) return refuse(why, atl + "frequencies: " + msg2);
            for (uint64_t e = 0; e < m; e++) {
                const std::string ate = atl + "column " + std::to_string(e) + ": ";
                AirProgram::Column v;
                if (!column(&v)) return refuse(why, ate + msg2);
                if (at >= sec_words) return refuse(why, ate + "filter runs past the blob");
                const uint64_t np = sec[at] & 0xFFFFFFFFu, ns = sec[at] >> 32;
                at++;
                if (np > AIR_LOGUP_MAX_FILTER_PRODUCTS) return refuse(why, ate + "filter of " + std::to_string(np) + " products (at most " + std::to_string(AIR_LOGUP_MAX_FILTER_PRODUCTS) + ")");
                if (ns > AIR_LOGUP_MAX_FILTER_SUMS) return refuse(why, ate + "filter of " + std::to_string(ns) + " sums (at most " + std::to_string(AIR_LOGUP_MAX_FILTER_SUMS) + ")");
                AirProgram::Filter f;
                f.n_products = (uint32_t)np;
                for (uint64_t k = 0; k < 2 * np + ns; k++) {
                    AirProgram::Column fc;
                    if (!column(&fc)) return refuse(why, ate + "filter: " + msg2);
                    f.cols.push_back(std::move(fc));
                }
                lk.cols.push_back(std::move(v));
                lk.filters.push_back(std::move(f));
            }
            P.logups.push_back(std::move(lk));
        }
        P.logup_section2 = true;
        if (at < sec_words && sec[at] == AIR_PERM_MAGIC)
            return refuse(why, "permutation pairs and LogUp lookups together (the two share the middle matrix of a proof)");
        if (at < sec_words && sec[at] == AIR_LOGUP_MAGIC) return refuse(why, "LogUp sections of both versions together (declare every lookup in the general one)");
        if (at != sec_words) return refuse(why, "trailing words after the LogUp section");
        if (P.logup_polys() > STARKHIP_AIR_MAX_LOGUP_POLYS)
            return refuse(why, "LogUp lookups make " + std::to_string(P.logup_polys()) + " auxiliary polynomials (at most " + std::to_string(STARKHIP_AIR_MAX_LOGUP_POLYS) + ")");
    }
    if (out) *out = std::move(P);
    return true;
}

gl_t air_constraint_value_at(const AirProgram& P, uint32_t group_word, uint32_t term_word, const gl_t* local, const gl_t* next, const gl_t* pis) {
    gl_t G, body;
    air_constraint_parts_at(P, group_word, term_word, local, next, pis, &G, &body);
    return gl_mul(G, body);
}

void air_constraint_parts_at(const AirProgram& P, uint32_t group_word, uint32_t term_word, const gl_t* local, const gl_t* next, const gl_t* pis,
                             gl_t* G_out, gl_t* body_out) {
    auto cell = [&](uint32_t ref) { return gl_from_u64(((ref & REF_NEXT) ? next : local)[ref & REF_COL_MASK]); };  // any word of the class mod p
    AirReader rd(P, group_word);
    GroupWord grp;
    rd.group(&grp);
    gl_t G = 1;
    for (uint32_t j = 0; j < grp.n_gates; j++) {
        const uint32_t ref = rd.ref();
        G = gl_mul(G, (ref & REF_COMPL) ? gl_sub(1, cell(ref)) : cell(ref));
    }
    rd = AirReader(P, term_word);
    gl_t body = 0;
    for (;;) {
        const TermWord tw = rd.term();
        gl_t u = 1;
        for (uint32_t f = 0; f < tw.nf; f++) u = gl_mul(u, cell(rd.ref()));
        if (tw.ck == CK_PLUS) body = gl_add(body, u);
        else if (tw.ck == CK_MINUS) body = gl_sub(body, u);
        else if (tw.ck == CK_CONST) body = gl_add(body, gl_mul(u, P.consts[tw.idx]));
        else if (tw.ck == CK_PI) body = gl_add(body, gl_mul(u, pis[tw.idx]));
        else body = gl_sub(body, gl_mul(u, pis[tw.idx]));
        if (tw.last) break;
    }
    *G_out = G;
    *body_out = body;
}

gl_t air_constraint_value(const AirProgram& P, uint32_t k, const gl_t* local, const gl_t* next, const gl_t* pis) {
    // the group of constraint k: the last one whose first constraint is <= k
    const size_t g = (size_t)(std::upper_bound(P.group_k0.begin(), P.group_k0.end(), k) - P.group_k0.begin()) - 1;
    AirReader rd(P, P.group_off[g]);
    GroupWord grp;
    rd.group(&grp);
    for (uint32_t j = 0; j < grp.n_gates; j++) rd.ref();
    for (uint32_t c = P.group_k0[g]; c < k; c++) {  // the constraints of the group ahead of k
        TermWord tw;
        do {
            tw = rd.term();
            for (uint32_t f = 0; f < tw.nf; f++) rd.ref();
        } while (!tw.last);
    }
    return air_constraint_value_at(P, P.group_off[g], (uint32_t)(rd.w - P.code.data()), local, next, pis);
}

}  // namespace starkhip
