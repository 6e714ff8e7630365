// Flat constraint program ("AIR IR") + the symbolic builder that produces it.
//
// The reference evaluates an AIR by calling S::eval_packed_generic once per LDE
// point (e.g. /root/reference/src/fp12_mul.rs:58-99) with a ConstraintConsumer that
// folds constraint k into acc = acc*alpha + c_k.  A GPU cannot
// call Rust generics, so here each AIR is *described once* as data: the gadget
// functions (air_fp*.cpp) run the same control flow as the reference's
// add_*_constraints functions but on symbolic expressions, and every
// yield_constr.constraint*/ call becomes one record of this program, in the same
// order (the order fixes the power of alpha each constraint gets).
//
// Every constraint of the four AIRs has the shape  mask(kind) * gate_1..gate_g * body
//  where gate_i is a trace cell c or (1 - c) and body is a short
// sum of  coef * cell * cell...  terms.  Consecutive constraints with identical
// (kind, gates) form a GROUP so an evaluator can Horner-fold the bodies and multiply
// by the gate product once:
//     acc_j <- acc_j * alpha_j^m + mask * G * (sum_k body_k alpha_j^(m-1-k))
// which equals the reference's per-constraint fold exactly (field arithmetic is exact).
//
// Code stream (uint32 words):
//   GROUP word : [3:0]=1  [5:4]=kind  [15:8]=n_gates  [31:16]=m (1..AIR_MAX_GROUP)
//   n_gates x cellref
//   m constraints, each = 1+ TERM records; TERM word:
//       [1:0]=nf (cell factors)  [4:2]=ck  [5]=last term of this constraint  [31:6]=idx
//     ck: 0 => +1, 1 => -1, 2 => consts[idx], 3 => +public_inputs[idx], 4 => -public_inputs[idx]
//     followed by nf x cellref
//   END word   : 0
// cellref: [23:0]=column  [30]=next row  [31]=complement (gates only: value 1 - cell)
//
// Permutation pairs (starky's Stark::permutation_pairs(), COMPAT.md P1-P8): an OPTIONAL section of the blob after the group table,
//   AIR_PERM_MAGIC, n_pairs, then per pair: n_entries, n_entries words  lhs column | rhs column << 32.
// A program without pairs has no section and keeps its bytes.  The pairs are cut into batches of B = max(1, degree - 1) in
// declaration order; a batch has one Z polynomial per challenge (2), index batch * 2 + challenge.
//
// LogUp lookups (starky >= 0.2's Lookup { columns, table_column, frequencies_column }, COMPAT.md L1-L7): the OTHER optional section, in
// the same place -- a program has pairs or LogUp lookups, not both --
//   AIR_LOGUP_MAGIC, n_lookups, then per lookup: n_columns, table column | frequencies column << 32, n_columns column words.
// A lookup's columns are cut in declaration order into helper batches of degree - 1 (logup.h has the polynomials' order).
// The general form of the same section (upstream's Column and Filter, COMPAT.md 2c), never beside the first:
//   AIR_LOGUP2_MAGIC, n_lookups, then per lookup: n_columns, COLUMN table, COLUMN frequencies, n_columns x { COLUMN value, FILTER }
//   COLUMN := n_local | n_next << 32, constant, then (n_local + n_next) x { trace column, coefficient }   (local terms first)
//   FILTER := n_products | n_sums << 32, then 2 n_products + n_sums COLUMNs (each product's A then B, then the sums)
// A COLUMN is constant + sum coefficient * cell over the local and the next row; a FILTER is sum A B + sum C, and 1 when it is empty.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "gl.h"

namespace starkhip {

enum : uint32_t { KIND_PLAIN = 0, KIND_TRANSITION = 1, KIND_FIRST = 2, KIND_LAST = 3 };
enum : uint32_t { CK_PLUS = 0, CK_MINUS = 1, CK_CONST = 2, CK_PI = 3, CK_NEG_PI = 4 };
enum : uint32_t { REF_NEXT = 1u << 30, REF_COMPL = 1u << 31, REF_COL_MASK = 0xFFFFFFu };
static const uint32_t AIR_MAX_GROUP = 255;
static const uint64_t AIR_MAGIC = 0x3152495F52494153ULL;  // "SAIR_IR1"
static const uint64_t AIR_PERM_MAGIC = 0x3153524941504D50ULL;  // "PMPAIRS1": the section of permutation pairs
static const uint64_t AIR_LOGUP_MAGIC = 0x3130535055474F4CULL;  // "LOGUPS01": the section of LogUp lookups
static const uint64_t AIR_LOGUP2_MAGIC = 0x3230535055474F4CULL;  // "LOGUPS02": the same over Columns and Filters
static const uint32_t AIR_LOGUP_MAX_TERMS = 16, AIR_LOGUP_MAX_FILTER_PRODUCTS = 4, AIR_LOGUP_MAX_FILTER_SUMS = 4;

// The rows a constraint of `kind` applies to, of a trace of n rows: the one rule of the device checkers' walker
// (kernels_check.hip) and of the host replay (check_report.cpp).  Written without short-circuit operators: in the walker's loop
// `kind` changes and the row does not, and this way the row's two comparisons leave the loop and no branch on `kind` is left in it.
template <class I>
GL_HD bool constraint_applies(uint32_t kind, I row, I n) {
    const bool is_first = row == 0, is_last = row == n - 1;
    return (kind == KIND_PLAIN) | ((kind == KIND_TRANSITION) & !is_last) | ((kind == KIND_FIRST) & is_first) | ((kind == KIND_LAST) & is_last);
}

// The two code words above, decoded: the only place that knows their bit layout.
struct GroupWord {
    uint32_t kind, n_gates, m;
    static GroupWord decode(uint32_t w) { return {(w >> 4) & 3u, (w >> 8) & 255u, w >> 16}; }
    uint32_t encode() const { return 1u | (kind << 4) | (n_gates << 8) | (m << 16); }
    static bool is_group(uint32_t w) { return (w & 15u) == 1u; }  // the tag alone: END (0) is not one
};
struct TermWord {
    uint32_t nf, ck, idx;
    bool last;
    static TermWord decode(uint32_t w) { return {w & 3u, (w >> 2) & 7u, w >> 6, (w & 32u) != 0}; }
    uint32_t encode() const { return nf | (ck << 2) | (last ? 32u : 0u) | (idx << 6); }
};

struct AirProgram {
    uint32_t n_cols = 0, n_pis = 0, degree = 0, n_constraints = 0;
    std::vector<uint64_t> consts;
    std::vector<uint32_t> code;
    // per group: word offset of the GROUP word, and number of constraints before it
    std::vector<uint32_t> group_off, group_k0;
    // permutation pairs: per pair its entries, lhs column | rhs column << 32 (empty for every built-in AIR)
    std::vector<std::vector<uint64_t>> perm_pairs;
    uint32_t perm_batch_size() const { return degree > 1 ? degree - 1 : 1; }  // B: quotient_degree_factor, and permutation_batch_size()
    uint32_t perm_batches() const { return (uint32_t)((perm_pairs.size() + perm_batch_size() - 1) / perm_batch_size()); }
    uint32_t perm_zs() const { return 2 * perm_batches(); }  // nZ: one Z per (batch, challenge)
    // LogUp lookups (empty for every built-in AIR).  A Column is constant + sum coef * cell, the first n_local terms on the local row and
    // the others on the next; a Filter is sum A B + sum C over Columns (`cols`: each product's A then B, then the sums), 1 when empty.
    struct Column {
        struct Term { uint32_t col; gl_t coef; };
        uint32_t n_local = 0;
        gl_t constant = 0;
        std::vector<Term> terms;
        Column() {}
        Column(uint32_t col) : n_local(1), terms{{col, 1}} {}  // a plain column: one local cell, coefficient 1, constant 0
        bool plain() const { return n_local == 1 && terms.size() == 1 && terms[0].coef == 1 && constant == 0; }
        uint32_t col() const { return terms.empty() ? ~0u : terms[0].col; }  // of a plain one
        operator uint32_t() const { return col(); }                             // (code that knows plain lookups alone reads a column number)
        bool operator==(const Column& o) const {
            if (n_local != o.n_local || constant != o.constant || terms.size() != o.terms.size()) return false;
            for (size_t k = 0; k < terms.size(); k++)
                if (terms[k].col != o.terms[k].col || terms[k].coef != o.terms[k].coef) return false;
            return true;
        }
        void push(std::vector<uint64_t>& b) const {
            b.push_back((uint64_t)n_local | ((uint64_t)(terms.size() - n_local) << 32));
            b.push_back(constant);
            for (const Term& t : terms) { b.push_back(t.col); b.push_back(t.coef); }
        }
        template <class F> void each_column(const F& f) const { for (const Term& t : terms) f(t.col); }
    };
    struct Filter {
        uint32_t n_products = 0;
        std::vector<Column> cols;
        bool empty() const { return cols.empty(); }
        void push(std::vector<uint64_t>& b) const {
            b.push_back((uint64_t)n_products | ((uint64_t)(cols.size() - 2 * n_products) << 32));
            for (const Column& c : cols) c.push(b);
        }
    };
    // `cols` under `filters` (one each) looked up in `table` with the multiplicities in `freq`
    struct Logup {
        std::vector<Column> cols;
        std::vector<Filter> filters;
        Column table, freq;
        bool plain() const {
            for (const Column& v : cols) if (!v.plain()) return false;
            for (const Filter& f : filters) if (!f.empty()) return false;
            return table.plain() && freq.plain();
        }
        template <class F> void each_column(const F& f) const {  // every trace column the lookup reads
            table.each_column(f);
            freq.each_column(f);
            for (const Column& v : cols) v.each_column(f);
            for (const Filter& fl : filters) for (const Column& c : fl.cols) c.each_column(f);
        }
    };
    bool logup_section2 = false;  // the lookups came from (and go back into) the general section
    bool logup_general() const {  // some lookup is not plain: the general kernels run
        for (const Logup& l : logups) if (!l.plain()) return true;
        return false;
    }
    std::vector<Logup> logups;
    uint32_t logup_batch_size() const { return degree > 1 ? degree - 1 : 1; }
    uint32_t logup_helpers(size_t l) const { return (uint32_t)((logups[l].cols.size() + logup_batch_size() - 1) / logup_batch_size()); }  // H_l
    uint32_t logup_polys() const {  // nA = 2 sum (H_l + 1): per challenge and lookup the helpers, then Z
        uint32_t a = 0;
        for (size_t l = 0; l < logups.size(); l++) a += logup_helpers(l) + 1;
        return 2 * a;
    }
    uint32_t logup_constraints() const { return logup_polys() + 2 * (uint32_t)logups.size(); }  // nL = 2 sum (H_l + 2)

    // blob layout (u64 words): magic, n_cols, n_pis, degree, n_constraints, n_consts,
    // n_code_words, n_groups, consts[], code[] (two u32 per u64, zero padded),
    // group_off[] / group_k0[] packed as (off | k0<<32), then the section of permutation pairs or of LogUp lookups if there are any
    std::vector<uint64_t> serialize() const {
        std::vector<uint64_t> b;
        b.push_back(AIR_MAGIC);
        b.push_back(n_cols);
        b.push_back(n_pis);
        b.push_back(degree);
        b.push_back(n_constraints);
        b.push_back(consts.size());
        b.push_back(code.size());
        b.push_back(group_off.size());
        b.insert(b.end(), consts.begin(), consts.end());
        for (size_t i = 0; i < code.size(); i += 2) {
            uint64_t w = code[i];
            if (i + 1 < code.size()) w |= (uint64_t)code[i + 1] << 32;
            b.push_back(w);
        }
        for (size_t i = 0; i < group_off.size(); i++)
            b.push_back((uint64_t)group_off[i] | ((uint64_t)group_k0[i] << 32));
        if (!perm_pairs.empty()) {
            b.push_back(AIR_PERM_MAGIC);
            b.push_back(perm_pairs.size());
            for (const auto& pr : perm_pairs) {
                b.push_back(pr.size());
                b.insert(b.end(), pr.begin(), pr.end());
            }
        }
        if (!logups.empty() && !logup_section2) {  // (a program of the first section has plain lookups only)
            b.push_back(AIR_LOGUP_MAGIC);
            b.push_back(logups.size());
            for (const Logup& l : logups) {
                b.push_back(l.cols.size());
                b.push_back((uint64_t)l.table.col() | ((uint64_t)l.freq.col() << 32));
                for (const Column& v : l.cols) b.push_back(v.col());
            }
        }
        if (!logups.empty() && logup_section2) {
            b.push_back(AIR_LOGUP2_MAGIC);
            b.push_back(logups.size());
            for (const Logup& l : logups) {
                b.push_back(l.cols.size());
                l.table.push(b);
                l.freq.push(b);
                for (size_t k = 0; k < l.cols.size(); k++) {
                    l.cols[k].push(b);
                    l.filters[k].push(b);
                }
            }
        }
        return b;
    }
};

// Forward cursor over the code of a VALIDATED program (the builder's, or one air_parse_checked accepted): nothing is checked
// here.  The caller reads in the stream's own order: group(), its n_gates x ref(), then per constraint term() and its nf x ref()
// until a term is `last`, m constraints in all, then group() again.
struct AirReader {
    const uint32_t* w;
    explicit AirReader(const AirProgram& p, size_t word = 0) {
        static const uint32_t END = 0;  // a default-constructed program has no code at all
        w = p.code.empty() ? &END : p.code.data() + word;
    }
    bool group(GroupWord* g) {  // false at END
        if (!GroupWord::is_group(*w)) return false;
        *g = GroupWord::decode(*w++);
        return true;
    }
    TermWord term() { return TermWord::decode(*w++); }
    uint32_t ref() { return *w++; }  // the next cellref: a gate of the group, or a factor of the term, just read
};

// ------------------------------------------------------------------ symbolic layer
struct Mono {
    gl_t coef;                  // canonical, non-zero
    int pi;                     // -1 or public-input index (coefficient multiplies PI[pi])
    std::vector<uint32_t> f;    // sorted cell refs (col | REF_NEXT)
    bool same_vars(const Mono& o) const { return pi == o.pi && f == o.f; }
};

struct Poly {
    std::vector<Mono> m;
    void add_mono(const Mono& x) {
        if (x.coef == 0) return;
        for (size_t i = 0; i < m.size(); i++)
            if (m[i].same_vars(x)) {
                m[i].coef = gl_add(m[i].coef, x.coef);
                if (m[i].coef == 0) m.erase(m.begin() + i);
                return;
            }
        m.push_back(x);
    }
    bool is_const(gl_t c) const { return m.size() == 1 && m[0].pi < 0 && m[0].f.empty() && m[0].coef == c; }
    bool is_single_cell() const { return m.size() == 1 && m[0].pi < 0 && m[0].f.size() == 1 && m[0].coef == 1; }
    // 1 - cell ?
    bool is_complement(uint32_t* cell) const {
        if (m.size() != 2) return false;
        const Mono *one = nullptr, *neg = nullptr;
        for (auto& x : m) {
            if (x.pi < 0 && x.f.empty() && x.coef == 1) one = &x;
            if (x.pi < 0 && x.f.size() == 1 && x.coef == GL_P - 1) neg = &x;
        }
        if (!one || !neg) return false;
        *cell = neg->f[0];
        return true;
    }
};

inline Poly poly_mul(const Poly& a, const Poly& b) {
    Poly r;
    for (auto& x : a.m)
        for (auto& y : b.m) {
            Mono z;
            z.coef = gl_mul(x.coef, y.coef);
            if (x.pi >= 0 && y.pi >= 0) throw std::runtime_error("air_ir: product of two public inputs");
            z.pi = x.pi >= 0 ? x.pi : y.pi;
            z.f = x.f;
            z.f.insert(z.f.end(), y.f.begin(), y.f.end());
            std::sort(z.f.begin(), z.f.end());
            r.add_mono(z);
        }
    return r;
}

// value = prod(gates) * body
struct Expr {
    std::vector<uint32_t> gates;  // cellref, may carry REF_COMPL
    Poly body;

    Expr() {}
    static Expr constant(gl_t c) {
        Expr e;
        Mono m;
        m.coef = gl_from_u64(c);
        m.pi = -1;
        e.body.add_mono(m);
        return e;
    }
    static Expr cell(uint32_t ref) {
        Expr e;
        Mono m;
        m.coef = 1;
        m.pi = -1;
        m.f.push_back(ref);
        e.body.m.push_back(m);
        return e;
    }
    static Expr pub(int i) {
        Expr e;
        Mono m;
        m.coef = 1;
        m.pi = i;
        e.body.m.push_back(m);
        return e;
    }
    // fold gates into the body (expanded polynomial)
    Poly expanded() const {
        Poly p = body;
        for (uint32_t g : gates) {
            Poly q;
            Mono c;
            c.coef = 1;
            c.pi = -1;
            c.f.push_back(g & ~REF_COMPL);
            if (g & REF_COMPL) {
                Mono one;
                one.coef = 1;
                one.pi = -1;
                q.m.push_back(one);
                c.coef = GL_P - 1;
            }
            q.m.push_back(c);
            p = poly_mul(p, q);
        }
        return p;
    }
};

inline Expr operator+(const Expr& a, const Expr& b) {
    Expr r;
    r.body = a.expanded();
    Poly pb = b.expanded();
    for (auto& x : pb.m) r.body.add_mono(x);
    return r;
}
inline Expr operator-(const Expr& a, const Expr& b) {
    Expr r;
    r.body = a.expanded();
    Poly pb = b.expanded();
    for (auto x : pb.m) {
        x.coef = gl_neg(x.coef);
        r.body.add_mono(x);
    }
    return r;
}
inline Expr operator*(const Expr& a, const Expr& b) {
    Expr r;
    r.gates = a.gates;
    r.gates.insert(r.gates.end(), b.gates.begin(), b.gates.end());
    uint32_t c;
    if (a.body.is_const(1)) {
        r.body = b.body;
    } else if (b.body.is_const(1)) {
        r.body = a.body;
    } else if (a.body.is_single_cell()) {
        r.gates.push_back(a.body.m[0].f[0]);
        r.body = b.body;
    } else if (b.body.is_single_cell()) {
        r.gates.push_back(b.body.m[0].f[0]);
        r.body = a.body;
    } else if (a.body.is_complement(&c)) {
        r.gates.push_back(c | REF_COMPL);
        r.body = b.body;
    } else if (b.body.is_complement(&c)) {
        r.gates.push_back(c | REF_COMPL);
        r.body = a.body;
    } else {
        r.body = poly_mul(a.body, b.body);
    }
    return r;
}
inline Expr operator*(const Expr& a, uint64_t k) { return a * Expr::constant(k); }
inline Expr operator-(const Expr& a, uint64_t k) { return a - Expr::constant(k); }
inline Expr operator+(const Expr& a, uint64_t k) { return a + Expr::constant(k); }

// ------------------------------------------------------------------ builder
class AirBuilder {
  public:
    AirBuilder(uint32_t n_cols, uint32_t n_pis, uint32_t degree) {
        prog_.n_cols = n_cols;
        prog_.n_pis = n_pis;
        prog_.degree = degree;
    }

    Expr L(uint32_t col) const { check_col(col); return Expr::cell(col); }
    Expr N(uint32_t col) const { check_col(col); return Expr::cell(col | REF_NEXT); }
    Expr PI(uint32_t i) const {
        if (i >= prog_.n_pis) throw std::runtime_error("air_ir: public input index out of range");
        return Expr::pub((int)i);
    }
    static Expr C(uint64_t c) { return Expr::constant(c); }
    static Expr one() { return Expr::constant(1); }

    void constraint(const Expr& e) { emit(KIND_PLAIN, e); }
    void transition(const Expr& e) { emit(KIND_TRANSITION, e); }
    void first_row(const Expr& e) { emit(KIND_FIRST, e); }
    void last_row(const Expr& e) { emit(KIND_LAST, e); }

    // one PermutationPair: the lhs columns, under any row permutation, hold what the rhs columns hold (checked by air_parse_checked)
    void permutation_pair(const std::vector<std::pair<uint32_t, uint32_t>>& entries) {
        std::vector<uint64_t> e;
        for (const auto& lr : entries) {
            check_col(lr.first);
            check_col(lr.second);
            e.push_back((uint64_t)lr.first | ((uint64_t)lr.second << 32));
        }
        prog_.perm_pairs.push_back(std::move(e));
    }

    // One lookup of column `input` in table column `table` through the witness columns permuted_input (pi) and permuted_table (pt), in
    // the form of evm's eval_lookups: the constraint (N(pi) - L(pi)) (N(pi) - N(pt)) on every row and the last-row constraint
    // N(pi) - N(pt), whose next row is row 0; then the pairs [(input, pi)] and [(table, pt)], in that order.  starkhip_lookup_columns
    // fills pi and pt; lookups() is the list it takes.  The validator's limits decide what fits: two pairs need degree >= 3, and an
    // AIR holds at most B batches of B = degree - 1 pairs.  One batch shares one challenge: COMPAT.md 2a says what that shows.
    void lookup(uint32_t input, uint32_t table, uint32_t permuted_input, uint32_t permuted_table) {
        constraint((N(permuted_input) - L(permuted_input)) * (N(permuted_input) - N(permuted_table)));
        last_row(N(permuted_input) - N(permuted_table));
        permutation_pair({{input, permuted_input}});
        permutation_pair({{table, permuted_table}});
        lookups_.push_back({input, table, permuted_input, permuted_table});
    }
    struct Lookup { uint32_t input, table, permuted_input, permuted_table; };  // as starkhip_lookup_t

    // One LogUp lookup (COMPAT.md L1-L7): every cell of `columns` occurs in column `table`, and column `frequencies` holds, row by row,
    // how often the row's table value is looked up.  No constraint is emitted here: the prover and the verifiers add the helper and Z
    // constraints after the AIR's own.  The validator refuses it beside permutation pairs and at degree 1.
    void logup(const std::vector<uint32_t>& columns, uint32_t table, uint32_t frequencies) {
        AirProgram::Logup lk;
        for (uint32_t c : columns) lk.cols.push_back(AirProgram::Column(c));
        lk.filters.resize(columns.size());
        lk.table = AirProgram::Column(table);
        lk.freq = AirProgram::Column(frequencies);
        check_logup(lk);
        prog_.logups.push_back(std::move(lk));
    }
    // The general LogUp lookup: pairs of a looked-up Column and its Filter (an empty one for none), a table Column and a frequencies
    // Column.  Column { constant, local terms, next terms } and Filter { products, sums } are AirProgram's; column_of() makes one.  Once a
    // general lookup is declared every lookup of the program, plain ones included, goes into the general section.
    static AirProgram::Column column_of(gl_t constant, const std::vector<std::pair<uint32_t, gl_t>>& local, const std::vector<std::pair<uint32_t, gl_t>>& next = {}) {
        AirProgram::Column c;
        c.constant = constant;
        c.n_local = (uint32_t)local.size();
        for (const auto& t : local) c.terms.push_back({t.first, t.second});
        for (const auto& t : next) c.terms.push_back({t.first, t.second});
        return c;
    }
    static AirProgram::Filter filter_of(const std::vector<std::pair<AirProgram::Column, AirProgram::Column>>& products, const std::vector<AirProgram::Column>& sums = {}) {
        AirProgram::Filter f;
        f.n_products = (uint32_t)products.size();
        for (const auto& ab : products) { f.cols.push_back(ab.first); f.cols.push_back(ab.second); }
        f.cols.insert(f.cols.end(), sums.begin(), sums.end());
        return f;
    }
    void logup_columns(const std::vector<std::pair<AirProgram::Column, AirProgram::Filter>>& pairs, const AirProgram::Column& table, const AirProgram::Column& frequencies) {
        AirProgram::Logup lk;
        for (const auto& vf : pairs) { lk.cols.push_back(vf.first); lk.filters.push_back(vf.second); }
        lk.table = table;
        lk.freq = frequencies;
        check_logup(lk);
        prog_.logups.push_back(std::move(lk));
        prog_.logup_section2 = true;
    }
    const std::vector<Lookup>& lookups() const { return lookups_; }

    uint32_t count() const { return prog_.n_constraints; }

    AirProgram finish() {
        flush_group();
        prog_.code.push_back(0);
        return prog_;
    }

  private:
    struct Pending {
        std::vector<uint32_t> words;  // encoded terms of one constraint
    };
    AirProgram prog_;
    std::map<uint64_t, uint32_t> const_idx_;
    bool open_ = false;
    uint32_t cur_kind_ = 0;
    std::vector<uint32_t> cur_gates_;
    std::vector<Pending> cur_;
    std::vector<Lookup> lookups_;

    void check_col(uint32_t col) const {
        if (col >= prog_.n_cols) throw std::runtime_error("air_ir: column " + std::to_string(col) + " out of range");
    }

    void check_logup(const AirProgram::Logup& lk) const {
        lk.each_column([&](uint32_t col) { check_col(col); });
    }

    uint32_t const_index(gl_t c) {
        auto it = const_idx_.find(c);
        if (it != const_idx_.end()) return it->second;
        uint32_t i = (uint32_t)prog_.consts.size();
        prog_.consts.push_back(c);
        const_idx_[c] = i;
        return i;
    }

    void emit(uint32_t kind, const Expr& e) {
        std::vector<uint32_t> gates = e.gates;
        std::sort(gates.begin(), gates.end());
        Poly body = e.body;
        if (body.m.empty()) {
            // identically-zero constraint: keep its index (alpha power) with an explicit 0 term
            Mono z;
            z.coef = 0;
            z.pi = -1;
            body.m.push_back(z);
        }
        size_t maxf = 0;
        for (auto& m : body.m) maxf = std::max(maxf, m.f.size());
        size_t deg = gates.size() + maxf + ((kind == KIND_FIRST || kind == KIND_LAST) ? 1 : 0);
        if (deg > prog_.degree)
            throw std::runtime_error("air_ir: constraint " + std::to_string(prog_.n_constraints) + " has degree " +
                                     std::to_string(deg) + " > " + std::to_string(prog_.degree));
        if (!open_ || kind != cur_kind_ || gates != cur_gates_ || cur_.size() >= AIR_MAX_GROUP) {
            flush_group();
            open_ = true;
            cur_kind_ = kind;
            cur_gates_ = gates;
        }
        Pending p;
        for (size_t t = 0; t < body.m.size(); t++) {
            const Mono& m = body.m[t];
            if (m.f.size() > 3) throw std::runtime_error("air_ir: term with more than 3 cell factors");
            uint32_t ck, idx = 0;
            if (m.pi >= 0) {
                if (m.coef == 1) ck = CK_PI;
                else if (m.coef == GL_P - 1) ck = CK_NEG_PI;
                else throw std::runtime_error("air_ir: scaled public input");
                idx = (uint32_t)m.pi;
            } else if (m.coef == 1) {
                ck = CK_PLUS;
            } else if (m.coef == GL_P - 1) {
                ck = CK_MINUS;
            } else {
                ck = CK_CONST;
                idx = const_index(m.coef);
            }
            p.words.push_back(TermWord{(uint32_t)m.f.size(), ck, idx, t + 1 == body.m.size()}.encode());
            for (uint32_t r : m.f) p.words.push_back(r);
        }
        cur_.push_back(std::move(p));
        prog_.n_constraints++;
    }

    void flush_group() {
        if (!open_) return;
        prog_.group_off.push_back((uint32_t)prog_.code.size());
        prog_.group_k0.push_back(prog_.n_constraints - (uint32_t)cur_.size());
        prog_.code.push_back(GroupWord{cur_kind_, (uint32_t)cur_gates_.size(), (uint32_t)cur_.size()}.encode());
        for (uint32_t g : cur_gates_) prog_.code.push_back(g);
        for (auto& p : cur_) prog_.code.insert(prog_.code.end(), p.words.begin(), p.words.end());
        cur_.clear();
        open_ = false;
    }
};

}  // namespace starkhip
