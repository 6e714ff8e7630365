"""Symbolic builder of constraint programs for user-defined AIRs (register_air).

The Python twin of `Expr` / `AirBuilder` in csrc/air_ir.h, rule for rule, so a program written here serialises to exactly the words
the C++ builder would produce: cells of the local (`L`) and next (`N`) row, public inputs (`PI`), constants, `+ - *`; a product with a
single cell or with `1 - cell` becomes a gate of the constraint, every other product is expanded; consecutive constraints with the same
kind and gates share a group (at most 255), and coefficients other than +-1 go to the const table in order of first use.

    b = AirBuilder(n_cols=4, n_pis=3, degree=3)
    b.first_row(b.L(0) - b.PI(0))
    b.transition(b.N(1) - b.L(0) - b.L(1))
    b.constraint(b.L(3) * (1 - b.L(3)))
    air = register_air(b.finish(), name="MyStark")

Limits (checked here as the C++ builder checks them): at most 3 cell factors per term (after gate extraction), no product of two
public inputs, a public input only with coefficient +-1, and every constraint within the declared degree (gates + the most factors of
a term, + 1 for first / last-row constraints).
"""
import numpy as np

P = 0xFFFFFFFF00000001
AIR_MAGIC = 0x3152495F52494153  # "SAIR_IR1"
AIR_PERM_MAGIC = 0x3153524941504D50  # "PMPAIRS1": the section of permutation pairs
AIR_LOGUP_MAGIC = 0x3130535055474F4C  # "LOGUPS01": the section of LogUp lookups
AIR_LOGUP2_MAGIC = 0x3230535055474F4C  # "LOGUPS02": the same over Columns and Filters
KIND_PLAIN, KIND_TRANSITION, KIND_FIRST, KIND_LAST = 0, 1, 2, 3
CK_PLUS, CK_MINUS, CK_CONST, CK_PI, CK_NEG_PI = 0, 1, 2, 3, 4
REF_NEXT, REF_COMPL, REF_COL_MASK = 1 << 30, 1 << 31, 0xFFFFFF
AIR_MAX_GROUP = 255


class _Mono:
    __slots__ = ("coef", "pi", "f")

    def __init__(self, coef, pi=-1, f=()):
        self.coef, self.pi, self.f = coef, pi, list(f)

    def copy(self):
        return _Mono(self.coef, self.pi, self.f)


def _add_mono(monos, x):
    if x.coef == 0:
        return
    for i, m in enumerate(monos):
        if m.pi == x.pi and m.f == x.f:
            m.coef = (m.coef + x.coef) % P
            if m.coef == 0:
                del monos[i]
            return
    monos.append(x.copy())


def _poly_mul(a, b):
    r = []
    for x in a:
        for y in b:
            if x.pi >= 0 and y.pi >= 0:
                raise ValueError("air_builder: product of two public inputs")
            _add_mono(r, _Mono(x.coef * y.coef % P, x.pi if x.pi >= 0 else y.pi, sorted(x.f + y.f)))
    return r


def _is_const(body, c):
    return len(body) == 1 and body[0].pi < 0 and not body[0].f and body[0].coef == c


def _is_single_cell(body):
    return len(body) == 1 and body[0].pi < 0 and len(body[0].f) == 1 and body[0].coef == 1


def _complement_cell(body):
    """cell if body is 1 - cell, else None"""
    if len(body) != 2:
        return None
    one = neg = None
    for x in body:
        if x.pi < 0 and not x.f and x.coef == 1:
            one = x
        if x.pi < 0 and len(x.f) == 1 and x.coef == P - 1:
            neg = x
    return neg.f[0] if one is not None and neg is not None else None


class Expr:
    """value = prod(gates) * body (csrc/air_ir.h `Expr`)."""

    def __init__(self, gates=(), body=()):
        self.gates = list(gates)
        self.body = [m.copy() for m in body]

    @staticmethod
    def constant(c):
        e = Expr()
        _add_mono(e.body, _Mono(int(c) % P))
        return e

    @staticmethod
    def cell(ref):
        return Expr(body=[_Mono(1, -1, [ref])])

    @staticmethod
    def pub(i):
        return Expr(body=[_Mono(1, i)])

    def expanded(self):
        p = [m.copy() for m in self.body]
        for g in self.gates:
            c = _Mono(1, -1, [g & ~REF_COMPL])
            if g & REF_COMPL:
                c.coef = P - 1
                q = [_Mono(1), c]
            else:
                q = [c]
            p = _poly_mul(p, q)
        return p

    def __add__(self, other):
        other = _expr(other)
        r = Expr(body=self.expanded())
        for x in other.expanded():
            _add_mono(r.body, x)
        return r

    def __sub__(self, other):
        other = _expr(other)
        r = Expr(body=self.expanded())
        for x in other.expanded():
            _add_mono(r.body, _Mono((P - x.coef) % P, x.pi, x.f))
        return r

    def __mul__(self, other):
        a, b = self, _expr(other)
        r = Expr(gates=a.gates + b.gates)
        if _is_const(a.body, 1):
            r.body = [m.copy() for m in b.body]
        elif _is_const(b.body, 1):
            r.body = [m.copy() for m in a.body]
        elif _is_single_cell(a.body):
            r.gates.append(a.body[0].f[0])
            r.body = [m.copy() for m in b.body]
        elif _is_single_cell(b.body):
            r.gates.append(b.body[0].f[0])
            r.body = [m.copy() for m in a.body]
        elif _complement_cell(a.body) is not None:
            r.gates.append(_complement_cell(a.body) | REF_COMPL)
            r.body = [m.copy() for m in b.body]
        elif _complement_cell(b.body) is not None:
            r.gates.append(_complement_cell(b.body) | REF_COMPL)
            r.body = [m.copy() for m in a.body]
        else:
            r.body = _poly_mul(a.body, b.body)
        return r

    def __radd__(self, other):
        return _expr(other) + self

    def __rsub__(self, other):
        return _expr(other) - self

    def __rmul__(self, other):
        return _expr(other) * self

    def __neg__(self):
        return Expr.constant(0) - self


def _expr(x):
    if isinstance(x, Expr):
        return x
    if isinstance(x, (int, np.integer)):
        return Expr.constant(int(x))
    raise TypeError(f"air_builder: cannot use {type(x).__name__} in a constraint")


class Column:
    """constant + sum coefficient * local[column] + sum coefficient * next[column] (starky's `Column`, COMPAT.md §2c): what a general
    LogUp lookup looks up, its table and its frequencies.  `local` and `next` are lists of (trace column, coefficient); a coefficient
    is reduced mod p (so -1 is p - 1) and must not be 0.  The next row of the last row is row 0."""

    def __init__(self, local=(), next=(), constant=0):
        self.local = [(int(c), int(k) % P) for c, k in local]
        self.next = [(int(c), int(k) % P) for c, k in next]
        self.constant = int(constant) % P

    @staticmethod
    def single(col):
        """the plain column `col`: one local cell, coefficient 1, constant 0"""
        return Column([(col, 1)])

    @staticmethod
    def const(c):
        return Column(constant=c)

    def is_plain(self):
        return len(self.local) == 1 and not self.next and self.local[0][1] == 1 and self.constant == 0

    def words(self):
        w = [len(self.local) | (len(self.next) << 32), self.constant]
        for c, k in self.local + self.next:
            w += [c, k]
        return w


class Filter:
    """sum A * B + sum C over `Column`s (starky's `Filter`): `products` a list of (A, B), `sums` a list of C.  The empty filter is 1."""

    def __init__(self, products=(), sums=()):
        self.products = [(_column(a), _column(b)) for a, b in products]
        self.sums = [_column(c) for c in sums]

    def is_empty(self):
        return not self.products and not self.sums

    def words(self):
        w = [len(self.products) | (len(self.sums) << 32)]
        for a, b in self.products:
            w += a.words() + b.words()
        for c in self.sums:
            w += c.words()
        return w


def _column(x):
    """a Column, or a trace column's number for the plain one"""
    return x if isinstance(x, Column) else Column.single(int(x))


class AirBuilder:
    """csrc/air_ir.h `AirBuilder`: constraints in the order of the reference's eval_packed_generic (the order fixes each one's power
    of alpha); finish() returns the serialised program as a numpy uint64 array."""

    def __init__(self, n_cols, n_pis, degree):
        self.n_cols, self.n_pis, self.degree = int(n_cols), int(n_pis), int(degree)
        self.n_constraints = 0
        self.consts, self._const_idx = [], {}
        self.code, self.group_off, self.group_k0 = [], [], []
        self._open, self._kind, self._gates, self._cur = False, 0, [], []
        self.perm_pairs = []
        self.lookups = []  # (input, table, permuted_input, permuted_table) of every lookup()
        self.logups = []  # (columns, table, frequencies) of every logup()
        self.general_logups = []  # every lookup, in declaration order, as (pairs, table, frequencies) of Columns and Filters
        self._logup_general = False  # a logup_columns() was declared: all of them go into the general section

    def L(self, col):
        self._check_col(col)
        return Expr.cell(col)

    def N(self, col):
        self._check_col(col)
        return Expr.cell(col | REF_NEXT)

    def PI(self, i):
        if not 0 <= i < self.n_pis:
            raise ValueError("air_builder: public input index out of range")
        return Expr.pub(i)

    @staticmethod
    def C(c):
        return Expr.constant(c)

    @staticmethod
    def one():
        return Expr.constant(1)

    def constraint(self, e):
        self._emit(KIND_PLAIN, _expr(e))

    def transition(self, e):
        self._emit(KIND_TRANSITION, _expr(e))

    def first_row(self, e):
        self._emit(KIND_FIRST, _expr(e))

    def last_row(self, e):
        self._emit(KIND_LAST, _expr(e))

    def permutation_pair(self, entries):
        """One of starky's `permutation_pairs()`: entries = [(lhs column, rhs column), ...]; the rows of the lhs columns are a permutation
        of the rows of the rhs columns.  Pairs are batched B = max(1, degree - 1) at a time in the order they are declared here."""
        entries = [(int(l), int(r)) for l, r in entries]
        for l, r in entries:
            self._check_col(l)
            self._check_col(r)
        self.perm_pairs.append(entries)

    def lookup(self, input, table, permuted_input, permuted_table):
        """One lookup of column `input` in table column `table` through the witness columns `permuted_input` (pi) and `permuted_table`
        (pt), in the form of evm's `eval_lookups`: the constraint (N(pi) - L(pi)) * (N(pi) - N(pt)) on every row and the last-row
        constraint N(pi) - N(pt), whose next row is row 0; then the pairs [(input, pi)] and [(table, pt)], in that order.  The four
        columns are recorded in `self.lookups`, the list `Prover.lookup_columns` takes to fill pi and pt.  The validator's limits
        decide what fits: two pairs need degree >= 3, and an AIR holds at most B batches of B = degree - 1 pairs.  One batch shares
        one challenge: COMPAT.md §2a says what that does and does not show."""
        cols = tuple(int(c) for c in (input, table, permuted_input, permuted_table))
        pi, pt = cols[2], cols[3]
        self.constraint((self.N(pi) - self.L(pi)) * (self.N(pi) - self.N(pt)))
        self.last_row(self.N(pi) - self.N(pt))
        self.permutation_pair([(cols[0], pi)])
        self.permutation_pair([(cols[1], pt)])
        self.lookups.append(cols)

    def logup(self, columns, table, frequencies):
        """One LogUp lookup (starky >= 0.2's `Lookup`; COMPAT.md L1 - L7): every cell of `columns` occurs in column `table`, and column
        `frequencies` holds, row by row, how often that row's table value is looked up.  No constraint is emitted here: prover and
        verifiers add the helper and Z constraints after the AIR's own.  The validator refuses it beside permutation pairs and at degree 1."""
        columns = [int(c) for c in columns]
        for c in columns + [int(table), int(frequencies)]:
            self._check_col(c)
        self.logups.append((columns, int(table), int(frequencies)))
        self.general_logups.append(([(Column.single(c), Filter()) for c in columns], Column.single(table), Column.single(frequencies)))

    def logup_columns(self, pairs, table, frequencies):
        """One general LogUp lookup (COMPAT.md §2c): `pairs` is a list of (Column, Filter or None) -- each looked-up value with the filter
        that says on which rows it is looked up (1) or not (0) --, `table` and `frequencies` are Columns; a trace column's number stands
        for the plain Column.  Once one is declared the program's lookups, those of logup() included, go into the "LOGUPS02" section in
        declaration order; a program with logup() alone keeps its "LOGUPS01" bytes."""
        pairs = [(_column(v), f if f is not None else Filter()) for v, f in pairs]
        table, frequencies = _column(table), _column(frequencies)
        for v, f in pairs:
            for col in [v] + [x for ab in f.products for x in ab] + f.sums:
                self._check_column(col)
        self._check_column(table)
        self._check_column(frequencies)
        self.general_logups.append((pairs, table, frequencies))
        self._logup_general = True

    def count(self):
        return self.n_constraints

    def finish(self):
        self._flush()
        self.code.append(0)
        words = [AIR_MAGIC, self.n_cols, self.n_pis, self.degree, self.n_constraints, len(self.consts), len(self.code), len(self.group_off)]
        words += self.consts
        code = self.code + [0] * (len(self.code) & 1)
        words += [code[i] | (code[i + 1] << 32) for i in range(0, len(code), 2)]
        words += [off | (k0 << 32) for off, k0 in zip(self.group_off, self.group_k0)]
        if self.perm_pairs:  # the optional section; a program without pairs keeps its bytes
            words += [AIR_PERM_MAGIC, len(self.perm_pairs)]
            for entries in self.perm_pairs:
                words += [len(entries)] + [l | (r << 32) for l, r in entries]
        if self._logup_general:  # the general section holds every lookup
            words += [AIR_LOGUP2_MAGIC, len(self.general_logups)]
            for pairs, table, freq in self.general_logups:
                words += [len(pairs)] + table.words() + freq.words()
                for v, f in pairs:
                    words += v.words() + f.words()
        elif self.logups:  # the other optional section, in the same place
            words += [AIR_LOGUP_MAGIC, len(self.logups)]
            for columns, table, freq in self.logups:
                words += [len(columns), table | (freq << 32)] + columns
        return np.array(words, dtype=np.uint64)

    def _check_col(self, col):
        if not 0 <= col < self.n_cols:
            raise ValueError(f"air_builder: column {col} out of range")

    def _check_column(self, column):
        for c, k in column.local + column.next:
            self._check_col(c)
            if k == 0:
                raise ValueError("air_builder: zero coefficient in a Column")

    def _const_index(self, c):
        if c not in self._const_idx:
            self._const_idx[c] = len(self.consts)
            self.consts.append(c)
        return self._const_idx[c]

    def _emit(self, kind, e):
        gates = sorted(e.gates)
        body = [m.copy() for m in e.body] or [_Mono(0)]  # identically zero: keep its index with an explicit 0 term
        maxf = max(len(m.f) for m in body)
        deg = len(gates) + maxf + (1 if kind in (KIND_FIRST, KIND_LAST) else 0)
        if deg > self.degree:
            raise ValueError(f"air_builder: constraint {self.n_constraints} has degree {deg} > {self.degree}")
        if not self._open or kind != self._kind or gates != self._gates or len(self._cur) >= AIR_MAX_GROUP:
            self._flush()
            self._open, self._kind, self._gates = True, kind, gates
        words = []
        for t, m in enumerate(body):
            if len(m.f) > 3:
                raise ValueError("air_builder: term with more than 3 cell factors")
            idx = 0
            if m.pi >= 0:
                if m.coef == 1:
                    ck = CK_PI
                elif m.coef == P - 1:
                    ck = CK_NEG_PI
                else:
                    raise ValueError("air_builder: scaled public input")
                idx = m.pi
            elif m.coef == 1:
                ck = CK_PLUS
            elif m.coef == P - 1:
                ck = CK_MINUS
            else:
                ck, idx = CK_CONST, self._const_index(m.coef)
            words.append(len(m.f) | (ck << 2) | ((1 << 5) if t + 1 == len(body) else 0) | (idx << 6))
            words += m.f
        self._cur.append(words)
        self.n_constraints += 1

    def _flush(self):
        if not self._open:
            return
        self.group_off.append(len(self.code))
        self.group_k0.append(self.n_constraints - len(self._cur))
        self.code.append(1 | (self._kind << 4) | (len(self._gates) << 8) | (len(self._cur) << 16))
        self.code += self._gates
        for w in self._cur:
            self.code += w
        self._cur, self._open = [], False


SYSTEM_MAGIC = int.from_bytes(b"SYSCTL01", "little")


class SystemBuilder:
    """A system of tables tied by cross-table lookups (starky's `CrossTableLookup`, COMPAT.md §2d): `tables` are the ids of registered
    AIRs (what register_air returned for AirBuilder results), each proved on a trace of its own; ctl() declares that the rows the looking
    endpoints send are the rows the looked endpoint receives.  finish() returns the blob register_system takes.

        sb = SystemBuilder([cpu_air, range_air])
        sb.ctl(looked=(1, [0], Filter(sums=[Column.single(1)])), looking=[(0, [3], Filter(sums=[Column.single(4)]))])
        system = register_system(sb.finish())
    """

    def __init__(self, tables):
        self.tables = [int(t) for t in tables]
        self.ctls = []

    def ctl(self, looked, looking):
        """looked, and each of looking: (table index, columns, filter) -- `columns` a list of Columns (a trace column's number stands for
        the plain one), all of one width; `filter` a Filter, or None for the filter that is 1.  The filter's value is the multiplicity:
        0 / 1 selectors on both sides give a multiset equality, a multiplicity column as the looked side's filter a lookup."""
        eps = [(int(t), [_column(c) for c in cols], f if f is not None else Filter()) for t, cols, f in [looked] + list(looking)]
        self.ctls.append(eps)

    def finish(self):
        words = [SYSTEM_MAGIC, len(self.tables)] + self.tables + [len(self.ctls)]
        for eps in self.ctls:
            words += [len(eps[0][1]), len(eps) - 1]
            for t, cols, f in eps:
                words += [t, len(cols)]
                for c in cols:
                    words += c.words()
                words += f.words()
        return np.array(words, dtype=np.uint64)
