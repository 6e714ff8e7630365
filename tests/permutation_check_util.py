"""What the tests of starkhip_check_trace_permutations (CPU replay and GPU) share: the ground truth in Python -- collections.Counter
over tuples mod p, then the "highest rows" rule -- independent of the C++, the test AIRs beyond permutation_ref.make_air, the traces
that force a key collision, and the comparison of a report with the reference.  Test code."""
from collections import Counter, defaultdict

import numpy as np

import permutation_ref as R
import starky_bls12_381_amd as S
from starky_bls12_381_amd.air_builder import AirBuilder

P = R.P
_AIRS = {}


# ------------------------------------------------------------------------------------------------ the reference
def reference(pairs, trace):
    """pairs: [[(lhs column, rhs column), ...], ...]; trace: row-major, any representative of a cell.
    -> (per_pair [n_pairs], masks bool[n_pairs, 2, n], list [(pair, side, row), ...] in the fixed order)"""
    rows = [[int(x) % P for x in row] for row in np.asarray(trace).tolist()]
    n = len(rows)
    per_pair, masks, entries = [], np.zeros((len(pairs), 2, n), dtype=bool), []
    for q, pair in enumerate(pairs):
        tuples = [[tuple(row[e[side]] for e in pair) for row in rows] for side in (0, 1)]
        counts = [Counter(tuples[0]), Counter(tuples[1])]
        flagged = [[], []]
        for side in (0, 1):
            holding = defaultdict(list)
            for r, v in enumerate(tuples[side]):
                holding[v].append(r)  # ascending
            for v, rs in holding.items():
                surplus = counts[side][v] - counts[1 - side][v]
                if surplus > 0:
                    flagged[side] += rs[-surplus:]  # the highest rows holding v
        assert len(flagged[0]) == len(flagged[1])
        per_pair.append(len(flagged[0]))
        for side in (0, 1):
            for r in sorted(flagged[side]):
                masks[q, side, r] = True
                entries.append((q, side, r))
    return per_pair, masks, entries


def assert_equals_reference(rep, pairs, trace, cap=1024, undecided=()):
    """rep (a PermutationCheck) is the reference's answer for `trace`; the pairs in `undecided` are expected undecided instead."""
    per_pair, masks, entries = reference(pairs, trace)
    for q in undecided:
        per_pair[q] = S.PERM_UNDECIDED
        masks[q] = False
    entries = [e for e in entries if e[0] not in undecided]
    decided = [c for q, c in enumerate(per_pair) if q not in undecided]
    assert rep.pairs == len(pairs) and rep.pairs_undecided == len(undecided)
    assert rep.pairs_violated == sum(1 for c in decided if c)
    assert rep.unmatched == 2 * sum(decided) == len(entries)
    assert rep.per_pair.tolist() == per_pair
    assert np.array_equal(rep.masks, masks)
    assert rep.list.tolist() == [list(e) for e in entries[:cap]]
    return per_pair


def assert_same_report(a, b):
    """two PermutationChecks agree byte for byte: counts, per_pair, masks and list"""
    for f in ("pairs", "pairs_violated", "pairs_undecided", "unmatched", "reseeds"):
        assert getattr(a, f) == getattr(b, f), f
    assert np.array_equal(a.per_pair, b.per_pair) and np.array_equal(a.mask_words, b.mask_words) and np.array_equal(a.list, b.list)


# ------------------------------------------------------------------------------------------------ AIRs
def _register(key, build):
    if key not in _AIRS:
        blob = build()
        _AIRS[key] = (S.register_air(blob, name="PermCheck_%s" % "_".join(str(k) for k in key)), R.split_program(blob)[1])
    return _AIRS[key]


def range_air():
    """(air, pairs): two columns and ONE one-entry pair (0, 1) -- the range-check case, whose sort key is the cell itself"""
    def build():
        b = AirBuilder(2, 0, 2)
        b.constraint(b.L(0) - b.L(0))
        b.permutation_pair([(0, 1)])
        return b.finish()
    return _register(("range",), build)


# The validator accepts at most B batches of B = degree - 1 pairs, and degree <= 8: 49 pairs, not the 64 a program may list.  So the
# widest and most numerous it accepts: one pair of 64 entries (STARKHIP_AIR_MAX_PERMUTATION_ENTRIES) and 48 one-entry pairs.
WIDE_ENTRIES, WIDE_SINGLES = 64, 48


def wide_air():
    """(air, pairs): 128 columns of declared degree 8; pair 0 = {(c, 64 + c) for c < 64}, then the one-entry pairs (c, 64 + c), c < 48"""
    def build():
        b = AirBuilder(2 * WIDE_ENTRIES, 0, 8)
        b.constraint(b.L(0) - b.L(0))
        b.permutation_pair([(c, WIDE_ENTRIES + c) for c in range(WIDE_ENTRIES)])
        for c in range(WIDE_SINGLES):
            b.permutation_pair([(c, WIDE_ENTRIES + c)])
        return b.finish()
    return _register(("wide",), build)


def wide_trace(n_rows, seed):
    """a trace of wide_air() whose rhs half is the lhs half under one row permutation: every pair holds"""
    rng = np.random.default_rng(seed)
    lhs = rng.integers(0, P, (n_rows, WIDE_ENTRIES), dtype=np.uint64)
    return np.ascontiguousarray(np.concatenate([lhs, lhs[rng.permutation(n_rows)]], axis=1))


# ------------------------------------------------------------------------------------------------ collisions
def key(tup, s):
    return sum(pow(s, t, P) * (int(v) % P) for t, v in enumerate(tup)) % P


def collision_trace(n_rows, seed, trace_seed=5):
    """(trace of permutation_ref.make_air(3, 6), the two lhs tuples): a true permutation except that rhs cell (n - 1, column 4) is
    changed, with the lhs tuples (a, b, c) on row 0 and (a + s, b - 1, c) on row 1 -- equal keys under s = perm_check_seeds(seed)[0] --
    and their partners on two rhs rows"""
    s = S.perm_check_seeds(seed)[0]
    trace = R.make_trace(3, n_rows, trace_seed)[0]
    a, b, c = 1234567, 7654321, 1111111
    t0, t1 = (a, b, c), ((a + s) % P, b - 1, c)
    for tup, lhs_row in ((t0, 0), (t1, 1)):
        old = [int(x) for x in trace[lhs_row, 0:3]]
        rhs_row = next(r for r in range(n_rows) if [int(x) for x in trace[r, 3:6]] == old)
        trace[lhs_row, 0:3] = tup
        trace[rhs_row, 3:6] = tup
    trace[n_rows - 1, 4] = (int(trace[n_rows - 1, 4]) + 1) % P
    return trace, (t0, t1)


def undecided_difference(seed, width=5):
    """a nonzero d of `width` >= 5 words with sum_t s^t d_t = 0 mod p for each of the four attempt seeds s: a vector in the null space
    of their 4 x width Vandermonde matrix, by Gaussian elimination mod p with the free variables set to 1"""
    seeds = S.perm_check_seeds(seed)
    m = [[pow(s, t, P) for t in range(width)] for s in seeds]
    piv = []
    for col in range(width):
        r = next((i for i in range(len(piv), len(m)) if m[i][col]), None)
        if r is None:
            continue
        m[len(piv)], m[r] = m[r], m[len(piv)]
        row = m[len(piv)]
        inv = pow(row[col], P - 2, P)
        m[len(piv)] = row = [x * inv % P for x in row]
        for i in range(len(m)):
            if i != len(piv) and m[i][col]:
                f = m[i][col]
                m[i] = [(x - f * y) % P for x, y in zip(m[i], row)]
        piv.append(col)
        if len(piv) == len(m):
            break
    d = [0 if c in piv else 1 for c in range(width)]
    for i, col in enumerate(piv):
        d[col] = -sum(m[i][c] * d[c] for c in range(width) if c not in piv) % P
    assert any(d) and all(key(d, s) == 0 for s in seeds)
    return d


def undecided_trace(n_rows, seed, trace_seed=9):
    """a satisfying trace of wide_air() in which lhs rows 0 and 1 (and their rhs partners) differ by undecided_difference(seed) in
    entries 0 .. 4 of the wide pair and in nothing else: equal keys under every attempt seed"""
    trace = wide_trace(n_rows, trace_seed)
    d = undecided_difference(seed)
    lhs1 = [int(x) for x in trace[1, :WIDE_ENTRIES]]
    rhs_row = next(r for r in range(n_rows) if [int(x) for x in trace[r, WIDE_ENTRIES:]] == lhs1)
    new = [int(x) for x in trace[0, :WIDE_ENTRIES]]
    for t, dt in enumerate(d):
        new[t] = (new[t] + dt) % P
    trace[1, :WIDE_ENTRIES] = new
    trace[rhs_row, WIDE_ENTRIES:] = new
    return trace
