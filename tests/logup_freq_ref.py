"""What the tests of starkhip_logup_frequencies (CPU replay and GPU) share: the ground truth in Python -- numpy's unique, searchsorted
and bincount, nothing of the C++ -- and the AIRs and traces they run on.  The rule (include/starkhip.h, "LogUp FREQUENCIES"), per
lookup with m looked-up columns, table column t and frequencies column f over n rows, cells read mod p: row r of t is a FIRST when no
earlier row holds its value; a looked-up cell is MISSING when its value occurs nowhere in t; when no cell is missing, f[r] = the
number of looked-up cells equal to t[r] on a first and 0 elsewhere; otherwise f stays as it was.  fill() asserts on its own output
that sum f = m n, that f is nonzero only on firsts, and (small shapes) that logup_ref.polys_and_closing closes to 0 with it."""
import numpy as np

import logup_ref as L

P = L.P
CLOSING_CELLS = 4096  # the closing values are Python-integer loops: checked up to this many looked-up cells per lookup


def make_air(n_cols, lookups, degree=3):
    """A program of n_cols columns whose LogUp lookups are `lookups` = [(columns, table, frequencies), ...]; its own constraints (on
    column 0 alone) are there because a program has some, no test here proves them."""
    from starky_bls12_381_amd.air_builder import AirBuilder
    b = AirBuilder(n_cols, 1, degree)
    b.transition(b.N(0) - b.L(0) - 1)
    b.first_row(b.L(0) - b.PI(0))
    for cols, table, freq in lookups:
        b.logup(list(cols), table, freq)
    return b.finish()


def view(trace, layout):
    """the trace as [n][C] whatever its layout (a view: writes go through)"""
    return trace if layout == 0 else trace.T


class Expected:
    """fill()'s result: `trace` (the filled copy, in the layout given), `per_lookup`, `per_column` (np.uint32), `masks`
    (bool [lookups][n]), `list` (np.uint64 [min(cap, missing_rows)][2]), and the report's counts."""


def fill(trace, lookups, layout=0, cap=1024, degree=3):
    out = trace.copy()
    t, o = view(trace, layout), view(out, layout)
    n = t.shape[0]
    e = Expected()
    e.trace, e.lookups, e.failed, e.missing_cells, e.missing_rows = out, len(lookups), 0, 0, 0
    per_lookup, per_column, masks, entries = [], [], np.zeros((len(lookups), n), dtype=bool), []
    for q, (cols, table, freq) in enumerate(lookups):
        tv = t[:, table] % np.uint64(P)
        uniq, first = np.unique(tv, return_index=True)  # first: the lowest row of each value
        cells = t[:, list(cols)] % np.uint64(P)
        pos = np.searchsorted(uniq, cells)
        hit = uniq[np.minimum(pos, len(uniq) - 1)] == cells
        miss = ~hit
        per_column += [int(x) for x in miss.sum(axis=0)]
        per_lookup.append(int(miss.sum()))
        masks[q] = miss.any(axis=1)
        if per_lookup[-1]:
            e.failed += 1
            e.missing_cells += per_lookup[-1]
            e.missing_rows += int(masks[q].sum())
            entries += [(q, int(r)) for r in np.nonzero(masks[q])[0]]
            continue
        f = np.zeros(n, dtype=np.uint64)
        f[first] = np.bincount(pos.reshape(-1), minlength=len(uniq)).astype(np.uint64)
        o[:, freq] = f
        # ---- the reference's own output, checked
        m = len(cols)
        assert int(f.sum()) == m * n
        is_first = np.zeros(n, dtype=bool)
        is_first[first] = True
        assert not f[~is_first].any()
        if m * n <= CLOSING_CELLS:
            rows = [[int(x) for x in row] for row in o]
            _, closing, zeros = L.polys_and_closing([(list(cols), table, freq)], degree, rows, (0x123456789ABCDEF % P, 0xFEDCBA987654321 % P))
            assert zeros == 0 and closing == [[0], [0]], (q, closing, zeros)
    e.per_lookup, e.per_column, e.masks = np.array(per_lookup, dtype=np.uint32), np.array(per_column, dtype=np.uint32), masks
    e.list = np.array(entries[:cap], dtype=np.uint64).reshape(-1, 2)
    return e


def assert_same(rep, e):
    """a LogupReport against fill()'s Expected"""
    assert (rep.lookups, rep.failed, rep.missing_cells, rep.missing_rows) == (e.lookups, e.failed, e.missing_cells, e.missing_rows), rep
    assert np.array_equal(rep.per_lookup, e.per_lookup)
    assert np.array_equal(rep.per_column, e.per_column)
    assert np.array_equal(rep.masks, e.masks)
    assert np.array_equal(rep.list, e.list)


def assert_same_report(a, b):
    """two LogupReports"""
    assert (a.lookups, a.failed, a.missing_cells, a.missing_rows) == (b.lookups, b.failed, b.missing_cells, b.missing_rows)
    for x, y in ((a.per_lookup, b.per_lookup), (a.per_column, b.per_column), (a.mask_words, b.mask_words), (a.list, b.list)):
        assert np.array_equal(x, y)


# ---- traces.  Columns: 0 the program's own, 1 the table, then per lookup its m columns and its frequencies column.
TABLE = 1


def layout_of(m, n_lookups, tables=None):
    """[(columns, table, frequencies)] and the column count: lookup l has columns first .. first + m - 1 and frequencies first + m;
    tables: the table column of each lookup (default: all share column 1), further tables follow the lookups' columns"""
    lookups = []
    for l in range(n_lookups):
        first = 2 + l * (m + 1)
        lookups.append((list(range(first, first + m)), TABLE if tables is None else tables[l], first + m))
    n_cols = 2 + n_lookups * (m + 1)
    if tables is not None:
        n_cols = max(n_cols, max(tables) + 1)
    return lookups, n_cols


def make_trace(n, lookups, n_cols, seed, kind="uniform", layout=0):
    """A trace whose lookups hold, frequencies columns holding junk (the fill must overwrite every row).  kind: "uniform" picks,
    "equal" (every cell one value), "duplicates" (the table holds each value about four times), "big" (values up to p - 1, every
    third looked-up or table cell written as c + p where that fits 64 bits)."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n, n_cols), dtype=np.uint64)
    t[:, 0] = np.arange(n, dtype=np.uint64) + np.uint64(7)
    for tab in sorted({tb for _, tb, _ in lookups}):
        if kind == "duplicates":
            vals = rng.integers(0, max(1, n // 4), size=n).astype(np.uint64) * np.uint64(3) + np.uint64(5)
        elif kind == "big":
            vals = rng.integers(0, P, size=n, dtype=np.uint64)
            vals[0], vals[n - 1] = P - 1, 0
        else:
            vals = rng.permutation(n).astype(np.uint64) * np.uint64(5) + np.uint64(11)
        t[:, tab] = vals
    for cols, tab, freq in lookups:
        m = len(cols)
        picks = np.full((n, m), int(rng.integers(0, n))) if kind == "equal" else rng.integers(0, n, size=(n, m))
        t[:, cols] = t[:, tab][picks]
        t[:, freq] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    if kind == "big":
        named = sorted({c for cols, tab, _ in lookups for c in list(cols) + [tab]})
        for c in named:
            col = t[::3, c]
            small = col < np.uint64((1 << 64) - P)
            col[small] += np.uint64(P)
            t[::3, c] = col
    return np.ascontiguousarray(t if layout == 0 else t.T)


def run(call, air, trace, lookups, layout=0, cap=1024):
    """call(air, trace, layout, cap) -> LogupReport on a copy of `trace`; checks the copy and the report against fill() and that nothing
    but frequencies columns changed.  Returns (the filled copy, the report)."""
    got = trace.copy()
    rep = call(air, got, layout, cap)
    e = fill(trace, lookups, layout, cap)
    assert_same(rep, e)
    assert np.array_equal(got, e.trace)
    return got, rep
