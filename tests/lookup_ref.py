"""What the tests of starkhip_lookup_columns (CPU replay and GPU) share: the ground truth in Python -- numpy sorts and boolean masks,
independent of the C++ -- which also asserts on its own output what a lookup witness must have, the data cases, and the comparison of
a filled trace and its report with the reference.  Test code."""
import numpy as np

P = 0xFFFFFFFF00000001
_P = np.uint64(P)


def canonical(x):
    return np.asarray(x, dtype=np.uint64) % _P


# ------------------------------------------------------------------------------------------------ the reference
def assert_witness(a, t, pi, pt):
    """pi, pt are a lookup witness for input a and table t (all canonical): two permutations, pi ascending, and on every row i, the
    wrap row included, (pi[i+1] - pi[i]) (pi[i+1] - pt[i+1]) = 0; pi[0] = pt[0]."""
    assert np.array_equal(np.sort(pi), np.sort(a)) and np.array_equal(np.sort(pt), np.sort(t))
    assert (pi[1:] >= pi[:-1]).all()
    nxt_pi, nxt_pt = np.roll(pi, -1), np.roll(pt, -1)
    assert ((nxt_pi == pi) | (nxt_pi == nxt_pt)).all()
    assert pi[0] == pt[0]
    assert not (pi >= _P).any() and not (pt >= _P).any()


def reference(a, t):
    """One lookup of input column a in table column t (any representative of a cell) -> (missing bool[n], permuted_input,
    permuted_table); the two columns are None when the lookup fails."""
    a, t = canonical(a), canonical(t)
    n = a.size
    missing = ~np.isin(a, t)
    if missing.any():
        return missing, None, None
    A, T = np.sort(a), np.sort(t)
    head = np.ones(n, dtype=bool)
    head[1:] = A[1:] != A[:-1]
    first = np.ones(n, dtype=bool)
    first[1:] = T[1:] != T[:-1]
    used = first & np.isin(T, a)
    assert int(head.sum()) == int(used.sum())
    pt = A.copy()
    pt[~head] = T[~used]  # the k-th non-head position takes the k-th unused entry
    assert_witness(a, t, A, pt)
    return missing, A, pt


def fill(trace, lookups, layout=0):
    """-> (the trace as the call must leave it, per_lookup [n_lookups], masks bool[n_lookups, n], list [(lookup, row), ...])"""
    trace = np.asarray(trace, dtype=np.uint64)
    cols = trace.T if layout == 0 else trace  # cols[c] = column c
    n = cols.shape[1]
    out = trace.copy()
    out_cols = out.T if layout == 0 else out
    per, masks, entries = [], np.zeros((len(lookups), n), dtype=bool), []
    for q, (i, t, pi, pt) in enumerate(lookups):
        missing, A, PT = reference(cols[i], cols[t])
        per.append(int(missing.sum()))
        masks[q] = missing
        entries += [(q, int(r)) for r in np.flatnonzero(missing)]
        if A is not None:
            out_cols[pi], out_cols[pt] = A, PT
    return out, per, masks, entries


def assert_report(rep, per, masks, entries, cap=1024):
    assert rep.lookups == len(per) and rep.failed == sum(1 for c in per if c) and rep.missing_rows == sum(per) == len(entries)
    assert rep.per_lookup.tolist() == per
    assert np.array_equal(rep.masks, masks)
    assert rep.list.tolist() == [list(e) for e in entries[:cap]]


def assert_same_report(a, b):
    """two LookupReports agree byte for byte"""
    for f in ("lookups", "failed", "missing_rows"):
        assert getattr(a, f) == getattr(b, f), f
    assert np.array_equal(a.per_lookup, b.per_lookup) and np.array_equal(a.mask_words, b.mask_words) and np.array_equal(a.list, b.list)


def run(call, trace, lookups, layout=0, cap=1024):
    """`call(trace, lookups, layout, cap)` fills its (writable) trace and returns a LookupReport: the filled trace and the report are
    the reference's.  -> (the filled trace, the report)"""
    want, per, masks, entries = fill(trace, lookups, layout)
    got = np.array(trace, dtype=np.uint64, copy=True, order="C")
    rep = call(got, lookups, layout, cap)
    assert np.array_equal(got, want)
    assert_report(rep, per, masks, entries, cap)
    return got, rep


# ------------------------------------------------------------------------------------------------ data
LOOKUP = (0, 1, 2, 3)  # of one_lookup_trace
N_COLS = 6


def data_cases(n, seed):
    """name -> (input column, table column) of n rows, every one a lookup that holds"""
    rng = np.random.default_rng(seed)
    cases = {}
    table = np.arange(n, dtype=np.uint64)
    cases["range"] = (rng.integers(0, n, n, dtype=np.uint64), table)
    cases["all_equal"] = (np.full(n, n // 2, dtype=np.uint64), table)  # one head
    spread = rng.permutation(table * np.uint64(3) + np.uint64(1))
    cases["permutation"] = (rng.permutation(spread), spread)  # no non-head: the second placement is empty
    dup = rng.integers(0, n // 2 + 1, n, dtype=np.uint64)
    cases["dup_table"] = (rng.choice(dup, n), dup)
    big = rng.integers(1 << 32, P, n, dtype=np.uint64)  # every sort digit matters
    big[0], big[n - 1] = P - 1, (1 << 32) + 1
    pick = rng.choice(big, n)
    pick[n - 1] = P - 1
    cases["big"] = (pick, rng.permutation(big))
    return cases


def one_lookup_trace(a, t, seed=0, layout=0):
    """[n][6] (or its transpose): columns 0 = a, 1 = t, 2 and 3 the output columns holding other bytes, 4 and 5 bystanders"""
    rng = np.random.default_rng(seed)
    n = len(a)
    cols = rng.integers(0, 1 << 63, (N_COLS, n), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    cols[0], cols[1] = a, t
    return np.ascontiguousarray(cols if layout == 1 else cols.T)


SHARED = [(0, 2, 3, 4), (1, 2, 5, 6)]  # two inputs, one table, of shared_table_trace
SHARED_COLS = 8


def shared_table_trace(n, seed, fail_first=False, layout=0):
    """[n][8]: inputs in columns 0 and 1, an 8-bit range table in column 2 (n >= 256) or 0 .. n - 1, outputs 3 .. 6, a bystander;
    fail_first: input 0 holds values the table lacks on rows 0 and n - 1"""
    rng = np.random.default_rng(seed)
    m = min(n, 256)
    cols = rng.integers(0, 1 << 63, (SHARED_COLS, n), dtype=np.uint64)
    cols[0], cols[1] = rng.integers(0, m, n, dtype=np.uint64), rng.integers(0, m, n, dtype=np.uint64)
    cols[2] = np.arange(n, dtype=np.uint64) % np.uint64(m)
    if fail_first:
        cols[0][0], cols[0][n - 1] = m, P - 1
    return np.ascontiguousarray(cols if layout == 1 else cols.T)


def missing_cases(n, seed):
    """name -> (input, table, the rows that must be reported): the table holds 10, 12, ..; the absent values lie below (3), between
    (an odd one) and above (2 n + 100) its values"""
    rng = np.random.default_rng(seed)
    table = rng.permutation(np.arange(n, dtype=np.uint64) * np.uint64(2) + np.uint64(10))
    absent = {"below": 3, "between": 9 + n - (n & 1), "above": 2 * n + 100}  # (odd, and inside 10 .. 2 n + 8)
    cases = {}
    for name, v in absent.items():
        a = rng.choice(table, n)
        r = {"below": 0, "between": n // 2, "above": n - 1}[name]
        a[r] = v
        cases["one_" + name] = (a, table, [r])
    a = np.array([list(absent.values())[i % 3] for i in range(n)], dtype=np.uint64)
    cases["every_row"] = (a, table, list(range(n)))
    return cases
