"""What starkhip_check_trace_free_cells must say about a trace: a brute force of its rule in plain Python from the program blob
(air_blob), a hand-written AIR whose free cells are known by construction, and the comparison the CPU and GPU tests share.
Test code."""
import functools

import numpy as np

import air_blob
import starky_bls12_381_amd as S
from random_air import random_air
from starky_bls12_381_amd.air_builder import AirBuilder

P = 0xFFFFFFFF00000001
DELTA = 0x9E3779B97F4A7C15
PLAIN, TRANSITION, FIRST, LAST = range(4)
# random_air (seed, columns, degree, rows) with, per case, (cells, free, columns all free, columns partly free) at DELTA
CPU_CASES = {(1, 1, 2, 8): (8, 7, 0, 1), (2, 7, 3, 16): (112, 17, 1, 1), (3, 40, 4, 32): (1280, 406, 5, 11), (4, 64, 5, 64): (4096, 1093, 4, 20),
             (5, 65, 3, 128): (8320, 2138, 10, 11), (11, 12, 3, 2): (24, 7, 3, 1), (12, 20, 4, 64): (1280, 439, 2, 8)}


def applies(kind, row, n):
    return kind == PLAIN or (kind == TRANSITION and row < n - 1) or (kind == FIRST and row == 0) or (kind == LAST and row == n - 1)


class Expected:
    """The rule, cell by cell: mask[r, c] is True when cell (r, c) is free."""

    def __init__(self, blob, trace, pis, delta=DELTA):
        n, n_cols = trace.shape
        rows = [[int(x) for x in row] for row in trace]
        pis = [int(x) for x in pis]
        caught = np.zeros((n, n_cols), dtype=bool)
        for kind, gates, terms in air_blob.constraints(air_blob.parse_blob(blob)):
            poly = air_blob.expand(gates, terms)
            reads = {r & (air_blob.COL_MASK | air_blob.REF_NEXT) for r in gates} | {r for _, _, cells in terms for r in cells}
            for ref in sorted(reads):
                col, as_next = ref & air_blob.COL_MASK, bool(ref & air_blob.REF_NEXT)
                for r in range(n):
                    frame = (r - 1) % n if as_next else r
                    if not applies(kind, frame, n):
                        continue
                    local, nxt = rows[frame], rows[(frame + 1) % n]
                    changed = list(nxt if as_next else local)
                    changed[col] = (changed[col] + delta) % P
                    if air_blob.evaluate(poly, local if as_next else changed, changed if as_next else nxt, pis):
                        caught[r, col] = True
        self.mask = ~caught
        self.per_column = self.mask.sum(axis=0).astype(np.uint32)
        self.summary = (n * n_cols, int(self.mask.sum()), int((self.per_column == n).sum()),
                        int(((self.per_column > 0) & (self.per_column < n)).sum()))


def summary(fc):
    return (fc.cells, fc.free, fc.free_columns, fc.partly_free_columns)


def assert_free_cells(got, want):
    assert summary(got) == want.summary
    assert got.per_column.dtype == np.uint32 and np.array_equal(got.per_column, want.per_column)
    assert got.mask.dtype == bool and np.array_equal(got.mask, want.mask)


def assert_same(a, b):
    """Two results of the library, bit for bit."""
    assert summary(a) == summary(b)
    assert np.array_equal(a.per_column, b.per_column)
    assert a.mask_words.tobytes() == b.mask_words.tobytes() and np.array_equal(a.mask, b.mask)


@functools.lru_cache(maxsize=None)
def case(key):
    """(blob, trace, public inputs) of random_air(*key); shared, read-only."""
    out = random_air(*key)
    for a in out:
        a.setflags(write=False)
    return out


def corrupt_one(trace, col):
    """The middle cell of column `col` plus one: a trace that violates the AIR.  The callers pick a boolean column that gates others,
    so that the free cells change with it."""
    bad = trace.copy()
    n = bad.shape[0]
    bad[n // 2, col] = np.uint64((int(bad[n // 2, col]) + 1) % P)
    return bad


@functools.lru_cache(maxsize=None)
def hand_air(n):
    """(blob, trace, public inputs, free rows per column, mask) of a six-column AIR of n rows with known free cells:
    0  x, x' = 3 x + 1 with x[0] and x[n - 1] public: no free cell
    1  b, b (1 - b) = 0: no free cell
    2  u, read by nothing: every cell free
    3  w and 4  v under b (w - v) = 0: free on exactly the rows with b = 0
    5  y, read only as y' = x by a transition constraint: row 0 free and nothing else"""
    rng = np.random.default_rng(1000 + n)
    x = [5]
    for _ in range(n - 1):
        x.append((3 * x[-1] + 1) % P)
    bit = [1 if r % 3 == 0 else 0 for r in range(n)]
    u = [int(v) for v in rng.integers(0, P, size=n, dtype=np.uint64)]
    v = [int(q) for q in rng.integers(0, P, size=n, dtype=np.uint64)]
    w = [v[r] if bit[r] else (v[r] + 1 + r) % P for r in range(n)]
    y = [int(rng.integers(0, P, dtype=np.uint64))] + x[:-1]
    b = AirBuilder(6, 2, 3)
    b.first_row(b.L(0) - b.PI(0))
    b.transition(b.N(0) - b.L(0) * 3 - 1)
    b.last_row(b.L(0) - b.PI(1))
    b.constraint(b.L(1) * (1 - b.L(1)))
    b.constraint(b.L(1) * (b.L(3) - b.L(4)))
    b.transition(b.N(5) - b.L(0))
    trace = np.array([x, bit, u, w, v, y], dtype=np.uint64).T.copy()
    pis = np.array([x[0], x[-1]], dtype=np.uint64)
    mask = np.zeros((n, 6), dtype=bool)
    mask[:, 2] = True
    mask[:, 3] = mask[:, 4] = np.array(bit) == 0
    mask[0, 5] = True
    blob = b.finish()
    for a in (blob, trace, pis, mask):
        a.setflags(write=False)
    return blob, trace, pis, mask.sum(axis=0).astype(np.uint32), mask


def register(blob, rows):
    return S.register_air(blob, default_rows=rows)
