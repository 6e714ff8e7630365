"""What starkhip_check_trace_free_cell_classes must say about a trace: a brute force of its rule in plain Python from the program blob
(air_blob; gates and body evaluated apart), a hand-written AIR whose classes are known by construction, and the comparisons the
CPU and GPU tests share.  Test code."""
import functools

import numpy as np

import air_blob
from free_cells_util import DELTA, P, applies
from starky_bls12_381_amd.air_builder import AirBuilder

# random_air (seed, columns, degree, rows) with, per case, (caught, silent, gated, unread, constraints never open, constraints) at
# DELTA: from a brute force of the rule that was written apart from the one below and from the library
CASES = {(1, 1, 2, 8): (1, 0, 0, 7, 0, 1), (2, 7, 3, 16): (95, 0, 1, 16, 1, 10), (3, 40, 4, 32): (874, 19, 39, 348, 2, 51),
         (4, 64, 5, 64): (3003, 133, 322, 638, 2, 73), (5, 65, 3, 128): (6182, 134, 599, 1405, 6, 76), (11, 12, 3, 2): (17, 0, 0, 7, 0, 9),
         (12, 20, 4, 64): (841, 106, 82, 251, 3, 20), (6, 130, 5, 256): (23180, 739, 3730, 5631, 14, 149)}


def gate_product(gates, local, nxt):
    g = 1
    for ref in gates:
        x = (nxt if ref & air_blob.REF_NEXT else local)[ref & air_blob.COL_MASK]
        g = g * ((1 - x) % P if ref & air_blob.REF_COMPL else x) % P
    return g


class Expected:
    """The rule, occurrence by occurrence: read, open, caught as bool [n, C], open_rows per constraint, and what follows from them."""

    def __init__(self, blob, trace, pis, delta=DELTA):
        n, n_cols = trace.shape
        rows = [[int(x) % P for x in row] for row in trace]
        pis = [int(x) for x in pis]
        self.read, self.open, self.caught = (np.zeros((n, n_cols), dtype=bool) for _ in range(3))
        open_rows = []
        for kind, gates, terms in air_blob.constraints(air_blob.parse_blob(blob)):
            body = air_blob.expand([], terms)  # the body alone: the gates stay a product of their own
            open_rows.append(sum(1 for r in range(n) if applies(kind, r, n) and gate_product(gates, rows[r], rows[(r + 1) % n]) != 0))
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
                    local, nxt = (local, changed) if as_next else (changed, nxt)
                    g = gate_product(gates, local, nxt)
                    self.read[r, col] = True
                    if g != 0:
                        self.open[r, col] = True
                    if g * air_blob.evaluate(body, local, nxt, pis) % P != 0:
                        self.caught[r, col] = True
        self.open_rows = np.array(open_rows, dtype=np.uint32)
        self.silent, self.gated, self.unread = self.open & ~self.caught, self.read & ~self.open, ~self.read
        self.per_column = np.stack([m.sum(axis=0) for m in (self.silent, self.gated, self.unread)], axis=1).astype(np.uint32)
        self.summary = (n * n_cols, int(self.caught.sum()), int(self.silent.sum()), int(self.gated.sum()), int(self.unread.sum()),
                        int((self.per_column[:, 0] > 0).sum()), int((self.open_rows == 0).sum()))


def summary(fc):
    return (fc.cells, fc.n_caught, fc.n_silent, fc.n_gated, fc.n_unread, fc.silent_columns, fc.constraints_never_open)


def assert_nested(fc, n):
    """read contains open contains caught, the classes partition the cells, and no bit at or beyond row n is set."""
    rd, op, ca = (fc.plane_words[i] for i in range(3))
    assert not (op & ~rd).any() and not (ca & ~op).any()
    assert (fc.caught | fc.silent | fc.gated | fc.unread).all()
    assert int(fc.caught.sum()) + int(fc.silent.sum()) + int(fc.gated.sum()) + int(fc.unread.sum()) == fc.cells == fc.read.size
    if n % 64:
        assert not (fc.plane_words[:, :, -1] >> np.uint64(n % 64)).any()


def assert_classes(got, want):
    """A result of the library against the brute force or a construction: planes, counts, summary."""
    n = want.read.shape[0]
    assert got.plane_words.dtype == np.uint64 and got.plane_words.shape == (3, want.read.shape[1], (n + 63) // 64)
    for name in ("read", "open", "caught", "silent", "gated", "unread"):
        assert getattr(got, name).dtype == bool and np.array_equal(getattr(got, name), getattr(want, name)), name
    assert got.per_column.dtype == np.uint32 and np.array_equal(got.per_column, want.per_column)
    assert got.open_rows.dtype == np.uint32 and np.array_equal(got.open_rows, want.open_rows)
    assert summary(got) == want.summary
    assert_nested(got, n)


def assert_same(a, b):
    """Two results of the library, bit for bit."""
    assert summary(a) == summary(b)
    assert a.per_column.tobytes() == b.per_column.tobytes() and a.open_rows.tobytes() == b.open_rows.tobytes()
    assert a.plane_words.tobytes() == b.plane_words.tobytes()


def assert_same_counts(bare, full):
    """A result without planes against one with."""
    assert bare.plane_words is None and bare.read is None and bare.silent is None
    assert summary(bare) == summary(full)
    assert np.array_equal(bare.per_column, full.per_column) and np.array_equal(bare.open_rows, full.open_rows)


class HandAir:
    pass


@functools.lru_cache(maxsize=None)
def hand_air(n):
    """A nine-column AIR of n rows whose classes are known by construction: free_cells_util.hand_air, a product constraint with a
    zero co-factor, and a first-row constraint whose gate is shut on row 0.
    0  x, x' = 3 x + 1 with x[0] and x[n - 1] public: caught
    1  b, b (1 - b) = 0: caught
    2  u, read by nothing: unread
    3  w and 4  v under b (w - v) = 0: caught where b = 1, gated where b = 0
    5  y, read only as y' = x by a transition constraint: row 0 unread, the rest caught
    6  s, 7  t, 8  z under z - s t = 0, t nonzero and read by nothing else: s and z caught, t silent exactly where s = 0
    and (1 - b) (x - PI0) = 0 on the first row, where b = 1: the one constraint that is never open.
    Returns an object with blob, trace, pis, the masks read / open / caught / silent / gated / unread, per_column, open_rows, summary."""
    rng = np.random.default_rng(2000 + n)
    x = [5]
    for _ in range(n - 1):
        x.append((3 * x[-1] + 1) % P)
    bit = [1 if r % 3 == 0 else 0 for r in range(n)]
    u = [int(q) for q in rng.integers(0, P, size=n, dtype=np.uint64)]
    v = [int(q) for q in rng.integers(0, P, size=n, dtype=np.uint64)]
    w = [v[r] if bit[r] else (v[r] + 1 + r) % P for r in range(n)]
    y = [int(rng.integers(0, P, dtype=np.uint64))] + x[:-1]
    s = [0 if r % 5 in (1, 2) else 7 + r for r in range(n)]  # n = 2: row 1 zero, row 0 not
    t = [int(q) for q in rng.integers(1, P, size=n, dtype=np.uint64)]
    z = [s[r] * t[r] % P for r in range(n)]
    b = AirBuilder(9, 2, 3)
    b.first_row(b.L(0) - b.PI(0))
    b.transition(b.N(0) - b.L(0) * 3 - 1)
    b.last_row(b.L(0) - b.PI(1))
    b.constraint(b.L(1) * (1 - b.L(1)))
    b.constraint(b.L(1) * (b.L(3) - b.L(4)))
    b.transition(b.N(5) - b.L(0))
    b.constraint(b.L(8) - b.L(6) * b.L(7))
    b.first_row((1 - b.L(1)) * (b.L(0) - b.PI(0)))
    h = HandAir()
    h.blob = b.finish()
    h.trace = np.array([x, bit, u, w, v, y, s, t, z], dtype=np.uint64).T.copy()
    h.pis = np.array([x[0], x[-1]], dtype=np.uint64)
    off, s_zero = np.array(bit) == 0, np.array(s) == 0
    h.read = np.ones((n, 9), dtype=bool)
    h.read[:, 2] = False
    h.read[0, 5] = False
    h.open = h.read.copy()
    h.open[off, 3] = h.open[off, 4] = False
    h.caught = h.open.copy()
    h.caught[s_zero, 7] = False
    h.silent, h.gated, h.unread = h.open & ~h.caught, h.read & ~h.open, ~h.read
    h.per_column = np.stack([m.sum(axis=0) for m in (h.silent, h.gated, h.unread)], axis=1).astype(np.uint32)
    # x first / transition / last, b (1 - b) on the rows with b = 1, b (w - v) likewise, y' = x, z = s t, and the shut first-row one
    ones = int(sum(bit))
    h.open_rows = np.array([1, n - 1, 1, ones, ones, n - 1, n, 0], dtype=np.uint32)
    h.n_off, h.n_s_zero = int(off.sum()), int(s_zero.sum())
    h.summary = (9 * n, 9 * n - h.n_s_zero - 2 * h.n_off - n - 1, h.n_s_zero, 2 * h.n_off, n + 1, 1, 1)
    for a in (h.blob, h.trace, h.pis, h.read, h.open, h.caught, h.silent, h.gated, h.unread, h.per_column, h.open_rows):
        a.setflags(write=False)
    return h
