"""Traces with cells at or above p, for the tests of the rule that every entry reading a trace reads a 64-bit word w as the field
element w mod p (include/starkhip.h): the cells 0 .. 2^32 - 2 are the only ones with a second 64-bit representative, c + p, so random
traces never hold one.  Here: `alias` (c -> c + p on a seeded share of the small cells), the edge values, a hand-written AIR whose
program holds every kind of term and gate the evaluators tell apart with a trace filler for it, a small AIR with one complemented
gate, and the rows on which a device walker that subtracts raw words calls a violated constraint satisfied.  Test code."""
import functools

import numpy as np

from starky_bls12_381_amd.air_builder import AirBuilder

P = 0xFFFFFFFF00000001
SMALL_MAX = (1 << 32) - 2  # the largest cell with an alias: SMALL_MAX + P = 2^64 - 1
EDGES = (0, 1, 2, 3, 0xFFFF, 1 << 31, (1 << 32) - 3, SMALL_MAX)
EDGES_ALIASED = tuple(e + P for e in EDGES)
assert EDGES_ALIASED[-1] == (1 << 64) - 1
ALL_SMALL_FLOOR, HAND_FLOOR = 0.5, 0.25  # the least share of words >= p at share 1.0: traces of small cells only / the hand-written AIR


def alias(trace, share, seed):
    """(a copy of `trace` with p added to a seeded `share` of its cells <= 2^32 - 2, the number of cells that got it)."""
    t = np.array(trace, dtype=np.uint64, copy=True)
    pick = (t <= np.uint64(SMALL_MAX)) & (np.random.default_rng(seed).random(t.shape) < share)
    t[pick] += np.uint64(P)
    return t, int(pick.sum())


def assert_aliased(aliased, canonical, floor, share=1.0, count=None):
    """What every test asserts of its inputs before it uses them: the aliased trace is the canonical one mod p, and at least `floor` of
    its words are >= p, so that no test passes by aliasing nothing.  The floors are stated for a trace aliased in full; a test that
    asks `alias` for a smaller share scales the floor by it, less the four standard deviations the seeded draw may fall short by."""
    aliased, canonical = np.asarray(aliased, dtype=np.uint64), np.asarray(canonical, dtype=np.uint64)
    assert aliased.shape == canonical.shape and np.array_equal(aliased % np.uint64(P), canonical)
    assert not (canonical >= np.uint64(P)).any()
    above = int((aliased >= np.uint64(P)).sum())
    if count is not None:
        assert above == count
    cells = aliased.size
    need = floor * cells if share >= 1.0 else floor * (share * cells - 4.0 * np.sqrt(share * (1.0 - share) * cells))
    assert above >= need and above > 0, (above, cells, share)


def canonical(trace):
    return np.asarray(trace, dtype=np.uint64) % np.uint64(P)


# ---------------------------------------------------------------- the hand-written AIR
N_COLS, N_PIS, DEGREE = 17, 4, 3
FREE_COLS = (0, 1, 3, 4, 5, 6, 7)  # edge values; the other columns follow from them
K_COEF = 0x123456789ABCDEF
PI0, PI1 = 0xFFFE, 5


@functools.lru_cache(maxsize=None)
def hand_blob():
    """Columns 0, 1, 3 .. 7 are free, the others are what the constraints make of them:
    k 0 .. 5   L1 - L0 + L2 in its six term orders (column 2 = L0 - L1)
    k 6        K L3 - L8: a single cell under a constant coefficient
    k 7, 8     L9 - L3 - PI0 and PI1 - L10 + L4: a public input under either sign
    k 9, 10    L3 L4 - L11 and L3 L4 L5 - L12: products of two and of three cells
    k 11       (1 - L7) (L5 - L13): a complemented gate, whose cell holds edge values, not bits
    k 12       L6 (L4 - L14): a plain gate, likewise
    k 13, 14   transitions N15 - L15 - L0 (a running sum) and N1 L5 - L16 (a next-row cell inside a product)
    k 15, 16   first row L15 = PI2, last row L15 = PI3"""
    b = AirBuilder(N_COLS, N_PIS, DEGREE)
    L, N = b.L, b.N
    b.constraint(L(1) - L(0) + L(2))
    b.constraint(L(1) + L(2) - L(0))
    b.constraint(-L(0) + L(1) + L(2))
    b.constraint(-L(0) + L(2) + L(1))
    b.constraint(L(2) + L(1) - L(0))
    b.constraint(L(2) - L(0) + L(1))
    b.constraint(L(3) * K_COEF - L(8))
    b.constraint(L(9) - L(3) - b.PI(0))
    b.constraint(b.PI(1) - L(10) + L(4))
    b.constraint(L(3) * L(4) - L(11))
    b.constraint(L(3) * L(4) * L(5) - L(12))
    b.constraint((1 - L(7)) * (L(5) - L(13)))
    b.constraint(L(6) * (L(4) - L(14)))
    b.transition(N(15) - L(15) - L(0))
    b.transition(N(1) * L(5) - L(16))
    b.first_row(L(15) - b.PI(2))
    b.last_row(L(15) - b.PI(3))
    assert b.count() == 17
    blob = b.finish()
    blob.setflags(write=False)
    return blob


@functools.lru_cache(maxsize=None)
def hand_trace(n):
    """(row-major trace, public inputs) of n rows satisfying hand_blob(): edge values in the free columns, every edge in each and
    the gates open and shut on different rows; shared, read-only."""
    rng = np.random.default_rng(7000 + n)
    t = [[0] * N_COLS for _ in range(n)]
    for c in FREE_COLS:
        picks = list(rng.permutation(len(EDGES))) + list(rng.integers(0, len(EDGES), size=max(0, n - len(EDGES))))
        for r in range(n):
            t[r][c] = EDGES[int(picks[r])]
    junk = [EDGES[int(x)] for x in rng.integers(0, len(EDGES), size=3 * n)]
    run = 3
    for r in range(n):
        x = t[r]
        x[2] = (x[0] - x[1]) % P
        x[8] = K_COEF * x[3] % P
        x[9] = (x[3] + PI0) % P
        x[10] = (PI1 + x[4]) % P
        x[11] = x[3] * x[4] % P
        x[12] = x[11] * x[5] % P
        x[13] = x[5] if x[7] != 1 else junk[3 * r]      # (1 - L7) = 0: the body is free
        x[14] = x[4] if x[6] != 0 else junk[3 * r + 1]  # L6 = 0 likewise
        x[15] = run
        run = (run + x[0]) % P
        x[16] = t[r + 1][1] * x[5] % P if r + 1 < n else junk[3 * r + 2]
    assert any(x[7] == 1 for x in t) and any(x[6] == 0 for x in t)
    trace = np.array(t, dtype=np.uint64)
    pis = np.array([PI0, PI1, t[0][15], t[n - 1][15]], dtype=np.uint64)
    trace.setflags(write=False)
    pis.setflags(write=False)
    return trace, pis


@functools.lru_cache(maxsize=None)
def hand_violating(n):
    """hand_trace(n) with cells raised by one: row n // 2 whole, columns 0 (every sum and the running sum) and 7 (the complemented
    gate's cell) on every third row, and the last row's running sum.  Small cells stay small, so they still have an alias."""
    trace, pis = hand_trace(n)
    bad = trace.copy()
    bump = lambda x: (x + np.uint64(1)) % np.uint64(P)  # noqa: E731  (no cell is 2^64 - 1 here: the trace is canonical)
    bad[n // 2] = bump(bad[n // 2])
    bad[::3, 0] = bump(bad[::3, 0])
    bad[1::3, 7] = bump(bad[1::3, 7])
    bad[n - 1, 15] = bump(bad[n - 1, 15])
    bad.setflags(write=False)
    return bad, pis


# ---------------------------------------------------------------- one complemented gate
GATE_CELLS = (2, 3, 77, SMALL_MAX)


@functools.lru_cache(maxsize=None)
def gate_blob():
    """(1 - L0) (L1^2 - L1)"""
    b = AirBuilder(2, 0, 3)
    b.constraint((1 - b.L(0)) * (b.L(1) * b.L(1) - b.L(1)))
    blob = b.finish()
    blob.setflags(write=False)
    return blob


def gate_trace(cell, n=8):
    """L0 = cell, L1 = 5 on every row: the constraint is (1 - cell) 20 there."""
    t = np.empty((n, 2), dtype=np.uint64)
    t[:, 0], t[:, 1] = cell, 5
    return t


# ---------------------------------------------------------------- rows a raw subtraction calls clean
@functools.lru_cache(maxsize=None)
def directed_blob():
    """L1 - L0 + L2 and the same constraint as -L0 + L1 + L2"""
    b = AirBuilder(3, 0, 2)
    b.constraint(b.L(1) - b.L(0) + b.L(2))
    b.constraint(-b.L(0) + b.L(1) + b.L(2))
    blob = b.finish()
    blob.setflags(write=False)
    return blob


DIRECTED_VALUE = P - (1 << 32) + 1  # 3 - 5 + (p - 2^32 + 3)


def directed_traces(n=8):
    """(aliased, canonical) rows L0 = p + 5, L1 = 3, L2 = p - 2^32 + 3.  Both constraints are p - 2^32 + 1 on every row, but a walker
    that subtracts the raw word p + 5 from 3 reaches 2^64 - 2, and the sum with L2 is then exactly p: zero."""
    a = np.empty((n, 3), dtype=np.uint64)
    a[:, 0], a[:, 1], a[:, 2] = P + 5, 3, P - (1 << 32) + 3
    return a, canonical(a)
