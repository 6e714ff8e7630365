"""starkhip_check_trace_free_cell_classes_replay (csrc/free_cells.cpp) against a brute force of the rule written in Python
(free_cell_classes_util.Expected), against recorded class counts, against starkhip_check_trace_free_cells_replay (its projection), and
on a hand-written AIR whose classes are known by construction; and that brute force against the audit's (free_cells_util.Expected).
No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from free_cell_classes_util import CASES, Expected, assert_classes, assert_nested, assert_same, assert_same_counts, hand_air, summary
from free_cells_util import CPU_CASES, DELTA, P, case, corrupt_one, register
from free_cells_util import Expected as AuditExpected

KEYS = list(CASES)


@functools.lru_cache(maxsize=None)
def expected(key):
    blob, trace, pis = case(key)
    return Expected(blob, trace, pis)


@functools.lru_cache(maxsize=None)
def replayed(key):
    blob, trace, pis = case(key)
    return S.free_cell_classes_replay(register(blob, key[3]), trace, pis)


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_replay_is_the_brute_force_and_the_recorded_counts(key):
    blob, trace, pis = case(key)
    caught, silent, gated, unread, never_open, constraints = CASES[key]
    want = expected(key)
    assert len(want.open_rows) == constraints
    assert (want.summary[1:5], want.summary[6]) == ((caught, silent, gated, unread), never_open)  # the rule as the issue reads it
    if key in CPU_CASES:
        assert silent + gated + unread == CPU_CASES[key][1]
    if key[0] not in (1, 2, 11):
        assert min(caught, silent, gated, unread) > 0  # every class is there: the comparison has teeth
    rows = replayed(key)
    assert_classes(rows, want)
    cols = S.free_cell_classes_replay(register(blob, key[3]), trace.T.copy(), pis, layout=1)
    assert_classes(cols, want)
    assert_same(rows, cols)
    assert_same_counts(S.free_cell_classes_replay(register(blob, key[3]), trace, pis, planes=False), rows)


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_caught_is_the_audits_rule_and_the_free_classes_partition_its_free_cells(key):
    blob, trace, pis = case(key)
    got = replayed(key)
    audit = S.free_cells_replay(register(blob, key[3]), trace, pis)
    assert np.array_equal(got.caught, ~audit.mask)
    live = np.uint64((1 << min(key[3], 64)) - 1)  # the words too: caught and free words are complements on the live rows
    assert ((got.plane_words[2] ^ audit.mask_words) == live).all()
    assert np.array_equal(got.silent | got.gated | got.unread, audit.mask)
    assert got.n_silent + got.n_gated + got.n_unread == audit.free and got.n_caught == audit.cells - audit.free
    assert np.array_equal(got.per_column.sum(axis=1, dtype=np.uint32), audit.per_column)
    assert_nested(got, key[3])


def assert_brute_forces_agree(classes, audit):
    assert np.array_equal(classes.caught, ~audit.mask)
    assert np.array_equal(classes.silent | classes.gated | classes.unread, audit.mask)
    assert np.array_equal(classes.per_column.sum(axis=1, dtype=np.uint32), audit.per_column)


# The library's audit is a projection of its classes, so the test above compares one replay loop with itself.  What keeps the two
# results independent are the two brute forces, written apart and neither touching the library: free_cells_util.Expected evaluates
# the expanded polynomial G * body, free_cell_classes_util.Expected gates and body apart.  Each pins its own replay; this holds them
# to each other.
@pytest.mark.parametrize("key", list(CPU_CASES), ids=str)
def test_the_two_brute_forces_agree(key):
    blob, trace, pis = case(key)
    assert_brute_forces_agree(expected(key), AuditExpected(blob, trace, pis))


@pytest.mark.parametrize("n", (2, 64, 128))
def test_the_two_brute_forces_agree_on_the_hand_written_air(n):
    h = hand_air(n)
    assert_brute_forces_agree(Expected(h.blob, h.trace, h.pis), AuditExpected(h.blob, h.trace, h.pis))


@pytest.mark.parametrize("n", (2, 64, 128))
def test_hand_written_air_has_the_classes_it_was_built_with(n):
    h = hand_air(n)
    assert O.check_trace(h.blob, h.trace, h.pis)[0] == 0
    assert 0 < h.n_off < n and 0 < h.n_s_zero < n
    air = register(h.blob, n)
    for layout, t in ((0, h.trace), (1, h.trace.T.copy())):
        got = S.free_cell_classes_replay(air, t, h.pis, layout=layout)
        assert_classes(got, h)
        assert got.per_column.tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, n], [0, h.n_off, 0], [0, h.n_off, 0], [0, 0, 1], [0, 0, 0],
                                           [h.n_s_zero, 0, 0], [0, 0, 0]]
    assert_classes(got, Expected(h.blob, h.trace, h.pis))
    other = S.free_cell_classes_replay(air, h.trace, h.pis, delta=12345)  # no root of an occurrence here
    assert_classes(other, h)


def test_replay_on_a_trace_that_violates_the_air():
    key = (3, 40, 4, 32)
    blob, trace, pis = case(key)
    bad = corrupt_one(trace, 9)
    assert O.check_trace(blob, bad, pis)[0] > 0
    want = Expected(blob, bad, pis)
    assert not np.array_equal(want.open, expected(key).open) and not np.array_equal(want.open_rows, expected(key).open_rows)
    air = register(blob, key[3])
    assert_classes(S.free_cell_classes_replay(air, bad, pis), want)
    assert_classes(S.free_cell_classes_replay(air, bad.T.copy(), pis, layout=1), want)


def test_cells_at_or_above_p_read_as_their_class():
    key = (12, 20, 4, 64)
    blob, trace, pis = case(key)
    aliased = trace.copy()
    small = aliased < np.uint64((1 << 64) - P)  # c + p still fits a word
    assert small.any() and (aliased == 0).any()
    aliased[small] += np.uint64(P)
    air = register(blob, key[3])
    for layout, t in ((0, aliased), (1, aliased.T.copy())):
        assert_same(S.free_cell_classes_replay(air, t, pis, layout=layout), replayed(key))


def test_merge_is_the_or_of_the_planes():
    key = (3, 40, 4, 32)
    blob, trace, pis = case(key)
    air = register(blob, key[3])
    a, b = replayed(key), S.free_cell_classes_replay(air, corrupt_one(trace, 9), pis)
    assert a.plane_words.tobytes() != b.plane_words.tobytes()
    m = a.merge(b)
    assert m.plane_words.tobytes() == (a.plane_words | b.plane_words).tobytes()
    assert_nested(m, key[3])
    for name in ("read", "open", "caught"):
        assert np.array_equal(getattr(m, name), getattr(a, name) | getattr(b, name))
    assert np.array_equal(m.open_rows, a.open_rows + b.open_rows)
    per = np.stack([m.silent.sum(axis=0), m.gated.sum(axis=0), m.unread.sum(axis=0)], axis=1)
    assert m.per_column.dtype == np.uint32 and np.array_equal(m.per_column, per)
    assert summary(m) == (a.cells, int(m.caught.sum()), int(m.silent.sum()), int(m.gated.sum()), int(m.unread.sum()),
                          int((per[:, 0] > 0).sum()), int((m.open_rows == 0).sum()))
    assert m.n_caught >= max(a.n_caught, b.n_caught) and m.n_unread == a.n_unread  # a cell caught in either trace; `read` is the AIR's
    assert a.merge(a).per_column.tobytes() == a.per_column.tobytes() and summary(a.merge(a))[:6] == summary(a)[:6]
    assert a.merge(a).plane_words.tobytes() == a.plane_words.tobytes() and np.array_equal(a.merge(a).open_rows, 2 * a.open_rows)
    with pytest.raises(S.StarkhipError):
        a.merge(S.free_cell_classes_replay(air, trace, pis, planes=False))
    with pytest.raises(S.StarkhipError):
        a.merge(replayed((12, 20, 4, 64)))


def _raw(air, trace, n_rows, n_cols, pis, delta, per=True, planes=True, opened=True, layout=0, n_constraints=8):
    per_column = np.full((n_cols, 3), 0xFFFFFFFF, dtype=np.uint32)
    words = np.full((3, n_cols, (max(n_rows, 1) + 63) // 64), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    open_rows = np.full(n_constraints, 0xFFFFFFFF, dtype=np.uint32)
    out = S.api._FreeCellClassesStruct()
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = S.lib.starkhip_check_trace_free_cell_classes_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, pis.ctypes.data_as(u64p),
                                                             delta, per_column.ctypes.data_as(u32p) if per else None,
                                                             words.ctypes.data_as(u64p) if planes else None,
                                                             open_rows.ctypes.data_as(u32p) if opened else None, C.byref(out))
    return rc, per_column, words, open_rows, tuple(getattr(out, name) for name, _ in S.api._FreeCellClassesStruct._fields_)


def test_arguments():
    h = hand_air(2)
    trace, pis = h.trace.copy(), h.pis.copy()
    air = register(h.blob, 2)
    for delta in (0, P, P + 5, (1 << 64) - 1):
        assert _raw(air, trace, 2, 9, pis, delta)[0] == S.ERR_BAD_SHAPE
        with pytest.raises(S.StarkhipError) as e:
            S.free_cell_classes_replay(air, trace, pis, delta=delta)
        assert e.value.code == S.ERR_BAD_SHAPE
    rc, per, words, opened, out = _raw(air, trace, 2, 9, pis, P - 2)
    assert rc == 0 and np.array_equal(per, h.per_column) and np.array_equal(opened, h.open_rows) and out == h.summary
    # n = 2: one word per column and plane, and only its two low bits can be set
    assert words.shape == (3, 9, 1) and not (words >> np.uint64(2)).any()
    for plane, mask in enumerate((h.read, h.open, h.caught)):
        assert [[bool(int(w) >> r & 1) for w in words[plane, :, 0]] for r in range(2)] == mask.tolist()
    for per_on, planes_on, open_on in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):  # NULL results
        rc, per2, words2, opened2, out2 = _raw(air, trace, 2, 9, pis, P - 2, per=per_on, planes=planes_on, opened=open_on)
        assert rc == 0 and out2 == out
        assert np.array_equal(per2, per) if per_on else (per2 == 0xFFFFFFFF).all()
        assert np.array_equal(words2, words) if planes_on else (words2 == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
        assert np.array_equal(opened2, opened) if open_on else (opened2 == 0xFFFFFFFF).all()
    # shapes are check_trace's: the column count, a power of two from 2 on, the layout, canonical public inputs; and a NULL `out`
    assert _raw(air, trace, 2, 8, pis, DELTA)[0] == S.ERR_BAD_SHAPE
    big = np.zeros((6, 9), dtype=np.uint64)
    for n_rows in (0, 1, 3, 6):
        assert _raw(air, big, n_rows, 9, pis, DELTA)[0] == S.ERR_BAD_SHAPE
    assert _raw(air, trace, 2, 9, pis, DELTA, layout=2)[0] == S.ERR_BAD_SHAPE
    assert _raw(air, trace, 2, 9, np.array([P, 0], dtype=np.uint64), DELTA)[0] == S.ERR_BAD_SHAPE
    assert _raw(S.AIR_CUSTOM_BASE + 100000, trace, 2, 9, pis, DELTA)[0] == S.ERR_BAD_AIR
    u64p = C.POINTER(C.c_uint64)
    assert S.lib.starkhip_check_trace_free_cell_classes_replay(air, trace.ctypes.data_as(C.c_void_p), 2, 9, 0, pis.ctypes.data_as(u64p), DELTA, None,
                                                               None, None, None) == S.ERR_BAD_SHAPE
    with pytest.raises(S.StarkhipError):
        S.free_cell_classes_replay(air, trace[:, :8], pis)
    with pytest.raises(S.StarkhipError):
        S.free_cell_classes_replay(air, trace, pis[:1])
    # a device entry without a context is refused before anything is read
    assert S.lib.starkhip_check_trace_free_cell_classes(None, air, trace.ctypes.data_as(C.c_void_p), 2, 9, 0, 0, pis.ctypes.data_as(u64p), DELTA, None,
                                                        None, None, C.byref(S.api._FreeCellClassesStruct())) == S.ERR_NO_DEVICE
