"""starkhip_check_trace_free_cells_replay (csrc/free_cells.cpp) against a brute force of the rule written in Python
(free_cells_util.Expected), against the CPU oracle's checker on every changed trace, and on a hand-written AIR whose free cells are
known by construction.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from free_cells_util import CPU_CASES, DELTA, P, Expected, assert_free_cells, assert_same, case, corrupt_one, hand_air, register, summary

KEYS = list(CPU_CASES)


@functools.lru_cache(maxsize=None)
def expected(key):
    blob, trace, pis = case(key)
    return Expected(blob, trace, pis)


def test_default_delta_is_the_documented_constant():
    assert S.DEFAULT_DELTA == DELTA and 0 < DELTA < P


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_replay_is_the_brute_force(key):
    blob, trace, pis = case(key)
    want = expected(key)
    assert want.summary == CPU_CASES[key]  # the inputs are the ones the counts were recorded for, and not degenerate
    air = register(blob, key[3])
    rows = S.free_cells_replay(air, trace, pis)
    assert_free_cells(rows, want)
    cols = S.free_cells_replay(air, trace.T.copy(), pis, layout=1)
    assert_free_cells(cols, want)
    assert_same(rows, cols)
    assert rows.mask_words.shape == (key[1], (key[3] + 63) // 64)


def test_replay_on_a_trace_that_violates_the_air():
    key = (3, 40, 4, 32)
    blob, trace, pis = case(key)
    bad = corrupt_one(trace, 9)
    assert O.check_trace(blob, bad, pis)[0] > 0
    want = Expected(blob, bad, pis)
    assert not np.array_equal(want.mask, expected(key).mask)
    air = register(blob, key[3])
    assert_free_cells(S.free_cells_replay(air, bad, pis), want)
    assert_free_cells(S.free_cells_replay(air, bad.T.copy(), pis, layout=1), want)


@pytest.mark.parametrize("key", KEYS[:3], ids=str)
def test_a_cell_is_free_exactly_when_the_oracle_accepts_the_changed_trace(key):
    blob, trace, pis = case(key)
    assert O.check_trace(blob, trace, pis)[0] == 0
    got = S.free_cells_replay(register(blob, key[3]), trace, pis)
    n, n_cols = trace.shape
    for r in range(n):
        for c in range(n_cols):
            changed = trace.copy()
            changed[r, c] = np.uint64((int(changed[r, c]) + DELTA) % P)
            assert (O.check_trace(blob, changed, pis)[0] == 0) == bool(got.mask[r, c]), (r, c)


@pytest.mark.parametrize("n", (2, 64, 128))
def test_hand_written_air_has_the_free_cells_it_was_built_with(n):
    blob, trace, pis, per_column, mask = hand_air(n)
    assert O.check_trace(blob, trace, pis)[0] == 0
    bits = int((trace[:, 1] == 0).sum())
    assert 0 < bits < n and per_column.tolist() == [0, 0, n, bits, bits, 1]
    air = register(blob, n)
    for layout, t in ((0, trace), (1, trace.T.copy())):
        got = S.free_cells_replay(air, t, pis, layout=layout)
        assert np.array_equal(got.per_column, per_column) and np.array_equal(got.mask, mask)
        assert summary(got) == (6 * n, n + 2 * bits + 1, 1, 3)
    assert_free_cells(got, Expected(blob, trace, pis))
    other = S.free_cells_replay(air, trace, pis, delta=12345)  # no root of a constraint here: -b, 1 - b, v - w are none of the two
    assert np.array_equal(other.mask, mask)


def _raw(air, trace, n_rows, n_cols, pis, delta, per=True, mask=True, layout=0):
    per_column = np.full(n_cols, 0xFFFFFFFF, dtype=np.uint32)
    words = np.full((n_cols, (max(n_rows, 1) + 63) // 64), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    out = S.api._FreeCellsStruct()
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rc = S.lib.starkhip_check_trace_free_cells_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, pis.ctypes.data_as(u64p), delta,
                                                      per_column.ctypes.data_as(u32p) if per else None, words.ctypes.data_as(u64p) if mask else None,
                                                      C.byref(out))
    return rc, per_column, words, out


def test_arguments():
    blob, trace, pis, per_column, mask = hand_air(2)
    trace, pis = trace.copy(), pis.copy()
    air = register(blob, 2)
    for delta in (0, P, P + 5, (1 << 64) - 1):
        assert _raw(air, trace, 2, 6, pis, delta)[0] == S.ERR_BAD_SHAPE
        with pytest.raises(S.StarkhipError) as e:
            S.free_cells_replay(air, trace, pis, delta=delta)
        assert e.value.code == S.ERR_BAD_SHAPE
    rc, per, words, out = _raw(air, trace, 2, 6, pis, P - 2)
    assert rc == 0 and np.array_equal(per, per_column)
    # n = 2: one word per column, and only its two low bits can be set
    assert words.shape == (6, 1) and all(int(w) >> 2 == 0 for w in words[:, 0])
    assert [[bool(int(w) >> r & 1) for w in words[:, 0]] for r in range(2)] == mask.tolist()
    want = (out.cells, out.free_cells, out.free_columns, out.partly_free_columns)
    assert want == (12, int(mask.sum()), 1, 3)
    for per_on, mask_on in ((False, True), (True, False), (False, False)):  # NULL per_column, NULL free_mask
        rc, per, words2, out = _raw(air, trace, 2, 6, pis, P - 2, per=per_on, mask=mask_on)
        assert rc == 0 and (out.cells, out.free_cells, out.free_columns, out.partly_free_columns) == want
        assert np.array_equal(per, per_column) if per_on else (per == 0xFFFFFFFF).all()
        assert np.array_equal(words2, words) if mask_on else (words2 == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    assert S.free_cells_replay(air, trace, pis, mask=False).mask is None
    # shapes are check_trace's: the column count, a power of two from 2 on, the layout, canonical public inputs
    assert _raw(air, trace, 2, 5, pis, DELTA)[0] == S.ERR_BAD_SHAPE
    big = np.zeros((6, 6), dtype=np.uint64)
    for n_rows in (0, 1, 3, 6):
        assert _raw(air, big, n_rows, 6, pis, DELTA)[0] == S.ERR_BAD_SHAPE
        assert S.lib.starkhip_check_trace_report_replay(air, big.ctypes.data_as(C.c_void_p), n_rows, 6, 0, pis.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                        None, None, None, 0, C.byref(S.api._CheckReportStruct())) == S.ERR_BAD_SHAPE
    assert _raw(air, trace, 2, 6, pis, DELTA, layout=2)[0] == S.ERR_BAD_SHAPE
    assert _raw(air, trace, 2, 6, np.array([P, 0], dtype=np.uint64), DELTA)[0] == S.ERR_BAD_SHAPE
    assert _raw(S.AIR_CUSTOM_BASE + 100000, trace, 2, 6, pis, DELTA)[0] == S.ERR_BAD_AIR
    with pytest.raises(S.StarkhipError):
        S.free_cells_replay(air, trace[:, :5], pis)
    with pytest.raises(S.StarkhipError):
        S.free_cells_replay(air, trace, pis[:1])
    # a device entry without a context is refused before anything is read
    assert S.lib.starkhip_check_trace_free_cells(None, air, trace.ctypes.data_as(C.c_void_p), 2, 6, 0, 0, pis.ctypes.data_as(C.POINTER(C.c_uint64)), DELTA,
                                                 None, None, C.byref(S.api._FreeCellsStruct())) == S.ERR_NO_DEVICE
