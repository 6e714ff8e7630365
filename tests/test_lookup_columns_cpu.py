"""starkhip_lookup_columns_replay -- the host driver of starkhip_lookup_columns over host loops -- against the Python reference of the
rule (lookup_ref.py), the refusals of both entries, AirBuilder.lookup in its two languages, and the Rust declarations.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import alias_util as A
import lookup_ref as R
import starky_bls12_381_amd as S
from starky_bls12_381_amd.air_builder import AirBuilder

P = R.P
SIZES = (2, 4, 64, 1024)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _replay(trace, lookups, layout, cap):
    return S.lookup_columns_replay(trace, lookups, layout=layout, cap=cap)


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_data_cases(n, layout):
    for name, (a, t) in R.data_cases(n, seed=n).items():
        trace = R.one_lookup_trace(a, t, seed=n, layout=layout)
        got, rep = R.run(_replay, trace, [R.LOOKUP], layout)
        assert rep.failed == 0 and rep.timings is None, name
        cols = got.T if layout == 0 else got
        if name == "all_equal":
            assert (cols[2] == n // 2).all() and cols[3][0] == n // 2
        if name == "permutation":
            assert np.array_equal(cols[2], cols[3])


@pytest.mark.parametrize("n", SIZES)
def test_cells_at_or_above_p_give_the_canonical_columns(n):
    a, t = R.data_cases(n, seed=3)["range"]
    trace = R.one_lookup_trace(a, t, seed=1)
    aliased, count = A.alias(trace, 1.0, seed=n)
    aliased[:, 2:] = trace[:, 2:]  # only the lookup's own cells
    A.assert_aliased(aliased[:, :2], trace[:, :2], A.ALL_SMALL_FLOOR)
    got, _ = R.run(_replay, aliased, [R.LOOKUP])
    plain, _ = R.run(_replay, trace, [R.LOOKUP])
    assert np.array_equal(got[:, 2:4], plain[:, 2:4]) and not (got[:, 2:4] >= np.uint64(P)).any()
    assert np.array_equal(got[:, :2], aliased[:, :2])  # the inputs keep their representatives


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_two_lookups_share_one_table(n, layout):
    trace = R.shared_table_trace(n, seed=n, layout=layout)
    _, rep = R.run(_replay, trace, R.SHARED, layout)
    assert rep.lookups == 2 and rep.failed == 0


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_a_failing_lookup_keeps_its_columns_beside_one_that_holds(n, layout):
    trace = R.shared_table_trace(n, seed=n + 1, fail_first=True, layout=layout)
    got, rep = R.run(_replay, trace, R.SHARED, layout)
    cols, before = (got.T, trace.T) if layout == 0 else (got, trace)
    assert rep.failed == 1 and rep.per_lookup.tolist() == [2, 0] and rep.list.tolist() == [[0, 0], [0, n - 1]]
    assert np.array_equal(cols[3:5], before[3:5])  # the prior bytes
    assert not np.array_equal(cols[5], before[5]) and not np.array_equal(cols[6], before[6])


@pytest.mark.parametrize("n", SIZES)
def test_missing_rows(n):
    for name, (a, t, rows) in R.missing_cases(n, seed=n).items():
        trace = R.one_lookup_trace(a, t, seed=2)
        got, rep = R.run(_replay, trace, [R.LOOKUP], cap=2048)
        assert rep.failed == 1 and rep.list[:, 1].tolist() == rows, name
        assert np.array_equal(got, trace), name


def test_a_short_cap_keeps_the_lowest_entries():
    n = 64
    trace = R.shared_table_trace(n, seed=5)
    trace[:, 0] = 1000 + np.arange(n, dtype=np.uint64)  # every row of lookup 0 ...
    trace[[3, 40], 1] = 2000  # ... and two of lookup 1
    for cap in (0, 1, 63, 64, 65, 66, 100):
        _, rep = R.run(_replay, trace, R.SHARED, cap=cap)
        assert rep.missing_rows == n + 2 and len(rep.list) == min(cap, n + 2)
    assert rep.list[-2:].tolist() == [[1, 3], [1, 40]]


def test_masks_have_no_bits_at_or_beyond_n_rows():
    for n in (2, 4, 64):
        a, t, _ = R.missing_cases(n, seed=1)["every_row"]
        rep = _replay(R.one_lookup_trace(a, t), [R.LOOKUP], 0, 0)
        assert rep.mask_words.tolist() == [[(1 << n) - 1 if n < 64 else (1 << 64) - 1]]


def _raw(trace, n_rows, n_cols, lookups=(R.LOOKUP,), n_lookups=None, layout=0, cap=4, with_list=True, with_out=True, with_lookups=True, device=False):
    arr, nl = S.api._lookup_array(lookups)
    lst = np.zeros((16, 2), dtype=np.uint64)
    out = S.api._LookupReportStruct()
    tail = (arr if with_lookups else None, nl if n_lookups is None else n_lookups, None, None,
            lst.ctypes.data_as(C.POINTER(C.c_uint64)) if with_list else None, cap, C.byref(out) if with_out else None)
    ptr = trace.ctypes.data_as(C.c_void_p) if trace is not None else None
    if device:
        return S.lib.starkhip_lookup_columns(C.c_void_p(), ptr, n_rows, n_cols, layout, 0, *tail)
    return S.lib.starkhip_lookup_columns_replay(ptr, n_rows, n_cols, layout, *tail)


def test_what_the_entries_refuse():
    n = 32
    trace = R.shared_table_trace(n, seed=1)
    assert _raw(trace.copy(), n, 8, R.SHARED) == 0
    assert _raw(trace.copy(), n, 8, R.SHARED, cap=0, with_list=False) == 0
    bad = [
        dict(lookups=[(8, 2, 3, 4)]), dict(lookups=[(0, 8, 3, 4)]), dict(lookups=[(0, 2, 8, 4)]), dict(lookups=[(0, 2, 3, 8)]),  # a column >= n_cols
        dict(lookups=[(0, 2, 3, 1 << 31)]),
        dict(lookups=[]), dict(lookups=[(0, 2, 3, 4)] * 65), dict(n_lookups=0), dict(with_lookups=False),  # how many lookups
        dict(lookups=[(0, 2, 0, 4)]), dict(lookups=[(0, 2, 3, 2)]), dict(lookups=[(0, 2, 3, 3)]),  # an output that is its own input, table, twin
        dict(lookups=[(0, 2, 3, 4), (1, 2, 5, 0)]), dict(lookups=[(0, 2, 1, 4), (1, 2, 5, 6)]),  # ... another lookup's input
        dict(lookups=[(0, 7, 3, 4), (1, 2, 7, 6)]), dict(lookups=[(0, 2, 3, 7), (1, 7, 5, 6)]),  # ... another lookup's table
        dict(lookups=[(0, 2, 3, 4), (1, 2, 3, 6)]), dict(lookups=[(0, 2, 3, 4), (1, 2, 5, 3)]), dict(lookups=[(0, 2, 3, 4), (0, 2, 3, 4)]),
        dict(n_rows=0), dict(n_rows=1), dict(n_rows=3), dict(n_rows=24), dict(n_rows=1 << 21),  # rows outside the limits
        dict(trace=None), dict(layout=2), dict(layout=-1), dict(n_cols=0),
        dict(cap=S.CHECK_LIST_MAX + 1), dict(cap=1, with_list=False), dict(with_out=False),
    ]
    for kw in bad:
        args = dict(trace=trace.copy(), n_rows=n, n_cols=8, lookups=R.SHARED)
        args.update(kw)
        before = None if args["trace"] is None else args["trace"].copy()
        assert _raw(**args) == S.ERR_BAD_SHAPE, kw
        assert before is None or np.array_equal(before, args["trace"]), kw
    # as many lookups as fit: 64 inputs sharing one table
    wide = np.zeros((4, 1 + 3 * 64), dtype=np.uint64)
    assert _raw(wide, 4, wide.shape[1], [(1 + q, 0, 65 + 2 * q, 66 + 2 * q) for q in range(64)]) == 0
    for call in (lambda: S.lookup_columns_replay(trace.copy(), []), lambda: S.lookup_columns_replay(trace.copy(), R.SHARED, cap=S.CHECK_LIST_MAX + 1),
                 lambda: S.lookup_columns_replay(trace[:, ::2], R.SHARED), lambda: S.lookup_columns_replay(trace.astype(np.int64), R.SHARED)):
        with pytest.raises(S.StarkhipError) as e:
            call()
        assert e.value.code == S.ERR_BAD_SHAPE
    # the device entry without a context refuses before it looks at anything else
    assert _raw(trace, n, 8, R.SHARED, device=True) == S.ERR_NO_DEVICE
    assert S.lib.starkhip_lookup_timings(C.c_void_p(), (C.c_float * 4)()) == S.ERR_NO_DEVICE


def _lookup_air(n_cols, degree, lookups):
    b = AirBuilder(n_cols, 0, degree)
    for lk in lookups:
        b.lookup(*lk)
    return b


def test_the_builders_agree_on_a_lookup():
    for n_cols, degree, lookups in ((4, 3, [(0, 1, 2, 3)]), (7, 3, [(0, 2, 3, 4), (1, 2, 5, 6)]), (8, 4, R.SHARED)):
        b = _lookup_air(n_cols, degree, lookups)
        assert b.lookups == [tuple(lk) for lk in lookups]
        assert b.perm_pairs == [p for (i, t, pi, pt) in lookups for p in ([(i, pi)], [(t, pt)])]
        assert b.count() == 2 * len(lookups)
        assert np.array_equal(b.finish(), S.lookup_air_blob(n_cols, degree, lookups))
    with pytest.raises(ValueError):
        _lookup_air(4, 3, [(0, 1, 2, 4)])
    with pytest.raises(S.StarkhipError):
        S.lookup_air_blob(4, 3, [(0, 1, 2, 4)])
    with pytest.raises(ValueError):  # the constraint has degree 2
        _lookup_air(4, 1, [(0, 1, 2, 3)])


def test_a_filled_trace_satisfies_the_air_the_builder_makes():
    n = 64
    b = _lookup_air(7, 3, [(0, 2, 3, 4), (1, 2, 5, 6)])
    air = S.register_air(b.finish(), name="LookupCpu_two")
    trace = R.shared_table_trace(n, seed=7)[:, :7].copy()
    trace[:, 3:] = 0
    _replay(trace, b.lookups, 0, 0)
    assert S.check_trace_report_replay(air, trace, []).violations == 0
    rep = S.check_trace_permutations_replay(air, trace)
    assert rep.pairs == 4 and rep.pairs_violated == 0 and rep.pairs_undecided == 0
    empty = trace.copy()
    empty[:, 3:] = 0
    assert S.check_trace_report_replay(air, empty, []).violations == 0  # (all-zero witness columns satisfy the two constraints ...)
    assert S.check_trace_permutations_replay(air, empty).pairs_violated == 4  # ... and no pair)


def test_rust_mirror_has_the_new_names():
    rs = open(os.path.join(ROOT, "bindings", "rust", "starkhip-sys", "src", "lib.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("starkhip_lookup_columns", "starkhip_lookup_columns_replay", "starkhip_lookup_timings"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
    for struct, ctype, rtype, mirror in (("starkhip_lookup_t", "uint32_t", "u32", S.api._LookupStruct),
                                         ("starkhip_lookup_report_t", "uint64_t", "u64", S.api._LookupReportStruct)):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1), flags=re.S)
        names = [w for decl in body.split(";") if decl.strip() for w in re.sub(r"\b%s\b" % ctype, "", decl).replace(",", " ").split()]
        rust = re.search(r"pub struct %s \{(.*?)\n\}" % struct, rs, re.S).group(1)
        assert re.findall(r"pub (\w+): %s" % rtype, rust) == names == [f for f, _ in mirror._fields_]
    assert names == ["lookups", "lookups_failed", "missing_rows", "listed"]
    assert "#define STARKHIP_LOOKUPS_MAX 64" in hdr and "STARKHIP_LOOKUPS_MAX: usize = 64" in rs and S.LOOKUPS_MAX == 64
