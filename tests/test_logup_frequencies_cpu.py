"""starkhip_logup_frequencies_replay -- the host driver of starkhip_logup_frequencies over host loops -- against the numpy reference
of logup_freq_ref.py, the refusals of both entries, the fillable test, the LogUp blob and the Rust declarations.  No device needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import logup_freq_ref as R
import starky_bls12_381_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P


def replay(air, trace, layout, cap):
    return S.logup_frequencies_replay(air, trace, layout=layout, cap=cap)


def registered(m, n_lookups, tables=None):
    lookups, n_cols = R.layout_of(m, n_lookups, tables)
    return S.register_air(R.make_air(n_cols, lookups)), lookups, n_cols


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 5])
@pytest.mark.parametrize("n", [2, 4, 64, 1024])
def test_replay_is_the_reference(n, m, layout):
    air, lookups, n_cols = registered(m, 2)
    for kind in ("uniform", "equal", "duplicates", "big"):
        trace = R.make_trace(n, lookups, n_cols, seed=n + m, kind=kind, layout=layout)
        _, rep = R.run(replay, air, trace, lookups, layout)
        assert rep.failed == 0 and rep.missing_cells == 0 and len(rep.list) == 0


def test_sixty_four_columns_in_one_lookup():
    air, lookups, n_cols = registered(64, 1)
    assert S.air_logup_columns(air) == 64 and S.air_logup_columns(registered(5, 2)[0]) == 10 and S.air_logup_columns(S.AIR_TEST_FIBONACCI) == 0
    with pytest.raises(S.StarkhipError):
        S.air_logup_columns(10 ** 6)
    R.run(replay, air, R.make_trace(64, lookups, n_cols, seed=3), lookups)


def test_a_duplicated_table_value_gives_its_count_to_the_lowest_row():
    air, lookups, n_cols = registered(2, 1)
    cols, table, freq = lookups[0]
    t = np.zeros((8, n_cols), dtype=np.uint64)
    t[:, table] = [9, 4, 9, 4, 7, 9, 4, 4 + P]
    t[:, cols[0]] = [9, 9, 4, 7, 7, 9 + P, 4, 4]
    t[:, cols[1]] = 9
    got, rep = R.run(replay, air, t, lookups)
    assert list(got[:, freq]) == [11, 3, 0, 0, 2, 0, 0, 0] and rep.failed == 0


def test_two_lookups_with_tables_of_their_own_and_two_that_share_one():
    air, lookups, n_cols = registered(2, 3, tables=[1, 11, 1])
    assert n_cols == 12
    for layout in (0, 1):
        R.run(replay, air, R.make_trace(64, lookups, n_cols, seed=5, layout=layout), lookups, layout)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_failing_lookup_keeps_its_column_beside_one_that_is_written(layout):
    air, lookups, n_cols = registered(2, 2)
    trace = R.make_trace(64, lookups, n_cols, seed=8, layout=layout)
    v = R.view(trace, layout)
    cols, table, freq = lookups[1]
    sorted_table = np.sort(v[:, table])
    below, between, above = int(sorted_table[0]) - 1, int(sorted_table[10]) + 1, int(sorted_table[-1]) + 1
    assert not np.isin([below, between, above], v[:, table]).any()
    v[3, cols[0]], v[3, cols[1]], v[40, cols[1]], v[63, cols[0]] = below, between, above, between + P
    before = v[:, freq].copy()
    got, rep = R.run(replay, air, trace, lookups, layout)
    assert np.array_equal(R.view(got, layout)[:, freq], before)                      # the failed lookup's column: untouched
    assert not np.array_equal(R.view(got, layout)[:, lookups[0][2]], v[:, lookups[0][2]])  # the other one: written
    assert (rep.failed, rep.missing_cells, rep.missing_rows) == (1, 4, 3)
    assert list(rep.per_lookup) == [0, 4] and list(rep.per_column) == [0, 0, 2, 2]   # per_column names the column
    assert [tuple(e) for e in rep.list] == [(1, 3), (1, 40), (1, 63)]


def test_the_list_is_cut_at_cap_in_lookup_then_row_order():
    air, lookups, n_cols = registered(1, 2)
    trace = R.make_trace(64, lookups, n_cols, seed=9)
    trace[::2, lookups[0][0][0]] = 1  # 32 rows of lookup 0
    trace[5, lookups[1][0][0]] = 2
    for cap in (0, 1, 32, 33, 1024):
        _, rep = R.run(replay, air, trace, lookups, cap=cap)
        assert len(rep.list) == min(cap, 33) and rep.missing_rows == 33 and rep.failed == 2


def raw(entry, air, trace, n_rows, n_cols, layout, cap, with_list=True, out=True):
    rep = S.api._LogupReportStruct()
    lst = np.zeros((max(1, cap), 2), dtype=np.uint64)
    tail = (None, None, None, lst.ctypes.data_as(S.api._u64p) if with_list else None, cap, C.byref(rep) if out else None)
    ptr = trace.ctypes.data_as(C.c_void_p) if trace is not None else None
    if entry == "device":
        return S.lib.starkhip_logup_frequencies(C.c_void_p(), air, ptr, n_rows, n_cols, layout, 0, *tail)
    return S.lib.starkhip_logup_frequencies_replay(air, ptr, n_rows, n_cols, layout, *tail)


def test_every_refusal():
    air, lookups, n_cols = registered(2, 2)
    t = R.make_trace(64, lookups, n_cols, seed=1)
    assert raw("device", air, t, 64, n_cols, 0, 0) == S.ERR_NO_DEVICE  # without a context nothing else is looked at
    assert raw("replay", air, t, 64, n_cols, 0, 16) == 0
    plain = S.register_air(R.make_air(n_cols, []))
    for bad_air in (plain, S.AIR_TEST_FIBONACCI, 10 ** 6):
        assert raw("replay", bad_air, t, 64, n_cols, 0, 0) == S.ERR_BAD_AIR
    for args in ((None, 64, n_cols, 0, 0), (t, 64, n_cols, 2, 0), (t, 64, n_cols + 1, 0, 0), (t, 48, n_cols, 0, 0), (t, 1, n_cols, 0, 0),
                 (t, 1 << (S.MAX_LOG_ROWS + 1), n_cols, 0, 0), (t, 64, n_cols, 0, S.CHECK_LIST_MAX + 1)):
        assert raw("replay", air, *args) == S.ERR_BAD_SHAPE, args[1:]
    assert raw("replay", air, t, 64, n_cols, 0, 4, with_list=False) == S.ERR_BAD_SHAPE
    assert raw("replay", air, t, 64, n_cols, 0, 0, out=False) == S.ERR_BAD_SHAPE
    for call in (lambda: S.logup_frequencies_replay(air, t[:, ::2]), lambda: S.logup_frequencies_replay(air, t.astype(np.int64)),
                 lambda: S.logup_frequencies_replay(air, t, cap=-1), lambda: S.logup_frequencies_replay(air, t, layout=2)):
        with pytest.raises(S.StarkhipError):
            call()


def test_an_air_that_is_not_fillable_is_refused_whatever_the_order():
    good = [([2, 3], 1, 4), ([5], 1, 6)]
    assert S.air_logup_fillable(S.register_air(R.make_air(8, good)))
    bad_lists = ([([2, 3], 1, 4), ([4], 1, 6)],   # a frequencies column that another lookup looks up
                 [([4], 1, 6), ([2, 3], 1, 4)],   # ... in the other order
                 [([2, 3], 1, 4), ([5], 4, 6)],   # ... that is another lookup's table
                 [([2, 3], 1, 4), ([5], 1, 4)],   # ... that is another lookup's frequencies column
                 [([2, 3], 1, 1)],                # ... that is its own table
                 [([2, 3], 1, 3)])                # ... that is one of its own columns
    for lookups in bad_lists:
        air = S.register_air(R.make_air(8, lookups))
        assert S.air_logup_fillable(air) is False
        t = R.make_trace(16, good, 8, seed=2)
        with pytest.raises(S.StarkhipError) as e:
            S.logup_frequencies_replay(air, t)
        assert e.value.code == S.ERR_BAD_SHAPE
        with pytest.raises(S.StarkhipError) as e:
            S.logup_blob_replay(air, t)
        assert e.value.code == S.ERR_BAD_AIR
    for air in (S.AIR_TEST_FIBONACCI, 10 ** 6):
        with pytest.raises(S.StarkhipError) as e:
            S.air_logup_fillable(air)
        assert e.value.code == S.ERR_BAD_AIR


def test_blob_layout_and_replay():
    air, lookups, n_cols = registered(2, 2)
    for layout in (0, 1):
        trace = R.make_trace(64, lookups, n_cols, seed=4, layout=layout)
        assert S.logup_blob_replay(air, trace, layout=layout) is None
        v = R.view(trace, layout)
        v[::4, lookups[0][0][1]] = 3
        v[7, lookups[1][0][0]] = 3
        v[7, lookups[1][0][1]] = 3
        kept = trace.copy()
        for cap in (0, 5, 16, 64):
            blob = S.logup_blob_replay(air, trace, layout=layout, cap=cap)
            assert np.array_equal(trace, kept)  # only read
            e = R.fill(trace, lookups, layout, cap)
            assert list(blob[:8]) == [S.LOGUP_MAGIC, air, 64, 2, 2, 17, min(cap, 17), 18] and blob.size == 8 + 2 * min(cap, 17)
            rep = S.logup_blob_layout(blob)
            assert (rep.air, rep.n_rows, rep.lookups, rep.failed, rep.missing_cells, rep.missing_rows) == (air, 64, 2, 2, 18, 17)
            assert np.array_equal(rep.list, e.list)
            # truncated, extended, another magic, a `listed` that disagrees
            for bad in (blob[:-1], blob[:7], np.append(blob, np.uint64(0)), blob[:0]):
                with pytest.raises(S.StarkhipError):
                    S.logup_blob_layout(bad)
            other = blob.copy()
            other[0] = S.LOOKUP_MAGIC
            with pytest.raises(S.StarkhipError):
                S.logup_blob_layout(other)
            with pytest.raises(S.StarkhipError):
                S.parse_lookup_blob(blob)  # the lookup blob's reader refuses a LogUp blob ...
            if cap:
                other = blob.copy()
                other[6] += 1
                with pytest.raises(S.StarkhipError):
                    S.logup_blob_layout(other)
    lookup_blob = np.array([S.LOOKUP_MAGIC, air, 64, 2, 1, 1, 1, 0, 0, 5], dtype=np.uint64)
    assert S.parse_lookup_blob(lookup_blob).missing_rows == 1
    with pytest.raises(S.StarkhipError):
        S.logup_blob_layout(lookup_blob)  # ... and the LogUp blob's reader a lookup blob
    violation = S.TraceViolation(S.logup_blob_replay(air, trace, layout=1, cap=3))
    assert violation.report is None and violation.lookup_report is None and violation.logup_report.missing_cells == 18


def test_rust_mirror_has_the_new_names():
    rs = open(os.path.join(ROOT, "bindings", "rust", "starkhip-sys", "src", "lib.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("starkhip_logup_frequencies", "starkhip_logup_frequencies_replay", "starkhip_logup_frequency_timings", "starkhip_air_logup_fillable",
                 "starkhip_air_logup_columns",
                 "starkhip_logup_blob_layout", "starkhip_logup_blob_replay"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
        c_args = re.search(r"\nint %s\(([^)]*)\)" % name, hdr).group(1).count(",")
        assert re.search(r"pub fn %s\s*\(([^)]*)\)" % name, rs).group(1).count(",") == c_args, name
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} starkhip_logup_report_t;", hdr).group(1), flags=re.S)
    names = [w for decl in body.split(";") if decl.strip() for w in re.sub(r"\buint64_t\b", "", decl).replace(",", " ").split()]
    rust = re.search(r"pub struct starkhip_logup_report_t \{(.*?)\n\}", rs, re.S).group(1)
    assert re.findall(r"pub (\w+): u64", rust) == names == [f for f, _ in S.api._LogupReportStruct._fields_]
    assert names == ["lookups", "lookups_failed", "missing_cells", "missing_rows", "listed"]
    magic = int(re.search(r"#define STARKHIP_LOGUP_MAGIC (0x[0-9A-Fa-f]+)ULL", hdr).group(1), 16)
    assert magic == S.LOGUP_MAGIC and magic.to_bytes(8, "little") == b"SSLGU001"
    assert int(re.search(r"pub const STARKHIP_LOGUP_MAGIC: u64 = (0x[0-9A-Fa-f_]+);", rs).group(1).replace("_", ""), 16) == magic
