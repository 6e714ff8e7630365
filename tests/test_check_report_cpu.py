"""The host half of starkhip_check_trace_report without a device (starkhip_check_trace_report_replay): argument checks, summary,
selection of the listed constraints, per-constraint ordering and truncation, against an expectation built from the CPU oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import starky_bls12_381_amd as S
from check_report_util import assert_report, case, check_caps, check_clean, check_corrupted
from random_air import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 7  # CASES[:7]: 8 to 1024 rows
FULL = 1 << 20


@pytest.fixture(scope="module")
def airs():
    return [None] + [S.register_air(case(i)[0], name=f"report{CASES[i][0]}", default_rows=CASES[i][3]) for i in range(1, N)]


# Seed 1 (one column, 8 rows) has the one-constraint program every one-column random AIR has, and test_custom_air_cpu.py expects to be the
# first to register it in a process: that case runs from test_trace_check_report_one_column_cpu.py, which pytest collects after it.
@pytest.mark.parametrize("i", range(1, N))
def test_clean_trace_gives_an_all_zero_report(airs, i):
    check_clean(airs[i], i)


@pytest.mark.parametrize("i", range(1, N))
def test_corrupted_trace_is_reported_as_the_oracle_sees_it(airs, i):
    check_corrupted(airs[i], i)


@pytest.mark.parametrize("i", range(1, N))
def test_cap_cuts_the_list_and_nothing_else(airs, i):
    check_caps(airs[i], i)


def test_a_cut_inside_a_constraint_keeps_its_lowest_rows(airs):
    _, _, bad, pis, want = case(4)  # seed 5: a constraint violated on 128 rows
    cap = 7
    assert want.cuts_inside_a_constraint(cap)
    rep = S.check_trace_report_replay(airs[4], bad, pis, cap=cap)
    assert_report(rep, want, cap)
    k = int(rep.list[-1][0])
    kept = [int(r) for kk, r, _ in rep.list if int(kk) == k]
    all_rows = [int(r) for kk, r, _ in want.list if int(kk) == k]
    assert len(kept) < len(all_rows) and kept == all_rows[:len(kept)]


def _raw(air, trace, pis, n_cols=None, cap=16, per=True, mask=True, n_rows=None, ctx=False):
    """The C entry points themselves: (rc, summary, per_constraint, row_mask, list)."""
    n = trace.shape[0] if n_rows is None else n_rows
    out = S.api._CheckReportStruct()
    p = np.zeros(S.air_num_constraints(air) if S.lib.starkhip_air_num_constraints(air) > 0 else 1, dtype=np.uint32)
    m = np.zeros((trace.shape[0] + 63) // 64, dtype=np.uint64)
    lst = np.zeros((min(cap, FULL), 3), dtype=np.uint64)
    tail = (S.api._p64(np.ascontiguousarray(pis, dtype=np.uint64)), p.ctypes.data_as(S.api._u32p) if per else None, S.api._p64(m) if mask else None,
            S.api._p64(lst) if cap else None, cap, C.byref(out))
    shape = (trace.ctypes.data_as(C.c_void_p), n, trace.shape[1] if n_cols is None else n_cols, 0)
    if ctx:
        rc = S.lib.starkhip_check_trace_report(C.c_void_p(), air, *shape, 0, *tail)
    else:
        rc = S.lib.starkhip_check_trace_report_replay(air, *shape, *tail)
    return rc, out, p, m, lst[:int(out.listed)]


def test_null_outputs_leave_the_others_unchanged(airs):
    _, _, bad, pis, want = case(3)
    rc, out, p, m, lst = _raw(airs[3], bad, pis, cap=16)
    assert rc == 0 and np.array_equal(p, want.per_constraint) and np.array_equal(m, want.row_mask) and np.array_equal(lst, want.list[:16])
    for per, mask in ((False, True), (True, False), (False, False)):
        rc, o, p2, m2, l2 = _raw(airs[3], bad, pis, cap=16, per=per, mask=mask)
        assert rc == 0
        assert (o.violations, o.constraints_violated, o.rows_violated, o.listed) == (want.violations, want.constraints_violated, len(want.rows), 16)
        assert np.array_equal(l2, lst)
        assert np.array_equal(p2, p) if per else not p2.any()
        assert np.array_equal(m2, m) if mask else not m2.any()
    rc, o, *_ = _raw(airs[3], bad, pis, cap=0)  # no list at all
    assert rc == 0 and o.listed == 0 and o.violations == want.violations


def test_refusals(airs):
    _, trace, _, pis, _ = case(3)
    air = airs[3]
    assert _raw(air, trace, pis, cap=FULL + 1)[0] == S.ERR_BAD_SHAPE
    with pytest.raises(S.StarkhipError) as e:
        S.check_trace_report_replay(air, trace, pis, cap=FULL + 1)
    assert e.value.code == S.ERR_BAD_SHAPE
    assert _raw(air, trace[:3], pis)[0] == S.ERR_BAD_SHAPE          # 3 rows
    assert _raw(air, trace, pis, n_cols=trace.shape[1] + 1)[0] == S.ERR_BAD_SHAPE
    assert len(pis) > 0
    big = pis.copy()
    big[0] = np.uint64(S.P)
    assert _raw(air, trace, big)[0] == S.ERR_BAD_SHAPE                # a public input that is not canonical
    assert _raw(air, trace, pis)[0] == 0
    unregistered = S.AIR_CUSTOM_BASE + S.AIR_CUSTOM_CAPACITY + 7
    assert S.lib.starkhip_air_num_constraints(unregistered) == S.ERR_BAD_AIR
    assert _raw(unregistered, trace, pis)[0] == S.ERR_BAD_AIR


def test_device_entry_point_without_a_context(airs):
    _, trace, _, pis, _ = case(1)
    assert _raw(airs[1], trace, pis, ctx=True)[0] == S.ERR_NO_DEVICE


def test_header_and_rust_binding_declare_the_report():
    hdr = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "starkhip-sys", "src", "lib.rs")).read()
    for name in ("starkhip_check_trace_report", "starkhip_check_trace_report_replay"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
    assert "STARKHIP_CHECK_LIST_MAX (1u << 20)" in hdr and "pub struct starkhip_check_report_t" in rs
