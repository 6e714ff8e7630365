"""The check blob of a prove with "check_trace" on, without a device: starkhip_check_blob_replay against
starkhip_check_trace_report_replay word for word, starkhip_check_blob_layout on those blobs and on what it must refuse, the new
error code and its string."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from check_report_util import case
from random_air import CASES

MAGIC = 0x3130304B48435353  # "SSCHK001"


def _bump(trace, r, c):
    bad = trace.copy()
    bad[r, c] = np.uint64((int(bad[r, c]) + 1) % S.P)
    return bad


@pytest.fixture(scope="module")
def traces():
    """[(air, satisfying trace, the same with one cell changed, public inputs)]: the toy AIR at 16 rows and one random AIR at 64"""
    t, pis = S.trace_fibonacci(0, 1, 16)
    blob, rt, _, rpis, _ = case(3)
    return [(S.AIR_TEST_FIBONACCI, t, _bump(t, 5, 1), pis),
            (S.register_air(blob, name=f"report{CASES[3][0]}", default_rows=CASES[3][3]), rt, _bump(rt, rt.shape[0] // 2, 0), rpis)]


def _expected_blob(air, trace, pis, layout, cap):
    rep = S.check_trace_report_replay(air, trace, pis, layout=layout, cap=cap)
    n = trace.shape[0] if layout == 0 else trace.shape[1]
    head = [MAGIC, air, n, rep.violations, rep.constraints_violated, rep.rows_violated, len(rep.list), 0]
    return rep, np.concatenate([np.array(head, dtype=np.uint64), rep.list.reshape(-1)])


@pytest.mark.parametrize("which", [0, 1])
def test_blob_replay_is_the_report_replay_word_for_word(traces, which):
    air, good, bad, pis = traces[which]
    total = S.check_trace_report_replay(air, bad, pis, cap=0).violations
    assert total > 1
    for layout, g, b in ((0, good, bad), (1, good.T.copy(), bad.T.copy())):
        for cap in (0, 1, total + 3):
            assert S.check_blob_replay(air, g, pis, layout=layout, cap=cap) is None
            rep, want = _expected_blob(air, b, pis, layout, cap)
            got = S.check_blob_replay(air, b, pis, layout=layout, cap=cap)
            assert got.dtype == np.uint64 and np.array_equal(got, want)
            assert len(rep.list) == min(cap, total)
            parsed = S.parse_check_blob(got)
            assert isinstance(parsed, S.CheckReport)
            assert (parsed.air, parsed.n_rows) == (air, good.shape[0])
            assert (parsed.violations, parsed.constraints_violated, parsed.rows_violated) == (rep.violations, rep.constraints_violated, rep.rows_violated)
            assert np.array_equal(parsed.list, rep.list)


def _layout(blob):
    out = S.api._CheckReportStruct()
    lst = S.api._u64p()
    rc = S.lib.starkhip_check_blob_layout(S.api._p64(blob), blob.size, C.byref(out), C.byref(lst))
    return rc, out, lst


def test_layout_points_into_the_blob_and_refuses_what_is_not_one(traces):
    air, good, bad, pis = traces[0]
    blob = S.check_blob_replay(air, bad, pis, cap=3)
    rc, out, lst = _layout(blob)
    assert rc == 0 and out.listed == 3 and out.violations == blob[3]
    assert C.addressof(lst.contents) == blob.ctypes.data + 8 * 8
    rc, out, lst = _layout(S.check_blob_replay(air, bad, pis, cap=0))
    assert rc == 0 and out.listed == 0 and out.violations == blob[3] and not lst
    # a proof blob (the oracle's, of the satisfying trace)
    proof = O.prove(S.air_program(air), S.StarkConfig.standard_fast_config(), S.trace_rows_to_poly_values(good), pis)
    assert _layout(proof)[0] == S.ERR_BAD_SHAPE
    with pytest.raises(S.StarkhipError) as e:
        S.parse_check_blob(proof)
    assert e.value.code == S.ERR_BAD_SHAPE
    # truncated: inside the list, inside the header, nothing
    for words in (blob.size - 1, blob.size - 3, 7, 0):
        assert _layout(blob[:words].copy())[0] == S.ERR_BAD_SHAPE
    longer = np.concatenate([blob, np.zeros(3, dtype=np.uint64)])
    assert _layout(longer)[0] == S.ERR_BAD_SHAPE
    # `listed` disagrees with the length
    for listed in (2, 4):
        wrong = blob.copy()
        wrong[6] = listed
        assert _layout(wrong)[0] == S.ERR_BAD_SHAPE
    wrong = blob.copy()
    wrong[0] ^= np.uint64(1)
    assert _layout(wrong)[0] == S.ERR_BAD_SHAPE
    assert S.lib.starkhip_check_blob_layout(None, 8, C.byref(out), C.byref(lst)) == S.ERR_BAD_SHAPE
    assert S.lib.starkhip_check_blob_layout(S.api._p64(blob), blob.size, None, None) == S.ERR_BAD_SHAPE
    assert S.lib.starkhip_check_blob_layout(S.api._p64(blob), blob.size, C.byref(out), None) == 0  # the list pointer is optional


def test_replay_refusals(traces):
    air, good, bad, pis = traces[0]
    with pytest.raises(S.StarkhipError) as e:
        S.check_blob_replay(air, bad, pis, cap=S.CHECK_LIST_MAX + 1)
    assert e.value.code == S.ERR_BAD_SHAPE
    with pytest.raises(S.StarkhipError) as e:
        S.check_blob_replay(air, bad[:3], pis)
    assert e.value.code == S.ERR_BAD_SHAPE
    with pytest.raises(S.StarkhipError) as e:
        S.check_blob_replay(S.AIR_CUSTOM_BASE + S.AIR_CUSTOM_CAPACITY + 7, bad, pis[:0])
    assert e.value.code == S.ERR_BAD_AIR


def test_error_code_and_string():
    assert S.ERR_TRACE == -9
    text = S.lib.starkhip_error_string(S.ERR_TRACE).decode()
    assert "trace" in text and "AIR" in text and text != S.lib.starkhip_error_string(-99).decode()
    blob = S.check_blob_replay(S.AIR_TEST_FIBONACCI, _bump(S.trace_fibonacci(0, 1, 16)[0], 5, 1), S.trace_fibonacci(0, 1, 16)[1])
    err = S.TraceViolation(blob)
    assert isinstance(err, S.StarkhipError) and err.code == S.ERR_TRACE and err.report.violations == blob[3]
    assert len(err.report.list) == min(16, int(blob[3]))


def test_context_and_pool_entries_without_a_device():
    out = np.zeros(2, dtype=np.uint64)
    assert S.lib.starkhip_check_stats(None, S.api._p64(out)) == S.ERR_NO_DEVICE
    assert S.lib.starkhip_pool_check_stats(None, S.api._p64(out)) == S.ERR_BAD_SHAPE
    assert S.lib.starkhip_set_option(None, b"check_trace", 1) == S.ERR_NO_DEVICE
