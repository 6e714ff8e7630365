"""The context option "check_trace": prove() checks the trace it has just uploaded against the AIR, on the device, before the LDE.
A satisfying trace is proven to the bytes it has with the option off; a violating one comes back as ERR_TRACE with the check blob
the CPU replay builds (small AIRs) or the device report gives (the built-ins), and the context goes on proving.  Rows: 2 (one
row-wave, mostly idle lanes), 64 and 128 (one and two row-waves, a cell changed on the first row, at the wave boundary and on the last
row), 2^14 (the long-trace path), FP12Mul at 16 rows (parked, host-hashed commitment), PairingPrecomp at 1024 (parked, 29 376
columns).  Forms: host rows and columns, a column table, a recording, device rows and columns."""
import os
import subprocess
import sys

import numpy as np
import pytest

import starky_bls12_381_amd as S
from bls_util import random_fp12
from config_cases import make_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = S.AIR_TEST_FIBONACCI


@pytest.fixture(scope="module")
def checked():
    """a second context on the device with the option on; the session's `prover` has it off and gives the reference bytes"""
    p = S.Prover(0)
    p.set_option("check_trace", 1)
    yield p
    p.close()


def _bump(trace, r, c, by=1):
    bad = trace.copy()
    bad[r, c] = np.uint64((int(bad[r, c]) + by) % S.P)
    return bad


def _refused(call):
    with pytest.raises(S.TraceViolation) as e:
        call()
    assert e.value.code == S.ERR_TRACE and e.value.blob[0] == S.CHECK_MAGIC
    return e.value


def _accepts(prover, checked, air, cfg, trace, pis, **kw):
    """the proof with the option on is the one with it off, verifies, and was counted as checked"""
    before = checked.check_stats()
    want = prover.prove(air, cfg, trace, pis, **kw)
    got = checked.prove(air, cfg, trace, pis, **kw)
    assert np.array_equal(got, want)
    S.verify_stark_proof(air, cfg, got)
    after = checked.check_stats()
    assert (after["checked"], after["rejected"]) == (before["checked"] + 1, before["rejected"])
    return want


def _refuses_like_the_replay(prover, checked, air, cfg, bad, pis, cap=16, **kw):
    before = checked.check_stats()
    err = _refused(lambda: checked.prove(air, cfg, bad, pis, **kw))
    layout = kw.get("layout", 0)
    assert np.array_equal(err.blob, S.check_blob_replay(air, bad, pis, layout=layout, cap=cap))
    count, first = prover.check_trace(air, bad, pis, layout=layout)
    assert err.report.violations == count and (cap == 0 or tuple(int(x) for x in err.report.list[0]) == first)
    after = checked.check_stats()
    assert (after["checked"], after["rejected"]) == (before["checked"] + 1, before["rejected"] + 1)
    return err


@pytest.mark.parametrize("n", [2, 64, 128])
def test_toy_air_rows_and_the_cells_that_matter(prover, checked, n):
    # (two rows at standard_fast's cap height are no shape: a config with a smaller cap, as tests/config_cases.py has for log_n = 1)
    cfg = S.StarkConfig.standard_fast_config() if n > 2 else make_config(2, 3, 2, 0, 2, 0)
    t, pis = S.trace_fibonacci(0, 1, n)
    want = _accepts(prover, checked, TOY, cfg, t, pis)
    for r in sorted({0, min(63, n - 1), min(64, n - 1), n - 1}):  # first row, both sides of the wave boundary, last row (the wrap frame)
        for c in (1, 3):
            bad = _bump(t, r, c)
            _refuses_like_the_replay(prover, checked, TOY, cfg, bad, pis)
            _refuses_like_the_replay(prover, checked, TOY, cfg, bad.T.copy(), pis, layout=1)
    assert np.array_equal(checked.prove(TOY, cfg, t, pis), want)  # the context is as usable as before


def test_the_list_is_cut_like_the_reports(prover, checked):
    cfg = S.StarkConfig.standard_fast_config()
    t, pis = S.trace_fibonacci(0, 1, 128)
    bad = t.copy()
    bad[:, 2] = (bad[:, 2] + np.uint64(1)) % np.uint64(S.P)  # the product column on every row: constraints violated on 128 rows each
    total = prover.check_trace(TOY, bad, pis)[0]
    assert total > 128
    try:
        for cap in (0, 1, 7, 130, total + 5):
            checked.set_option("check_trace_list", cap)
            err = _refuses_like_the_replay(prover, checked, TOY, cfg, bad, pis, cap=cap)
            assert len(err.report.list) == min(cap, total)
        with pytest.raises(S.StarkhipError) as e:
            checked.set_option("check_trace_list", S.CHECK_LIST_MAX + 1)
        assert e.value.code == S.ERR_BAD_SHAPE
        with pytest.raises(S.StarkhipError) as e:
            checked.set_option("check_trace", 2)
        assert e.value.code == S.ERR_BAD_SHAPE
    finally:
        checked.set_option("check_trace_list", 16)
    # option off again: the violating trace is proven (to something no verifier accepts) and nothing is counted
    before = checked.check_stats()
    checked.set_option("check_trace", 0)
    try:
        proof = checked.prove(TOY, cfg, _bump(t, 5, 3), pis)
        with pytest.raises(S.StarkhipError) as e:
            S.verify_stark_proof(TOY, cfg, proof)
        assert e.value.code == S.ERR_VERIFY
    finally:
        checked.set_option("check_trace", 1)
    assert checked.check_stats() == before


def _writes(trace):
    r, c = np.nonzero(trace)
    return np.stack([r.astype(np.uint64), c.astype(np.uint64), trace[r, c]], axis=1)


def test_host_forms_column_table_and_recording(prover, checked):
    """16 rows of Fibonacci(0, 1): every cell is below 2^32, as a recording needs"""
    cfg = S.StarkConfig.standard_fast_config()
    t, pis = S.trace_fibonacci(0, 1, 16)
    assert int(t.max()) < 1 << 32
    bad = _bump(t, 9, 0)
    want = _accepts(prover, checked, TOY, cfg, t, pis)
    blob = S.check_blob_replay(TOY, bad, pis)
    assert blob is not None
    before = checked.check_stats()
    # row-major and column-major host, a column table, a recording
    assert np.array_equal(checked.prove(TOY, cfg, t.T.copy(), pis, layout=1), want)
    assert np.array_equal(checked.prove_columns(TOY, cfg, [t[:, c].copy() for c in range(t.shape[1])], pis), want)
    assert np.array_equal(checked.prove(TOY, cfg, S.trace_from_writes(16, t.shape[1], _writes(t)), pis), want)
    for call in (lambda: checked.prove(TOY, cfg, bad, pis),
                 lambda: checked.prove(TOY, cfg, bad.T.copy(), pis, layout=1),
                 lambda: checked.prove_columns(TOY, cfg, [bad[:, c].copy() for c in range(bad.shape[1])], pis),
                 lambda: checked.prove(TOY, cfg, S.trace_from_writes(16, bad.shape[1], _writes(bad)), pis)):
        assert np.array_equal(_refused(call).blob, blob)
    after = checked.check_stats()
    assert (after["checked"], after["rejected"]) == (before["checked"] + 7, before["rejected"] + 4)
    assert np.array_equal(checked.prove(TOY, cfg, t, pis), want)


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import starky_bls12_381_amd as S
from check_report_util import case
torch.cuda.set_device(0)
blob, good, bad, pis, want = case(5)  # seed 6: 256 rows, several row-waves
air = S.register_air(blob)
cfg = S.StarkConfig.for_air(air)
n = good.shape[0]
pv = S.Prover(0)
ref = pv.prove(air, cfg, good, pis)
expect = S.check_blob_replay(air, bad, pis)
assert expect is not None and int(expect[3]) == want.violations
pv.set_option("check_trace", 1)
dev = lambda a: torch.from_numpy(a.copy().view(np.int64)).to("cuda:0")
g_rows, g_cols, b_rows, b_cols = dev(good), dev(good.T), dev(bad), dev(bad.T)
torch.cuda.synchronize()
for layout, g, b in ((0, g_rows, b_rows), (1, g_cols, b_cols)):
    assert np.array_equal(pv.prove_device(air, cfg, g.data_ptr(), n, pis, layout=layout), ref)
    try:
        pv.prove_device(air, cfg, b.data_ptr(), n, pis, layout=layout)
        raise SystemExit("a violating trace in device memory was proven")
    except S.TraceViolation as e:
        assert np.array_equal(e.blob, expect), layout
    assert np.array_equal(pv.prove_device(air, cfg, g.data_ptr(), n, pis, layout=layout), ref)
assert np.array_equal(b_cols.cpu().numpy().view(np.uint64), bad.T) and np.array_equal(g_cols.cpu().numpy().view(np.uint64), good.T)  # read in place
assert pv.check_stats() == {"checked": 6, "rejected": 2}
S.verify_stark_proof(air, cfg, ref)
pv.close()
print("device forms ok")
"""


def test_traces_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_long_trace_of_a_registered_toy_air(prover, checked):
    """2^14 rows: the trace is in `values`, which the long transform then turns into coefficients in place"""
    air = S.register_air(S.air_program(TOY), name="toy_copy", default_rows=1 << 14)
    cfg = S.StarkConfig.for_air(air)
    n = 1 << 14
    t, pis = S.trace_fibonacci(0, 1, n)
    want = _accepts(prover, checked, air, cfg, t, pis)
    for r, c in ((0, 0), (8191, 1), (n - 1, 2)):
        _refuses_like_the_replay(prover, checked, air, cfg, _bump(t, r, c), pis)
    assert np.array_equal(checked.prove(air, cfg, t, pis), want)


def _refuses_like_the_device_report(prover, checked, air, cfg, bad, pis, proofs):
    rep = prover.check_trace_report(air, bad, pis, cap=16)
    count, first = prover.check_trace(air, bad, pis)
    assert count > 0
    for prove in proofs:
        err = _refused(prove)
        head = [S.CHECK_MAGIC, air, bad.shape[0], rep.violations, rep.constraints_violated, rep.rows_violated, len(rep.list), 0]
        assert np.array_equal(err.blob, np.concatenate([np.array(head, dtype=np.uint64), rep.list.reshape(-1)]))
        assert err.report.violations == count and tuple(int(x) for x in err.report.list[0]) == first


def test_fp12_mul_parked_with_a_host_hashed_commitment(prover, checked):
    air = S.AIR_FP12_MUL
    cfg = S.StarkConfig.for_air(air)
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED7300), random_fp12(0x5EED7301))
    assert t.shape[0] == 16 and int(t.max()) < 1 << 32
    want = _accepts(prover, checked, air, cfg, t, pis)
    bad = t.copy()
    bad[9, 5] ^= np.uint64(4)  # one limb changed
    assert int(bad[9, 5]) < 1 << 32
    # the dense trace, and a recording rebuilt from it
    _refuses_like_the_device_report(prover, checked, air, cfg, bad, pis,
                                    [lambda: checked.prove(air, cfg, bad, pis),
                                     lambda: checked.prove(air, cfg, S.trace_from_writes(16, bad.shape[1], _writes(bad)), pis)])
    assert np.array_equal(checked.prove(air, cfg, S.trace_from_writes(16, t.shape[1], _writes(t)), pis), want)


def test_pairing_precomp_parked_with_29376_columns(prover, checked):
    from test_gpu_pool import _precomp_args
    air = S.AIR_PAIRING_PRECOMP
    cfg = S.StarkConfig.for_air(air)
    t, pis = S.trace_pairing_precomp(*_precomp_args(0x5EED7310))
    assert t.shape == (1024, 29376)
    want = _accepts(prover, checked, air, cfg, t, pis)
    bad = _bump(t, 700, 3, by=5)
    _refuses_like_the_device_report(prover, checked, air, cfg, bad, pis, [lambda: checked.prove(air, cfg, bad, pis)])
    assert np.array_equal(checked.prove(air, cfg, t, pis), want)
