"""starkhip_check_trace_report on the device (kernels_check.hip) against an expectation built from the CPU oracle, against its
own host replay, and against starkhip_check_trace, on random AIRs of 8 to 1024 rows and on a real FP12Mul trace."""
import os
import subprocess
import sys

import numpy as np
import pytest

import starky_bls12_381_amd as S
from bls_util import random_fp12
from check_report_util import Expected, assert_report, case
from random_air import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 7  # CASES[:7]: 8, 16, 32 rows (idle lanes), 64 (one wave), 128, 256, 1024 (several waves per constraint)
FULL = 1 << 20


@pytest.fixture(scope="module")
def airs():
    return [S.register_air(case(i)[0], name=f"report{CASES[i][0]}", default_rows=CASES[i][3]) for i in range(N)]


def _same(a, b):
    assert (a.violations, a.constraints_violated, a.rows_violated) == (b.violations, b.constraints_violated, b.rows_violated)
    for f in ("per_constraint", "row_mask", "rows", "list"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


@pytest.mark.parametrize("i", range(N))
def test_report_is_the_oracles_and_the_replays(prover, airs, i):
    _, trace, bad, pis, want = case(i)
    air = airs[i]
    for layout, clean, broken in ((0, trace, bad), (1, trace.T.copy(), bad.T.copy())):
        rep = prover.check_trace_report(air, clean, pis, layout=layout, cap=FULL)
        assert (rep.violations, rep.constraints_violated, rep.rows_violated) == (0, 0, 0)
        assert not rep.per_constraint.any() and not rep.row_mask.any() and rep.rows.size == 0 and rep.list.shape == (0, 3)
        assert_report(prover.check_trace_report(air, broken, pis, layout=layout, cap=FULL), want, FULL)
        for cap in (0, 1, 7, want.violations - 1):
            got = prover.check_trace_report(air, broken, pis, layout=layout, cap=cap)
            _same(got, S.check_trace_report_replay(air, broken, pis, layout=layout, cap=cap))
            assert_report(got, want, cap)


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first, as in tools/check_trace_bench.py
import starky_bls12_381_amd as S
from check_report_util import assert_report, case
torch.cuda.set_device(0)
blob, _, bad, pis, want = case(5)  # seed 6: 256 rows
air = S.register_air(blob)
pv = S.Prover(0)
cols = torch.from_numpy(bad.T.copy().view(np.int64)).to("cuda:0")
rows = torch.from_numpy(bad.copy().view(np.int64)).to("cuda:0")
torch.cuda.synchronize()
got = pv.check_trace_report_device(air, cols.data_ptr(), bad.shape[0], pis, layout=1, cap=1 << 20)
host = pv.check_trace_report(air, bad, pis, cap=1 << 20)
for f in ("violations", "constraints_violated", "rows_violated"):
    assert getattr(got, f) == getattr(host, f), f
for f in ("per_constraint", "row_mask", "rows", "list"):
    assert np.array_equal(getattr(got, f), getattr(host, f)), f
assert_report(got, want, 1 << 20)
assert pv.last_call_s > 0
assert_report(pv.check_trace_report_device(air, rows.data_ptr(), bad.shape[0], pis, layout=0, cap=9), want, 9)
assert np.array_equal(cols.cpu().numpy().view(np.uint64), bad.T)  # read in place, left as it was
pv.close()
print("device report ok")
"""


def test_report_of_a_trace_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device report ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("i", range(N))
def test_report_agrees_with_check_trace_and_leaves_it_alone(prover, airs, i):
    _, trace, bad, pis, _ = case(i)
    before = prover.check_trace(airs[i], bad, pis)
    rep = prover.check_trace_report(airs[i], bad, pis)
    assert before[0] == rep.violations
    assert before[1] == tuple(int(x) for x in rep.list[0])
    assert prover.check_trace(airs[i], bad, pis) == before  # the op-stream cache is shared
    assert prover.check_trace(airs[i], trace, pis) == (0, (0, 0, 0))


def test_wrong_public_input_on_a_clean_trace(prover, airs):
    for i in range(2, N):
        blob, trace, _, pis, _ = case(i)
        if not len(pis):
            continue
        n = trace.shape[0]
        wrong = pis.copy()
        wrong[0] = np.uint64((int(wrong[0]) + 1) % S.P)
        want = Expected(blob, trace, wrong)
        assert want.violations > 0
        rep = prover.check_trace_report(airs[i], trace, wrong, cap=FULL)
        assert np.array_equal(np.flatnonzero(rep.per_constraint), np.flatnonzero(want.per_constraint))
        assert set(rep.rows.tolist()) <= {0, n - 1} | set(want.rows.tolist())
        assert_report(rep, want, FULL)


def _fp12_mul_cases():
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED7200), random_fp12(0x5EED7201))
    assert t.shape[0] == 16
    width = t.shape[1]
    out = []
    for c in (0, 5, width // 7, width // 3, width // 2, 2 * width // 3, width - 2, width - 1):
        bad = t.copy()
        bad[9, c] = np.uint64((int(bad[9, c]) + 3) % S.P)
        out.append(bad)
    return t, pis, out


def test_report_on_a_real_fp12_mul_trace(prover):
    t, pis, bads = _fp12_mul_cases()
    blob = S.air_program(S.AIR_FP12_MUL)
    custom = S.register_air(blob)
    for air in (S.AIR_FP12_MUL, custom):
        rep = prover.check_trace_report(air, t, pis)
        assert (rep.violations, rep.constraints_violated, rep.rows_violated, len(rep.list)) == (0, 0, 0, 0) and not rep.per_constraint.any()
    broken = 0
    for bad in bads:  # one corrupted cell; not every cell is constrained on every row
        want = Expected(blob, bad, pis)
        rep = prover.check_trace_report(S.AIR_FP12_MUL, bad, pis, cap=FULL)
        assert_report(rep, want, FULL)
        _same(rep, prover.check_trace_report(custom, bad, pis, cap=FULL))  # the same AIR under a registered id
        broken += want.violations > 0
    assert broken > 0
