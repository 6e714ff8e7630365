"""starkhip_check_trace_free_cells on the device (kernels_free_classes.hip) against its host replay, bit for bit: a hand-written AIR
whose free cells are known by construction, random AIRs of 128 to 4096 rows, and a real FP12Mul trace."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import starky_bls12_381_amd as S
from bls_util import random_fp12
from check_report_util import corrupt
from free_cells_util import assert_same, case, corrupt_one, hand_air, register, summary

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# several chunks writing the same words, gates with and without complement; 128 rows: two waves, 4096: 64
RANDOM = [(5, 65, 3, 128), (6, 130, 5, 256), (8, 300, 5, 4096)]


@functools.lru_cache(maxsize=None)
def replay(key):
    blob, trace, pis = case(key)
    return S.free_cells_replay(register(blob, key[3]), trace, pis)


# 2 rows: 62 idle lanes, and the frames r - 1 and r + 1 coincide; 64: one wave, the wrap stays inside the word; 128: the next-pivot
# frame crosses the wave boundary and wraps from the last word to the first
@pytest.mark.parametrize("n", (2, 64, 128))
def test_hand_written_air(prover, n):
    blob, trace, pis, per_column, mask = hand_air(n)
    air = register(blob, n)
    got = prover.free_cells(air, trace, pis)
    assert np.array_equal(got.per_column, per_column) and np.array_equal(got.mask, mask)
    assert_same(got, S.free_cells_replay(air, trace, pis))
    assert got.mask_words.shape == (6, (n + 63) // 64)
    if n < 64:
        assert all(int(w) >> n == 0 for w in got.mask_words[:, 0])
    bare = prover.free_cells(air, trace, pis, mask=False)
    assert bare.mask is None and summary(bare) == summary(got) and np.array_equal(bare.per_column, got.per_column)


@pytest.mark.parametrize("key", RANDOM, ids=str)
def test_random_air_is_the_replay(prover, key):
    blob, trace, pis = case(key)
    want = replay(key)
    assert 0 < want.free < want.cells and want.partly_free_columns > 0
    air = register(blob, key[3])
    rows = prover.free_cells(air, trace, pis)
    assert_same(rows, want)
    assert_same(prover.free_cells(air, trace.T.copy(), pis, layout=1), want)  # column-major host memory
    assert_same(prover.free_cells(air, trace, pis), rows)  # the same bytes on every run
    other = prover.free_cells(air, trace, pis, delta=3)
    assert_same(other, S.free_cells_replay(air, trace, pis, delta=3))


def test_a_trace_that_violates_the_air(prover):
    key = RANDOM[1]
    blob, trace, pis = case(key)
    air = register(blob, key[3])
    bad = corrupt_one(trace, 10)
    assert prover.check_trace(air, bad, pis)[0] > 0
    want = S.free_cells_replay(air, bad, pis)
    assert not np.array_equal(want.mask, replay(key).mask)
    assert_same(prover.free_cells(air, bad, pis), want)


def test_real_fp12_mul_trace(prover):
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED7200), random_fp12(0x5EED7201))
    assert t.shape == (S.air_default_rows(S.AIR_FP12_MUL), S.air_columns(S.AIR_FP12_MUL))
    want = S.free_cells_replay(S.AIR_FP12_MUL, t, pis)
    got = prover.free_cells(S.AIR_FP12_MUL, t, pis)
    assert_same(got, want)
    assert 0 < got.free < got.cells and got.free_columns >= 1  # one column of FP12Mul is read by no constraint
    assert_same(prover.free_cells(S.AIR_FP12_MUL, t, pis), got)


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first, as in tools/check_trace_bench.py
import starky_bls12_381_amd as S
from free_cells_util import assert_same, case, register
torch.cuda.set_device(0)
key = (6, 130, 5, 256)
blob, trace, pis = case(key)
air = register(blob, key[3])
pv = S.Prover(0)
cols = torch.from_numpy(trace.T.copy().view(np.int64)).to("cuda:0")
rows = torch.from_numpy(trace.copy().view(np.int64)).to("cuda:0")
torch.cuda.synchronize()
want = S.free_cells_replay(air, trace, pis)
got = pv.free_cells_device(air, cols.data_ptr(), key[3], pis, layout=1)
assert_same(got, want)
assert pv.last_call_s > 0
assert_same(pv.free_cells(air, trace, pis), want)
assert_same(pv.free_cells(air, trace.T.copy(), pis, layout=1), want)
assert_same(pv.free_cells_device(air, rows.data_ptr(), key[3], pis, layout=0), want)
assert np.array_equal(cols.cpu().numpy().view(np.uint64), trace.T)  # read in place, left as it was
pv.close()
print("device free cells ok")
"""


def test_trace_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device free cells ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_context_serves_the_checkers_and_a_proof_afterwards(prover):
    key = RANDOM[1]
    blob, trace, pis = case(key)
    air = register(blob, key[3])
    bad = corrupt(trace)
    cfg = S.StarkConfig.standard_fast_config()
    fib, fib_pis = S.trace_fibonacci(3, 5, 256)

    def after(pv):
        rep = pv.check_trace_report(air, bad, pis, cap=1 << 20)
        return (pv.check_trace(air, bad, pis), (rep.violations, rep.constraints_violated, rep.rows_violated), rep.per_constraint.tobytes(),
                rep.row_mask.tobytes(), rep.list.tobytes(), pv.prove(S.AIR_TEST_FIBONACCI, cfg, fib, fib_pis).tobytes())

    fresh = S.Prover(0)
    try:
        want = after(fresh)
    finally:
        fresh.close()
    assert want[0][0] > 0
    first = prover.free_cells(air, trace, pis)
    assert after(prover) == want
    assert_same(prover.free_cells(air, trace, pis), first)  # and the audit after them
