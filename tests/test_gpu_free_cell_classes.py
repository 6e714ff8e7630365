"""starkhip_check_trace_free_cell_classes on the device (kernels_free_classes.hip) against its host replay, bit for bit: a hand-written
AIR whose classes are known by construction, random AIRs of 128 to 4096 rows, a violating trace, cells at or above p, a trace in
device memory, the audit as the projection of the classes, and the context shared with the audit, the checkers and a proof."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import starky_bls12_381_amd as S
from check_report_util import corrupt
from free_cell_classes_util import assert_classes, assert_same, assert_same_counts, hand_air
from free_cells_util import P, case, corrupt_one, register
from free_cells_util import assert_same as assert_same_audit
from free_cells_util import summary as summary_audit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# several chunks writing the same words, gates with and without complement; 128 rows: two waves, 4096: 64 waves per chunk
RANDOM = [(5, 65, 3, 128), (6, 130, 5, 256), (8, 300, 5, 4096)]


@functools.lru_cache(maxsize=None)
def replay(key):
    blob, trace, pis = case(key)
    return S.free_cell_classes_replay(register(blob, key[3]), trace, pis)


# 2 rows: 62 idle lanes, and the frames r - 1 and r + 1 coincide; 64: one wave; 128: the next-pivot frame crosses the wave boundary
# and wraps from the last word to the first
@pytest.mark.parametrize("n", (2, 64, 128))
def test_hand_written_air(prover, n):
    h = hand_air(n)
    air = register(h.blob, n)
    got = prover.free_cell_classes(air, h.trace, h.pis)
    assert_classes(got, h)
    assert_same(got, S.free_cell_classes_replay(air, h.trace, h.pis))
    assert_same(prover.free_cell_classes(air, h.trace.T.copy(), h.pis, layout=1), got)
    assert_same_counts(prover.free_cell_classes(air, h.trace, h.pis, planes=False), got)


@pytest.mark.parametrize("key", RANDOM, ids=str)
def test_random_air_is_the_replay(prover, key):
    blob, trace, pis = case(key)
    want = replay(key)
    assert min(want.n_caught, want.n_silent, want.n_gated, want.n_unread) > 0 and want.constraints_never_open > 0
    air = register(blob, key[3])
    rows = prover.free_cell_classes(air, trace, pis)
    assert_same(rows, want)
    assert_same(prover.free_cell_classes(air, trace.T.copy(), pis, layout=1), want)  # column-major host memory
    assert_same(prover.free_cell_classes(air, trace, pis), rows)  # the same bytes on every run
    assert_same(prover.free_cell_classes(air, trace, pis, delta=3), S.free_cell_classes_replay(air, trace, pis, delta=3))
    assert_same_counts(prover.free_cell_classes(air, trace, pis, planes=False), want)


def test_a_trace_that_violates_the_air(prover):
    key = RANDOM[1]
    blob, trace, pis = case(key)
    air = register(blob, key[3])
    bad = corrupt_one(trace, 10)
    assert prover.check_trace(air, bad, pis)[0] > 0
    want = S.free_cell_classes_replay(air, bad, pis)
    assert want.plane_words.tobytes() != replay(key).plane_words.tobytes() and not np.array_equal(want.open_rows, replay(key).open_rows)
    assert_same(prover.free_cell_classes(air, bad, pis), want)


def test_cells_at_or_above_p(prover):
    key = RANDOM[0]
    blob, trace, pis = case(key)
    aliased = trace.copy()
    small = aliased < np.uint64((1 << 64) - P)  # c + p still fits a word
    assert small.any() and (aliased == 0).any()
    aliased[small] += np.uint64(P)
    air = register(blob, key[3])
    assert_same(prover.free_cell_classes(air, aliased, pis), replay(key))
    assert_same(prover.free_cell_classes(air, aliased.T.copy(), pis, layout=1), replay(key))


# The audit's device entry is the classes' run and a projection of it on the host: the caught plane alone is read back and complemented
# on the live rows in the caller's buffer, per_column is the sum of the three class counts.  The shapes are the ones the projection
# itself can go wrong at -- 2 rows: one word per column, whose 62 high bits have to stay zero after the complement; 64: a full word;
# 128: two words; and the random AIRs, up to 64 words per column and several chunks.
@pytest.mark.parametrize("shape", [2, 64, 128] + RANDOM, ids=str)
def test_the_audit_is_the_projection_of_the_classes(prover, shape):
    if isinstance(shape, int):
        h = hand_air(shape)
        blob, trace, pis, n = h.blob, h.trace, h.pis, shape
    else:
        (blob, trace, pis), n = case(shape), shape[3]
    air = register(blob, n)
    audit = prover.free_cells(air, trace, pis)
    got = prover.free_cell_classes(air, trace, pis)
    live = np.uint64((1 << min(n, 64)) - 1)
    assert got.plane_words[2].shape == audit.mask_words.shape == (trace.shape[1], (n + 63) // 64)
    assert ((got.plane_words[2] ^ audit.mask_words) == live).all()
    assert np.array_equal(got.per_column.sum(axis=1, dtype=np.uint32), audit.per_column)
    bare = prover.free_cells(air, trace, pis, mask=False)  # no plane read back: the same counts and summary
    assert bare.mask is None and summary_audit(bare) == summary_audit(audit) and np.array_equal(bare.per_column, audit.per_column)


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first, as in tools/check_trace_bench.py
import starky_bls12_381_amd as S
from free_cell_classes_util import assert_same, assert_same_counts
from free_cells_util import case, register
torch.cuda.set_device(0)
key = (6, 130, 5, 256)
blob, trace, pis = case(key)
air = register(blob, key[3])
pv = S.Prover(0)
cols = torch.from_numpy(trace.T.copy().view(np.int64)).to("cuda:0")
rows = torch.from_numpy(trace.copy().view(np.int64)).to("cuda:0")
torch.cuda.synchronize()
want = S.free_cell_classes_replay(air, trace, pis)
got = pv.free_cell_classes_device(air, cols.data_ptr(), key[3], pis, layout=1)
assert_same(got, want)
assert pv.last_call_s > 0
assert_same(pv.free_cell_classes_device(air, rows.data_ptr(), key[3], pis, layout=0), want)
assert_same_counts(pv.free_cell_classes_device(air, cols.data_ptr(), key[3], pis, layout=1, planes=False), want)
assert np.array_equal(cols.cpu().numpy().view(np.uint64), trace.T)  # read in place, left as it was
assert np.array_equal(rows.cpu().numpy().view(np.uint64), trace)
pv.close()
print("device free cell classes ok")
"""


def test_trace_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device free cell classes ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_one_context_serves_both_audits_the_checkers_and_a_proof(prover):
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
        audit = fresh.free_cells(air, trace, pis)
        want = after(fresh)
    finally:
        fresh.close()
    assert want[0][0] > 0
    assert_same_audit(prover.free_cells(air, trace, pis), audit)
    got = prover.free_cell_classes(air, trace, pis)
    assert_same(got, replay(key))
    assert_same_audit(prover.free_cells(air, trace, pis), audit)  # the audit after the classes: the same buffers and compiled form
    assert np.array_equal(got.caught, ~audit.mask)
    assert after(prover) == want
    assert_same(prover.free_cell_classes(air, trace, pis), got)  # and the classes after them
