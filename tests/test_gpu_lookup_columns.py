"""starkhip_lookup_columns on the GPU (csrc/lookup_columns.hip over csrc/kernels_multiset.hip: keys and the stable sort, and
csrc/kernels_lookup.hip: mark, scan, the two placements; their tile and workgroup scan are csrc/block_scan.h's): the filled trace and the report equal the Python reference of lookup_ref.py and the C++ replay byte for byte.  The
shapes are where the kernels change shape: 2 rows (four items, less than a wave), 64 (2 n is two waves of one tile), 1024 (2 n fills
exactly two tiles of 1024 items), 4096, 2^14 (32 tiles: the sort's table scan takes its chunk sums and the placement more than one tile
total) and one run at 2^20 (2^21 items, 2048 tiles: the scan of the tile totals walks its row in eight pieces)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import alias_util as A
import lookup_ref as R
import starky_bls12_381_amd as S
from starky_bls12_381_amd.air_builder import AirBuilder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
SIZES = (2, 64, 1024, 4096, 1 << 14)


def _both(prover, trace, lookups, layout=0, cap=1024):
    """the device's trace and report and the replay's, each equal to the reference; and to each other"""
    got, rep = R.run(lambda t, lk, lay, c: prover.lookup_columns(t, lk, layout=lay, cap=c), trace, lookups, layout, cap)
    want, wrep = R.run(lambda t, lk, lay, c: S.lookup_columns_replay(t, lk, layout=lay, cap=c), trace, lookups, layout, cap)
    assert np.array_equal(got, want)
    R.assert_same_report(rep, wrep)
    assert set(rep.timings) == {"upload", "sort", "place", "read_back"} and rep.timings["sort"] > 0
    return got, rep


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_sizes(prover, n, layout):
    a, t = R.data_cases(n, seed=n)["range"]
    _both(prover, R.one_lookup_trace(a, t, seed=n, layout=layout), [R.LOOKUP], layout)
    got, rep = _both(prover, R.shared_table_trace(n, seed=n, fail_first=True, layout=layout), R.SHARED, layout)
    assert rep.per_lookup.tolist() == [2, 0]


def test_a_million_rows(prover):
    n = 1 << 20
    rng = np.random.default_rng(20)
    trace = np.zeros((4, n), dtype=np.uint64)  # column-major
    trace[0] = rng.integers(0, 1 << 16, n, dtype=np.uint64)  # a 16-bit range check ...
    trace[1] = np.arange(n, dtype=np.uint64) % np.uint64(1 << 16)  # ... in a table that holds every value sixteen times
    trace[2:] = 7
    got = trace.copy()
    rep = prover.lookup_columns(got, [R.LOOKUP], layout=1)
    want, per, masks, entries = R.fill(trace, [R.LOOKUP], layout=1)
    assert np.array_equal(got, want)
    R.assert_report(rep, per, masks, entries)
    again = trace.copy()
    R.assert_same_report(prover.lookup_columns(again, [R.LOOKUP], layout=1), rep)
    assert np.array_equal(again, got)
    trace[0][[5, n - 1]] = 1 << 16  # two rows the table lacks
    got = trace.copy()
    rep = prover.lookup_columns(got, [R.LOOKUP], layout=1)
    assert np.array_equal(got, trace) and rep.list.tolist() == [[0, 5], [0, n - 1]] and rep.mask_words.sum() == (1 << 5) + (1 << 63)


def test_data_cases(prover):
    n = 1024
    for name, (a, t) in R.data_cases(n, seed=11).items():
        for layout in (0, 1):
            _, rep = _both(prover, R.one_lookup_trace(a, t, seed=3, layout=layout), [R.LOOKUP], layout)
            assert rep.failed == 0, name
    for name, (a, t, rows) in R.missing_cases(n, seed=12).items():
        got, rep = _both(prover, R.one_lookup_trace(a, t, seed=4), [R.LOOKUP], cap=2048)
        assert rep.list[:, 1].tolist() == rows, name
    _both(prover, R.shared_table_trace(n, seed=13), R.SHARED)
    a, t, _ = R.missing_cases(n, seed=14)["every_row"]
    for cap in (0, 1, 1023):
        _, rep = _both(prover, R.one_lookup_trace(a, t), [R.LOOKUP], cap=cap)
        assert len(rep.list) == cap


def test_cells_at_or_above_p_give_the_canonical_columns(prover):
    n = 1024
    a, t = R.data_cases(n, seed=3)["range"]
    trace = R.one_lookup_trace(a, t, seed=1)
    aliased, _ = A.alias(trace, 1.0, seed=n)
    aliased[:, 2:] = trace[:, 2:]
    A.assert_aliased(aliased[:, :2], trace[:, :2], A.ALL_SMALL_FLOOR)
    got, _ = _both(prover, aliased, [R.LOOKUP])
    plain, _ = _both(prover, trace, [R.LOOKUP])
    assert np.array_equal(got[:, 2:4], plain[:, 2:4]) and not (got[:, 2:4] >= np.uint64(P)).any()


def test_two_calls_give_identical_bytes(prover):
    n = 4096
    trace = R.shared_table_trace(n, seed=21, fail_first=True)
    first, again = trace.copy(), trace.copy()
    rep = prover.lookup_columns(first, R.SHARED)
    R.assert_same_report(prover.lookup_columns(again, R.SHARED), rep)
    assert first.tobytes() == again.tobytes()
    R.assert_same_report(prover.lookup_columns(again, R.SHARED), rep)  # over its own output
    assert first.tobytes() == again.tobytes()


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import lookup_ref as R
import starky_bls12_381_amd as S
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
pv = S.Prover(0)
for n in (64, 1024, 1 << 14):
    for layout in (0, 1):
        for fail in (False, True):
            trace = R.shared_table_trace(n, seed=n + layout, fail_first=fail, layout=layout)
            want, per, masks, entries = R.fill(trace, R.SHARED, layout)
            t = dev(trace)
            torch.cuda.synchronize()
            rep = pv.lookup_columns_device(t.data_ptr(), n, R.SHARED_COLS, R.SHARED, layout=layout)
            R.assert_report(rep, per, masks, entries)
            got = t.cpu().numpy().view(np.uint64)
            assert np.array_equal(got, want)  # the whole trace: only the output columns of lookups that hold differ
            changed = np.flatnonzero((got != trace).any(axis=layout))
            assert set(changed) <= ({5, 6} if fail else {3, 4, 5, 6}) and len(changed)
            host = trace.copy()
            R.assert_same_report(pv.lookup_columns(host, R.SHARED, layout=layout), rep)
            assert np.array_equal(host, got)
pv.close()
print("device forms ok")
"""


def test_traces_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _range_air():
    """7 columns of degree 3: inputs 0 and 1, an 8-bit range table in column 2, the permuted columns 3 .. 6"""
    b = AirBuilder(7, 0, 3)
    b.lookup(0, 2, 3, 4)
    b.lookup(1, 2, 5, 6)
    return S.register_air(b.finish(), name="LookupGpu_range8"), b.lookups


@pytest.mark.parametrize("hasher", (0, 1))
def test_end_to_end(prover, hasher):
    """Fill on the device, then check_trace, check_trace_permutations, prove and verify.  The unfilled trace must not pass: with its
    permuted columns ZERO it satisfies both constraints of each lookup (every factor is 0 - 0) and it is the pairs that fail; with
    the bytes of some other trace in them check_trace fails too."""
    n = 1024
    air, lookups = _range_air()
    assert lookups == R.SHARED
    trace = R.shared_table_trace(n, seed=31)[:, :7].copy()
    empty = trace.copy()
    empty[:, 3:] = 0
    filled = empty.copy()
    rep = prover.lookup_columns(filled, lookups)
    assert rep.failed == 0
    assert prover.check_trace(air, filled, [])[0] == 0
    perm = prover.check_trace_permutations(air, filled)
    assert perm.pairs == 4 and perm.pairs_violated == 0 and perm.pairs_undecided == 0
    assert prover.check_trace_permutations(air, empty).pairs_violated == 4
    assert prover.check_trace(air, trace, [])[0] > 0  # other bytes in the permuted columns
    cfg = S.StarkConfig.standard_fast_config()
    prover.set_option("hasher", hasher)
    try:
        proof = prover.prove(air, cfg, filled, [])
    finally:
        prover.set_option("hasher", 0)
    assert S.proof_hasher(proof) == hasher
    S.verify_stark_proof(air, cfg, proof)
