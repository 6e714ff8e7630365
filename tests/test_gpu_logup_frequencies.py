"""starkhip_logup_frequencies on the GPU (csrc/logup_frequencies.hip over csrc/kernels_multiset.hip: the stable sort of each table, and
csrc/kernels_logup_freq.hip: keys, count, write): the filled trace and the report equal the numpy reference of logup_freq_ref.py and
the C++ replay byte for byte.  The shapes are where the kernels change shape: 2 rows (less than a wave), 64 (one wave, one mask
word), 512 and 2048 (a size on each side of one sort tile of TILE_ITEMS = 1024 items) with 1024 itself (exactly one tile), 2^14 (16
tiles: the sort's table scan takes its chunk sums) and one run at 2^20 (the batch size falls to four lookups there)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import logup_freq_ref as R
import starky_bls12_381_amd as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 64, 512, 1024, 2048, 1 << 14)
TIMINGS = {"upload", "sort", "count", "write", "read_back"}


def registered(m, n_lookups, tables=None):
    lookups, n_cols = R.layout_of(m, n_lookups, tables)
    return S.register_air(R.make_air(n_cols, lookups)), lookups, n_cols


def _both(prover, air, trace, lookups, layout=0, cap=1024):
    """the device's trace and report and the replay's, each equal to the reference; and to each other"""
    got, rep = R.run(lambda a, t, lay, c: prover.logup_frequencies(a, t, layout=lay, cap=c), air, trace, lookups, layout, cap)
    want, wrep = R.run(lambda a, t, lay, c: S.logup_frequencies_replay(a, t, layout=lay, cap=c), air, trace, lookups, layout, cap)
    assert got.tobytes() == want.tobytes()
    R.assert_same_report(rep, wrep)
    assert set(rep.timings) == TIMINGS and rep.timings["sort"] > 0
    return got, rep


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_sizes(prover, n, layout):
    air, lookups, n_cols = registered(3, 3, tables=[1, 14, 1])  # two lookups share a table, one has its own
    for kind in ("uniform", "equal", "duplicates", "big"):
        _both(prover, air, R.make_trace(n, lookups, n_cols, seed=n, kind=kind, layout=layout), lookups, layout)


@pytest.mark.parametrize("combine", (0, 1))
def test_both_forms_of_the_count_give_the_same_bytes(combine):
    air, lookups, n_cols = registered(5, 2)
    pv = S.Prover(0)
    try:
        pv.set_option("logup_count_combine", combine)
        for kind in ("uniform", "equal", "duplicates"):
            _both(pv, air, R.make_trace(2048, lookups, n_cols, seed=combine + 1, kind=kind), lookups)
    finally:
        pv.close()


@pytest.mark.parametrize("layout", (0, 1))
def test_a_failing_lookup_keeps_its_column(prover, layout):
    air, lookups, n_cols = registered(2, 2)
    for n in (64, 2048):
        trace = R.make_trace(n, lookups, n_cols, seed=n, layout=layout)
        v = R.view(trace, layout)
        cols, table, freq = lookups[0]
        v[1, cols[0]], v[n - 1, cols[0]], v[n - 1, cols[1]], v[n // 2, cols[1]] = 3, 3 + R.P, 10 ** 12, 12
        before = v[:, freq].copy()
        for cap in (0, 2, 1024):
            got, rep = _both(prover, air, trace, lookups, layout, cap)
            assert np.array_equal(R.view(got, layout)[:, freq], before)
            assert (rep.failed, rep.missing_cells, rep.missing_rows) == (1, 4, 3) and list(rep.per_column) == [2, 2, 0, 0]
            assert len(rep.list) == min(cap, 3)


def test_sixty_four_lookups_of_sixty_four_rows(prover):
    air, lookups, n_cols = registered(1, 64)
    _both(prover, air, R.make_trace(64, lookups, n_cols, seed=64), lookups)


def test_a_million_rows_twice(prover):
    n = 1 << 20
    air, lookups, n_cols = registered(2, 1)
    cols, table, freq = lookups[0]
    rng = np.random.default_rng(20)
    trace = np.zeros((n_cols, n), dtype=np.uint64)  # column-major
    trace[cols[0]] = rng.integers(0, 1 << 16, n, dtype=np.uint64)     # a 16-bit range check ...
    trace[cols[1]] = 0                                                 # ... and one whose limbs are all 0 ...
    trace[table] = np.arange(n, dtype=np.uint64) % np.uint64(1 << 16)  # ... in a table that holds every value sixteen times
    trace[freq] = 7
    e = R.fill(trace, lookups, layout=1)
    got = trace.copy()
    rep = prover.logup_frequencies(air, got, layout=1)
    R.assert_same(rep, e)
    assert got.tobytes() == e.trace.tobytes()
    assert not got[freq][1 << 16:].any() and int(got[freq].sum()) == 2 * n
    again = trace.copy()
    R.assert_same_report(prover.logup_frequencies(air, again, layout=1), rep)
    assert again.tobytes() == got.tobytes()


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import logup_freq_ref as R
import starky_bls12_381_amd as S
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
pv = S.Prover(0)
lookups, n_cols = R.layout_of(2, 3, tables=[1, 11, 1])
air = S.register_air(R.make_air(n_cols, lookups))
freqs = {f for _, _, f in lookups}
for n in (64, 1024, 1 << 14):
    for layout in (0, 1):
        for fail in (False, True):
            trace = R.make_trace(n, lookups, n_cols, seed=n + layout, kind="duplicates", layout=layout)
            if fail:
                R.view(trace, layout)[n // 3, lookups[1][0][0]] = 1
            e = R.fill(trace, lookups, layout)
            t = dev(trace)
            torch.cuda.synchronize()
            rep = pv.logup_frequencies_device(air, t.data_ptr(), n, n_cols, layout=layout)
            R.assert_same(rep, e)
            got = t.cpu().numpy().view(np.uint64)
            assert got.tobytes() == e.trace.tobytes()  # the whole trace: only the frequencies columns of lookups that hold differ
            changed = set(np.flatnonzero((got != trace).any(axis=layout)))
            assert changed == (freqs - {lookups[1][2]} if fail else freqs), changed
            host = trace.copy()
            R.assert_same_report(pv.logup_frequencies(air, host, layout=layout), rep)
            assert host.tobytes() == got.tobytes()
pv.close()
print("device forms ok")
"""


def test_traces_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
