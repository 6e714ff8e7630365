"""The fill of LogUp frequencies inside prove() and the pools ("fill_frequencies" on a fillable AIR with LogUp lookups;
csrc/logup_frequencies.hip: logup_fill_in_prove).

The AIR and traces are logup_ref.make_air / make_trace at degree 3 with m = 3 and two lookups: their table values are distinct, so
numpy's bincount -- which make_trace fills the frequencies with -- IS the rule.  Ground truth for proofs: the path that existed
before, the numpy-filled trace proved with the option off.  Rows: 64 and 2^14 (the long LDE path, sixteen sort tiles).
Trace forms: host rows, host columns, a column table and device tensors in both layouts.  A recording holds cells below 2^32 only,
which make_trace's own columns (squares and cubes mod p) are not: the recording (prove_compact) is proved on
logup_freq_ref.make_air / make_trace, whose cells are all small and whose own constraints hold with PI0 = 7; its table has
duplicates, so there the ground truth for the column is logup_freq_ref.fill."""
import os
import subprocess
import sys

import numpy as np
import pytest

import logup_ref as R
import starky_bls12_381_amd as S
from logup_util import logup_air, logup_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEGREE, M, LOOKUPS = 3, 3, 2
ROWS = (64, 1 << 14)
FREQS = [R.lookup_columns(M, l)[1] for l in range(LOOKUPS)]


@pytest.fixture(scope="module")
def filler():
    """a second context with "fill_frequencies" on; the session's `prover` has it off and gives the reference bytes"""
    p = S.Prover(0)
    p.set_option("fill_frequencies", 1)
    yield p
    p.close()


_cases = {}


def case(prover, n, hasher=0):
    """(air, blob, cfg, public inputs, the trace with ZEROED frequencies, the numpy-filled trace, its proof with the option off), once"""
    if (n, hasher) not in _cases:
        air, blob = logup_air(DEGREE, M, LOOKUPS)
        cfg = logup_config(DEGREE, 3)
        filled, pis = R.make_trace(DEGREE, M, LOOKUPS, n, seed=n + 1)
        zeroed = filled.copy()
        zeroed[:, FREQS] = 0
        prover.set_option("hasher", hasher)
        try:
            want = prover.prove(air, cfg, filled, pis)
        finally:
            prover.set_option("hasher", 0)
        filled.setflags(write=False)
        zeroed.setflags(write=False)
        _cases[(n, hasher)] = (air, blob, cfg, pis, zeroed, filled, want)
    return _cases[(n, hasher)]


def bad_trace(zeroed, n):
    """one limb outside the table: lookup 1, row n - 3, its second column"""
    bad = zeroed.copy()
    bad[n - 3, R.lookup_columns(M, 1)[0][1]] = 3  # the table's values are 11 + 5 k
    return bad


@pytest.mark.parametrize("n", ROWS)
def test_without_the_option_zeroed_frequencies_do_not_close(prover, n):
    air, blob, cfg, pis, zeroed, filled, want = case(prover, n)
    with pytest.raises(S.StarkhipError) as e:
        prover.prove(air, cfg, zeroed, pis)
    assert e.value.code == S.ERR_QUOTIENT_NOT_DIVISIBLE


@pytest.mark.parametrize("hasher", (0, 1))
@pytest.mark.parametrize("n", ROWS)
def test_proof_bytes_of_every_host_form(prover, filler, n, hasher):
    air, blob, cfg, pis, zeroed, filled, want = case(prover, n, hasher)
    C = zeroed.shape[1]
    filler.set_option("hasher", hasher)
    try:
        before = zeroed.copy()
        proofs = {"rows": filler.prove(air, cfg, zeroed, pis),
                  "columns": filler.prove(air, cfg, np.ascontiguousarray(zeroed.T), pis, layout=1),
                  "column table": filler.prove_columns(air, cfg, [zeroed[:, c].copy() for c in range(C)], pis),
                  "filled already": filler.prove(air, cfg, filled, pis)}
        assert np.array_equal(zeroed, before)
    finally:
        filler.set_option("hasher", 0)
    for form, proof in proofs.items():
        assert proof.tobytes() == want.tobytes(), form
    assert S.proof_hasher(want) == hasher
    S.verify_stark_proof(air, cfg, proofs["rows"])
    if n == 64:
        R.verify_or_raise(blob, cfg, proofs["rows"], hasher)
    ms = filler.last_logup_frequency_timings()
    assert ms["sort"] > 0 and filler.last_timings()["upload"] >= ms["sort"]  # the last fill of the context, inside phase 0


PROVE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(150, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import starky_bls12_381_amd as S
from test_gpu_logup_fill_in_prove import ROWS, case
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.array(a, order="C", copy=True).view(np.int64)).to("cuda:0")
ref, pv = S.Prover(0), S.Prover(0)
pv.set_option("fill_frequencies", 1)
for n in ROWS:
    air, blob, cfg, pis, zeroed, filled, want = case(ref, n)
    for layout in (0, 1):
        arg = np.ascontiguousarray(zeroed.T) if layout else np.ascontiguousarray(zeroed)
        t = dev(arg)
        torch.cuda.synchronize()
        proof = pv.prove_device(air, cfg, t.data_ptr(), n, pis, layout=layout)
        assert proof.tobytes() == want.tobytes(), (n, layout)
        assert np.array_equal(t.cpu().numpy().view(np.uint64), arg), (n, layout)  # the caller's tensor is only read
    S.verify_stark_proof(air, cfg, proof)
ref.close()
pv.close()
print("device forms ok")
"""


def test_proof_bytes_of_device_tensors():
    r = subprocess.run([sys.executable, "-c", PROVE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "device forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_fill_runs_before_the_check(prover, filler):
    air, blob, cfg, pis, zeroed, filled, want = case(prover, 64)
    filler.set_option("check_trace", 1)
    try:
        before = filler.check_stats()
        assert filler.prove(air, cfg, zeroed, pis).tobytes() == want.tobytes()
        assert filler.check_stats() == {"checked": before["checked"] + 1, "rejected": before["rejected"]}
    finally:
        filler.set_option("check_trace", 0)
    for bad in (2, -1):
        with pytest.raises(S.StarkhipError) as e:
            filler.set_option("fill_frequencies", bad)
        assert e.value.code == S.ERR_BAD_SHAPE


def test_an_air_that_is_not_fillable_is_refused_and_others_are_untouched(prover, filler):
    import logup_freq_ref as F
    lookups = [([2, 3], 1, 4), ([4], 1, 5)]  # lookup 1 looks lookup 0's frequencies up
    air = S.register_air(F.make_air(6, lookups))
    t = np.zeros((64, 6), dtype=np.uint64)
    t[:, 0] = np.arange(64) + 1
    with pytest.raises(S.StarkhipError) as e:
        filler.prove(air, logup_config(3, 3), t, [1])
    assert e.value.code == S.ERR_BAD_AIR
    t, pis = S.trace_fibonacci(0, 1, 64)  # an AIR without LogUp lookups: nothing changes
    cfg = S.StarkConfig.standard_fast_config()
    assert np.array_equal(filler.prove(S.AIR_TEST_FIBONACCI, cfg, t, pis), prover.prove(S.AIR_TEST_FIBONACCI, cfg, t, pis))


@pytest.mark.parametrize("n", ROWS)
def test_a_cell_outside_the_table_is_refused_with_the_logup_blob(prover, filler, n):
    air, blob, cfg, pis, zeroed, filled, want = case(prover, n)
    bad = bad_trace(zeroed, n)
    for cap in (16, 0):
        filler.set_option("check_trace_list", cap)
        try:
            before = filler.check_stats()
            for call in (lambda: filler.prove(air, cfg, bad, pis),
                         lambda: filler.prove(air, cfg, np.ascontiguousarray(bad.T), pis, layout=1),
                         lambda: filler.prove_columns(air, cfg, [bad[:, c].copy() for c in range(bad.shape[1])], pis)):
                with pytest.raises(S.TraceViolation) as e:
                    call()
                assert e.value.code == S.ERR_TRACE and e.value.report is None and e.value.lookup_report is None
                assert e.value.blob.tobytes() == S.logup_blob_replay(air, bad, cap=cap).tobytes()
                rep = e.value.logup_report
                assert (rep.air, rep.n_rows, rep.lookups, rep.failed, rep.missing_cells, rep.missing_rows) == (air, n, LOOKUPS, 1, 1, 1)
                assert rep.list.tolist() == [[1, n - 3]][:cap]
            after = filler.check_stats()
            assert (after["checked"], after["rejected"]) == (before["checked"] + 3, before["rejected"] + 3)
        finally:
            filler.set_option("check_trace_list", 16)
    assert filler.prove(air, cfg, zeroed, pis).tobytes() == want.tobytes()  # the context is as usable as before


def _writes(trace):
    r, c = np.nonzero(trace)
    return np.stack([r.astype(np.uint64), c.astype(np.uint64), trace[r, c]], axis=1)


@pytest.mark.parametrize("n", ROWS)
def test_a_recording_is_filled_and_a_failing_one_refused(prover, filler, n):
    import logup_freq_ref as F
    lookups, C = F.layout_of(2, 3, tables=[1, 11, 1])  # two lookups share table 1, one has table 11
    air = S.register_air(F.make_air(C, lookups))
    cfg, pis = logup_config(3, 3), [7]
    zeroed = F.make_trace(n, lookups, C, seed=n, kind="duplicates")
    zeroed[:, [f for _, _, f in lookups]] = 0
    assert int(zeroed.max()) < 1 << 32
    filled = F.fill(zeroed, lookups).trace
    assert not np.array_equal(filled, zeroed)
    want = prover.prove(air, cfg, filled, pis)
    S.verify_stark_proof(air, cfg, want)
    with pytest.raises(S.StarkhipError) as e:
        prover.prove(air, cfg, S.trace_from_writes(n, C, _writes(zeroed)), pis)
    assert e.value.code == S.ERR_QUOTIENT_NOT_DIVISIBLE
    assert filler.prove(air, cfg, S.trace_from_writes(n, C, _writes(zeroed)), pis).tobytes() == want.tobytes()
    assert filler.prove(air, cfg, zeroed, pis).tobytes() == want.tobytes()
    bad = zeroed.copy()
    bad[n - 2, lookups[2][0][0]] = 1  # the tables' values are 5 + 3 k
    bad[5, lookups[1][0][1]] = 2
    with pytest.raises(S.TraceViolation) as e:
        filler.prove(air, cfg, S.trace_from_writes(n, C, _writes(bad)), pis)
    assert e.value.blob.tobytes() == S.logup_blob_replay(air, bad).tobytes()
    rep = e.value.logup_report
    assert (rep.failed, rep.missing_cells, rep.missing_rows) == (2, 2, 2) and rep.list.tolist() == [[1, 5], [2, n - 2]]
    assert filler.prove(air, cfg, S.trace_from_writes(n, C, _writes(zeroed)), pis).tobytes() == want.tobytes()


def test_pool_fills_and_hands_the_blob_through_wait(prover):
    n = 64
    air, blob, cfg, pis, zeroed, filled, want = case(prover, n)
    bad = bad_trace(zeroed, n)
    want_blob = S.logup_blob_replay(air, bad)
    pool = S.ProofPool(0, big_contexts=1, small_contexts=1, verify_proofs=True)
    try:
        pool.set_option("fill_frequencies", 1)
        for value in (2, -1):
            with pytest.raises(S.StarkhipError) as e:
                pool.set_option("fill_frequencies", value)
            assert e.value.code == S.ERR_BAD_SHAPE
        assert pool.wait(pool.submit(air, cfg, zeroed, pis))[0].tobytes() == want.tobytes()
        # Nothing grows from proof to proof.  That no buffer grows INSIDE a proof is not this reading's to show: the fill inside
        # prove() allocates nothing at all -- it takes what work_buffers() has listed and ensured before the first phase and returns
        # an error when a buffer is not there -- so every filling proof of this file fails if the fill's buffers are not listed.
        held = pool.reservation()["device_bytes"]
        tickets = [pool.submit(air, cfg, zeroed, pis),
                   pool.submit(air, cfg, np.ascontiguousarray(bad.T), pis, layout=1),
                   pool.submit_columns(air, cfg, [zeroed[:, c].copy() for c in range(zeroed.shape[1])], pis)]
        assert pool.wait(tickets[0])[0].tobytes() == want.tobytes()
        with pytest.raises(S.TraceViolation) as e:
            pool.wait(tickets[1])
        assert e.value.blob.tobytes() == want_blob.tobytes() and e.value.logup_report.list.tolist() == [[1, n - 3]]
        assert pool.wait(tickets[2])[0].tobytes() == want.tobytes()
        assert pool.reservation()["device_bytes"] == held
        assert pool.check_stats()["rejected"] == 1
        assert pool.verify_stats()["proofs_checked"] == 3  # the refused trace never reached the verifier
        # read at submit: with the option off the zeroed trace is what it is to a pool today
        pool.set_option("fill_frequencies", 0)
        with pytest.raises(S.StarkhipError) as e:
            pool.wait(pool.submit(air, cfg, zeroed, pis))
        assert e.value.code == S.ERR_QUOTIENT_NOT_DIVISIBLE
    finally:
        pool.close()
