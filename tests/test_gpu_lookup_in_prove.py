"""The lookups of a trace in batches (csrc/lookup_columns.hip: grid.y = lookup over csrc/kernels_multiset.hip and
csrc/kernels_lookup.hip) and the fill inside prove() and the pools ("fill_lookups" on an AIR registered with its lookups).

Ground truth for columns: tests/lookup_ref.py.  Ground truth for proofs: the path that existed before -- fill with
starkhip_lookup_columns, then prove with the option off.  Rows: 2 (four items, less than a wave), 512 (2 n is exactly one tile of
1024 items), 1024 (two tiles, and input 0 is one value on every row: a run of equal keys over the tile boundary), 4096, 2^14 (the
long LDE path) and, for the fill alone, 2^18 (512 tiles: the scan of the tile totals walks its row in two pieces).  Lookups: 1 and 2
at degree 3, 5 at degree 5 (B = 4; rate_bits 2) -- with "lookup_batch" = 2 those are the uneven batches 2, 2, 1.
A recording is among the trace forms: S.trace_from_writes builds one of any trace whose cells are below 2^32, as these are."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lookup_ref as R
import starky_bls12_381_amd as S
from bls_util import random_fp12
from config_cases import make_config
from starky_bls12_381_amd.air_builder import AirBuilder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# n_cols, degree, lookups: value columns, one or two range tables, the permuted columns (and a bystander for L = 1)
SHAPES = {1: (5, 3, [(0, 1, 2, 3)]),
          2: (7, 3, [(0, 2, 3, 4), (1, 2, 5, 6)]),
          5: (17, 5, [(q, 5 if q < 3 else 6, 7 + 2 * q, 8 + 2 * q) for q in range(5)])}  # lookups 0 .. 2 share table 5, 3 and 4 table 6
L_FOR_ROWS = {2: 1, 512: 2, 1024: 5, 4096: 2, 1 << 14: 5}


def lookup_air(L):
    """-> (the id registered with the lookups, the plain registration of the same blob, lookups, n_cols)"""
    n_cols, degree, lookups = SHAPES[L]
    b = AirBuilder(n_cols, 0, degree)
    for lk in lookups:
        b.lookup(*lk)
    blob = b.finish()
    assert b.lookups == lookups
    return S.register_air(blob, name=f"LookupFill_{L}", lookups=b.lookups), S.register_air(blob, name=f"LookupPlain_{L}"), lookups, n_cols


def lookup_trace(L, n, seed, fail=()):
    """[n][C], every cell below 2^32: inputs below m = min(n, 256) -- input 0 one value on every row -- the tables hold 0 .. m - 1, the
    permuted columns garbage (non-zero, no witness); fail: (lookup, row) whose input cell gets a value the table lacks"""
    n_cols, _, lookups = SHAPES[L]
    rng = np.random.default_rng(seed)
    m = min(n, 256)
    t = rng.integers(1, 1 << 31, (n, n_cols), dtype=np.uint64)
    for q, (i, tab, _, _) in enumerate(lookups):
        t[:, i] = m // 2 if q == 0 else rng.integers(0, m, n, dtype=np.uint64)
    for k, tab in enumerate(sorted({lk[1] for lk in lookups})):
        col = np.arange(n, dtype=np.uint64) % np.uint64(m)
        t[:, tab] = col if k == 0 else rng.permutation(col)
    for q, r in fail:
        t[r, lookups[q][0]] = m + 7 + q
    return t


def config_for(air, n):
    # (two rows at standard_fast's cap height are no shape: a smaller cap, as tests/config_cases.py has for log_n = 1)
    return make_config(2, 3, 2, 0, 2, 0) if n == 2 else S.StarkConfig.for_air(air)


def _writes(trace):
    r, c = np.nonzero(trace)
    return np.stack([r.astype(np.uint64), c.astype(np.uint64), trace[r, c]], axis=1)


@pytest.fixture(scope="module")
def filler():
    """a second context with "fill_lookups" on; the session's `prover` has it off and gives the reference bytes"""
    p = S.Prover(0)
    p.set_option("fill_lookups", 1)
    yield p
    p.close()


_cases = {}


def case(prover, n, hasher=0):
    """(air, plain, lookups, cfg, the garbage trace, the filled trace, the proof of the filled trace with the option off), computed once"""
    if (n, hasher) not in _cases:
        L = L_FOR_ROWS[n]
        air, plain, lookups, _ = lookup_air(L)
        cfg = config_for(air, n)
        garbage = lookup_trace(L, n, seed=n)
        want_cols, per, _, _ = R.fill(garbage, lookups)
        assert sum(per) == 0
        filled = garbage.copy()
        assert prover.lookup_columns(filled, lookups).failed == 0
        assert np.array_equal(filled, want_cols)
        prover.set_option("hasher", hasher)
        try:
            want = prover.prove(air, cfg, filled, [])
        finally:
            prover.set_option("hasher", 0)
        garbage.setflags(write=False)
        filled.setflags(write=False)
        _cases[(n, hasher)] = (air, plain, lookups, cfg, garbage, filled, want)
    return _cases[(n, hasher)]


# ------------------------------------------------------------------------------------------------ the fill alone, in batches
@pytest.mark.parametrize("batch", (2, 0, 1))
@pytest.mark.parametrize("n", (2, 512, 1024))
def test_batched_fill_of_host_traces(filler, n, batch):
    """the staged path: [G][4][n] go up, two columns per holding lookup come back; lookup 2, in the middle of a batch, fails"""
    lookups = SHAPES[5][2]
    filler.set_option("lookup_batch", batch)
    try:
        for layout in (0, 1):
            for fail in ((), ((2, n - 1),), ((0, 0), (4, 1))):
                t = lookup_trace(5, n, seed=n + layout, fail=fail)
                t = np.ascontiguousarray(t.T) if layout else t
                got, rep = R.run(lambda a, lk, lay, c: filler.lookup_columns(a, lk, layout=lay, cap=c), t, lookups, layout)
                want, wrep = R.run(lambda a, lk, lay, c: S.lookup_columns_replay(a, lk, layout=lay, cap=c), t, lookups, layout)
                assert np.array_equal(got, want)
                R.assert_same_report(rep, wrep)
                assert rep.per_lookup.tolist() == [1 if any(q == f[0] for f in fail) else 0 for q in range(5)]
    finally:
        filler.set_option("lookup_batch", 0)
    for bad in (-1, 65):
        with pytest.raises(S.StarkhipError) as e:
            filler.set_option("lookup_batch", bad)
        assert e.value.code == S.ERR_BAD_SHAPE


FILL_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(150, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import lookup_ref as R
import starky_bls12_381_amd as S
from test_gpu_lookup_in_prove import SHAPES, lookup_trace
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.array(a, order="C", copy=True).view(np.int64)).to("cuda:0")
pv = S.Prover(0)
C, _, lookups = SHAPES[5]
for n, batches in ((2, (2, 0)), (512, (2, 0)), (1024, (2, 0)), (1 << 18, (0,))):
    for fail in ((), ((3, n // 2),)):  # lookup 3: the second of the batch 2, 3 -- its neighbours are written, its own columns are not
        trace = np.ascontiguousarray(lookup_trace(5, n, seed=n, fail=fail).T)  # column-major
        want, per, masks, entries = R.fill(trace, lookups, layout=1)
        replayed = trace.copy()
        wrep = S.lookup_columns_replay(replayed, lookups, layout=1)
        assert np.array_equal(replayed, want)
        for batch in batches:
            pv.set_option("lookup_batch", batch)
            for layout in ((1, 0) if n <= 1024 else (1,)):
                arg = trace if layout else np.ascontiguousarray(trace.T)
                t = dev(arg)
                torch.cuda.synchronize()
                rep = pv.lookup_columns_device(t.data_ptr(), n, C, lookups, layout=layout)
                R.assert_report(rep, per, masks, entries)
                R.assert_same_report(rep, wrep)
                got = t.cpu().numpy().view(np.uint64)
                got = got if layout else got.T
                assert np.array_equal(got, want), (n, batch, layout)  # every cell: the untouched ones are as they were
                changed = set(np.flatnonzero((got != trace).any(axis=1)).tolist())
                assert changed == {c for q, lk in enumerate(lookups) for c in lk[2:] if not per[q]}, (n, batch, changed)
pv.close()
print("batched fill ok")
"""


def test_batched_fill_of_device_traces():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", FILL_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "batched fill ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ proof bytes
@pytest.mark.parametrize("hasher", (0, 1))
@pytest.mark.parametrize("n", sorted(L_FOR_ROWS))
def test_proof_bytes_of_every_host_form(prover, filler, n, hasher):
    air, plain, lookups, cfg, garbage, filled, want = case(prover, n, hasher)
    C = garbage.shape[1]
    filler.set_option("hasher", hasher)
    filler.set_option("lookup_batch", 2 if n == 1024 else 0)  # five lookups as 2, 2, 1 once
    try:
        before = garbage.copy()
        proofs = {"rows": filler.prove(air, cfg, garbage, []),
                  "columns": filler.prove(air, cfg, np.ascontiguousarray(garbage.T), [], layout=1),
                  "column table": filler.prove_columns(air, cfg, [garbage[:, c].copy() for c in range(C)], []),
                  "recording": filler.prove(air, cfg, S.trace_from_writes(n, C, _writes(garbage)), [])}
        assert np.array_equal(garbage, before)
    finally:
        filler.set_option("hasher", 0)
        filler.set_option("lookup_batch", 0)
    for form, proof in proofs.items():
        assert np.array_equal(proof, want), form
    assert S.proof_hasher(want) == hasher
    S.verify_stark_proof(plain, cfg, proofs["rows"])
    ms = filler.last_lookup_timings()
    assert ms["sort"] > 0 and filler.last_timings()["upload"] >= ms["sort"]  # the last fill of the context, inside phase 0


def test_the_plain_registration_proves_the_same_bytes(prover):
    air, plain, lookups, cfg, garbage, filled, want = case(prover, 512)
    assert np.array_equal(prover.prove(plain, cfg, filled, []), want)
    S.verify_stark_proof(air, cfg, want)


PROVE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(150, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import starky_bls12_381_amd as S
from test_gpu_lookup_in_prove import case
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.array(a, order="C", copy=True).view(np.int64)).to("cuda:0")
ref, pv = S.Prover(0), S.Prover(0)
pv.set_option("fill_lookups", 1)
for hasher in (0, 1):
    for n in (2, 512, 1024, 4096, 1 << 14):
        air, plain, lookups, cfg, garbage, filled, want = case(ref, n, hasher)
        pv.set_option("hasher", hasher)
        for layout in (0, 1):
            arg = np.ascontiguousarray(garbage.T) if layout else np.ascontiguousarray(garbage)
            t = dev(arg)
            torch.cuda.synchronize()
            proof = pv.prove_device(air, cfg, t.data_ptr(), n, [], layout=layout)
            assert np.array_equal(proof, want), (hasher, n, layout)
            assert np.array_equal(t.cpu().numpy().view(np.uint64), arg), (hasher, n, layout)  # the caller's tensor is only read
        S.verify_stark_proof(plain, cfg, proof)
ref.close()
pv.close()
print("device forms ok")
"""


def test_proof_bytes_of_device_tensors():
    r = subprocess.run([sys.executable, "-c", PROVE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "device forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ order, and AIRs without a list
def test_the_fill_runs_before_the_check(prover, filler):
    air, plain, lookups, cfg, garbage, filled, want = case(prover, 1024)
    filler.set_option("check_trace", 1)
    try:
        before = filler.check_stats()
        assert np.array_equal(filler.prove(air, cfg, garbage, []), want)  # the check saw the filled columns
        assert filler.check_stats() == {"checked": before["checked"] + 1, "rejected": before["rejected"]}
        filler.set_option("fill_lookups", 0)
        with pytest.raises(S.TraceViolation) as e:
            filler.prove(air, cfg, garbage, [])
        assert int(e.value.blob[0]) == S.CHECK_MAGIC and e.value.report.violations > 0 and e.value.lookup_report is None
        assert np.array_equal(e.value.blob, S.check_blob_replay(air, garbage, []))
        # the plain registration has nothing to fill: refused by the check too, with the option on
        filler.set_option("fill_lookups", 1)
        with pytest.raises(S.TraceViolation) as e:
            filler.prove(plain, cfg, garbage, [])
        assert int(e.value.blob[0]) == S.CHECK_MAGIC
    finally:
        filler.set_option("check_trace", 0)
        filler.set_option("fill_lookups", 1)


def test_nothing_changes_where_there_is_no_list(prover, filler):
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED7400), random_fp12(0x5EED7401))
    cfg = S.StarkConfig.for_air(S.AIR_FP12_MUL)
    assert np.array_equal(filler.prove(S.AIR_FP12_MUL, cfg, t, pis), prover.prove(S.AIR_FP12_MUL, cfg, t, pis))
    t, pis = S.trace_fibonacci(0, 1, 64)
    cfg = S.StarkConfig.standard_fast_config()
    assert np.array_equal(filler.prove(S.AIR_TEST_FIBONACCI, cfg, t, pis), prover.prove(S.AIR_TEST_FIBONACCI, cfg, t, pis))
    air, plain, lookups, cfg, garbage, filled, want = case(prover, 512)
    for p in (filler, prover):  # unfilled columns under the plain id: the Zs do not close, as without the option
        with pytest.raises(S.StarkhipError) as e:
            p.prove(plain, cfg, garbage, [])
        assert e.value.code == S.ERR_QUOTIENT_NOT_DIVISIBLE
    assert np.array_equal(filler.prove(plain, cfg, filled, []), want)
    for bad in (2, -1):
        with pytest.raises(S.StarkhipError) as e:
            filler.set_option("fill_lookups", bad)
        assert e.value.code == S.ERR_BAD_SHAPE


# ------------------------------------------------------------------------------------------------ refusal
@pytest.mark.parametrize("n", (512, 1024))
def test_a_failing_lookup_is_refused_with_the_lookup_blob(prover, filler, n):
    air, plain, lookups, cfg, garbage, filled, want = case(prover, n)
    L = len(lookups)
    bad = lookup_trace(L, n, seed=n, fail=((L - 1, 3), (0, n - 1), (L - 1, n - 2)))  # the first and the last lookup fail, the others hold
    for cap in (16, 1, 0):
        filler.set_option("check_trace_list", cap)
        try:
            before = filler.check_stats()
            for call in (lambda: filler.prove(air, cfg, bad, []),
                         lambda: filler.prove(air, cfg, np.ascontiguousarray(bad.T), [], layout=1),
                         lambda: filler.prove_columns(air, cfg, [bad[:, c].copy() for c in range(bad.shape[1])], [])):
                with pytest.raises(S.TraceViolation) as e:
                    call()
                assert e.value.code == S.ERR_TRACE and e.value.report is None
                assert np.array_equal(e.value.blob, S.lookup_blob_replay(air, bad, cap=cap))
                rep = e.value.lookup_report
                assert (rep.air, rep.n_rows, rep.lookups, rep.failed, rep.missing_rows) == (air, n, L, 2, 3)
                assert rep.list.tolist() == [[0, n - 1], [L - 1, 3], [L - 1, n - 2]][:cap]
            after = filler.check_stats()
            assert (after["checked"], after["rejected"]) == (before["checked"] + 3, before["rejected"] + 3)
        finally:
            filler.set_option("check_trace_list", 16)
    assert np.array_equal(filler.prove(air, cfg, garbage, []), want)  # the context is as usable as before


# ------------------------------------------------------------------------------------------------ pools
def test_pool_fills_checks_and_verifies(prover):
    n = 512
    air, plain, lookups, cfg, garbage, filled, want = case(prover, n)
    other = lookup_trace(2, n, seed=77)
    other_filled = other.copy()
    assert prover.lookup_columns(other_filled, lookups).failed == 0
    want_other = prover.prove(air, cfg, other_filled, [])
    bad = lookup_trace(2, n, seed=78, fail=((1, 100),))
    blob = S.lookup_blob_replay(air, bad)
    assert blob is not None
    pool = S.ProofPool(0, big_contexts=1, small_contexts=2, verify_proofs=True)
    try:
        pool.set_option("fill_lookups", 1)
        pool.set_option("check_traces", 1)
        for value in (2, -1):
            with pytest.raises(S.StarkhipError) as e:
                pool.set_option("fill_lookups", value)
            assert e.value.code == S.ERR_BAD_SHAPE
        tickets = [pool.submit(air, cfg, garbage, []),
                   pool.submit_columns(air, cfg, [other[:, c].copy() for c in range(other.shape[1])], []),
                   pool.submit(air, cfg, np.ascontiguousarray(bad.T), [], layout=1),
                   pool.submit_columns(air, cfg, [garbage[:, c].copy() for c in range(garbage.shape[1])], [])]
        assert np.array_equal(pool.wait(tickets[0])[0], want)
        assert np.array_equal(pool.wait(tickets[1])[0], want_other)
        with pytest.raises(S.TraceViolation) as e:
            pool.wait(tickets[2])
        assert np.array_equal(e.value.blob, blob) and e.value.lookup_report.list.tolist() == [[1, 100]]
        assert np.array_equal(pool.wait(tickets[3])[0], want)
        assert pool.check_stats() == {"checked": 4, "rejected": 1}
        st = pool.verify_stats()
        assert st["proofs_checked"] == 3 and st["rejected"] == 0  # the refused trace never reached the verifier
        # read at submit: with the option off the garbage trace is what it is to a pool today -- refused by the check
        pool.set_option("fill_lookups", 0)
        with pytest.raises(S.TraceViolation) as e:
            pool.wait(pool.submit(air, cfg, garbage, []))
        assert int(e.value.blob[0]) == S.CHECK_MAGIC
    finally:
        pool.close()
