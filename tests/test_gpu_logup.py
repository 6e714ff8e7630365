"""LogUp lookups of registered AIRs on the GPU (COMPAT.md L1 - L7): the kernels of csrc/kernels_logup.hip against the Python reference
of tests/logup_ref.py, byte for byte, and whole proofs of AIRs with LogUp lookups -- degree 2, 3 and 5, both hashers, both quotient
evaluators, a pool -- through the product's CPU verifier, its device verifier and the Python mini-verifier.  Every shape is at most
2^14 rows x 21 columns."""
import os
import subprocess
import sys

import numpy as np
import pytest

import logup_ref as R
import starky_bls12_381_amd as S
from logup_util import GOLDEN_DEGREE, cpu_code, golden_case, load_golden, logup_air, logup_config, logup_flips, m_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
_REF = {}


def _case(degree, m, n_rows, n_lookups=2):
    """(air, lookups, trace with some cells >= p, challenges, the reference's polynomials and closing values), computed once"""
    key = (degree, m, n_rows, n_lookups)
    if key not in _REF:
        air, blob = logup_air(degree, m, n_lookups)
        _, lookups = R.split_program(blob)
        trace, _ = R.make_trace(degree, m, n_lookups, n_rows, seed=3 * n_rows + 7 * degree + m, noncanonical=True)
        assert (trace >= np.uint64(P)).any()
        rng = np.random.default_rng(n_rows + degree + 100 * m)
        ch = [int(x) for x in rng.integers(0, P, 2, dtype=np.uint64)]
        polys, closing, zeros = R.polys_and_closing(lookups, degree, trace.tolist(), ch)
        assert zeros == 0  # the seeds: no denominator is zero under these challenges
        _REF[key] = (air, lookups, trace, ch, np.array(polys, dtype=np.uint64), np.array(closing, dtype=np.uint64))
    return _REF[key]


# csrc/kernels_permutation.h: PERM_SPAN_ROWS = 1024 rows per workgroup of the prefix sum -- 2 rows stay inside a wave (the wrap row is
# row 1), 2048 rows are two spans (one boundary); the batches: m = 1, a full batch, a full batch and a batch of one
@pytest.mark.parametrize("n_rows", [2, 2048])
@pytest.mark.parametrize("degree,m", [(d, m) for d in (2, 3, 5) for m in m_cases(d)])
def test_polys_are_the_references(prover, degree, m, n_rows):
    air, lookups, trace, ch, ref_polys, ref_closing = _case(degree, m, n_rows)
    assert (ref_closing == 0).all() and ref_polys.shape[0] == S.air_logup_polys(air)
    for layout, t in ((0, trace), (1, np.ascontiguousarray(trace.T))):
        polys, closing, zeros = prover.logup_polys(air, t, ch, layout=layout)
        assert np.array_equal(polys, ref_polys) and np.array_equal(closing, ref_closing) and zeros == 0, (layout,)


@pytest.mark.parametrize("n_rows", [1024, 1 << 14])  # exactly one span, and sixteen
def test_polys_across_spans(prover, n_rows):
    air, lookups, trace, ch, ref_polys, ref_closing = _case(3, 3, n_rows, n_lookups=1)
    polys, closing, zeros = prover.logup_polys(air, trace, ch)
    assert np.array_equal(polys, ref_polys) and np.array_equal(closing, ref_closing) and zeros == 0
    again = prover.logup_polys(air, trace, ch)
    assert np.array_equal(again[0], polys) and np.array_equal(again[1], closing)  # twice in a row, the same bytes
    reduced = trace % np.uint64(P)  # cells >= p give the words of the reduced trace
    assert np.array_equal(prover.logup_polys(air, reduced, ch)[0], polys)


def test_zero_denominators_are_counted_and_inverted_to_zero(prover):
    air, lookups, trace, ch, _, _ = _case(5, 5, 2048)
    cols, table, freq = lookups[1]
    # chi_0 = p - a looked-up cell of row 1500, chi_1 = p - the table's cell of row 3: both kinds of denominator, one challenge each
    ch = [(P - int(trace[1500, cols[3]]) % P) % P, (P - int(trace[3, table]) % P) % P]
    ref_polys, ref_closing, ref_zeros = R.polys_and_closing(lookups, 5, trace.tolist(), ch)
    assert ref_zeros >= 2
    polys, closing, zeros = prover.logup_polys(air, trace, ch)
    assert zeros == ref_zeros
    assert polys.tolist() == ref_polys and closing.tolist() == ref_closing
    assert S.logup_polys_replay(air, trace, ch)[2] == ref_zeros


def test_wrong_frequencies_show_in_the_closing_values(prover):
    air, lookups, trace, ch, _, _ = _case(3, 3, 2048)
    bad = trace.copy()
    bad[1500, lookups[0][2]] = (int(bad[1500, lookups[0][2]]) + 1) % P
    polys, closing, zeros = prover.logup_polys(air, bad, ch)
    rp, rc, rz = S.logup_polys_replay(air, bad, ch)
    assert np.array_equal(polys, rp) and np.array_equal(closing, rc) and zeros == rz == 0
    assert closing[0, 0] != 0 and closing[1, 0] != 0 and closing[0, 1] == 0 and closing[1, 1] == 0


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import logup_ref as R
import starky_bls12_381_amd as S
from logup_util import logup_air, logup_config
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
pv = S.Prover(0)
air, blob = logup_air(3, 3, 2)
ch = [0x1234567890abcdef %% R.P, 0xfedcba0987654321 %% R.P]
for n in (128, 4096):
    trace = R.make_trace(3, 3, 2, n, seed=n, noncanonical=True)[0]
    want = S.logup_polys_replay(air, trace, ch)
    for layout, t in ((0, dev(trace)), (1, dev(trace.T))):
        torch.cuda.synchronize()
        polys, closing, zeros = pv.logup_polys_device(air, t.data_ptr(), n, ch, layout=layout)
        assert np.array_equal(polys, want[0]) and np.array_equal(closing, want[1]) and (closing == 0).all() and zeros == want[2] == 0, (n, layout)
cfg = logup_config(3, 3)
trace, pis = R.make_trace(3, 3, 2, 256, 11)
ref = pv.prove(air, cfg, trace, pis)
S.verify_stark_proof(air, cfg, ref)
for layout, t in ((0, dev(trace)), (1, dev(trace.T))):
    torch.cuda.synchronize()
    assert np.array_equal(pv.prove_device(air, cfg, t.data_ptr(), 256, pis, layout=layout), ref), layout
pv.close()
print("device forms ok")
"""


def test_traces_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ whole proofs
def _prove(prover, degree, n_rows, hasher, nq, seed=11, m=None, n_lookups=2):
    m = degree if m is None else m  # a full batch and a batch of one
    air, blob = logup_air(degree, m, n_lookups)
    cfg = logup_config(degree, nq)
    trace, pis = R.make_trace(degree, m, n_lookups, n_rows, seed)
    prover.set_option("hasher", hasher)
    try:
        return air, blob, cfg, trace, pis, prover.prove(air, cfg, trace, pis)
    finally:
        prover.set_option("hasher", S.HASHER_POSEIDON)


@pytest.mark.parametrize("hasher", [S.HASHER_POSEIDON, S.HASHER_KECCAK])
@pytest.mark.parametrize("n_rows", [32, 256, 1 << 14])
@pytest.mark.parametrize("degree", [2, 3, 5])
def test_prove_and_verify(prover, degree, n_rows, hasher):
    nq = 3 if n_rows <= 256 else 84  # the Python verifier hashes every opened leaf and path: few rounds keep it within seconds
    air, blob, cfg, trace, pis, proof = _prove(prover, degree, n_rows, hasher, nq)
    assert S.proof_hasher(proof) == hasher and int(proof[13]) == 0 and int(proof[14]) == S.air_logup_polys(air) > 0
    S.verify_stark_proof(air, cfg, proof)
    if n_rows <= 256:
        R.verify_or_raise(blob, cfg, proof, hasher)
    again = _prove(prover, degree, n_rows, hasher, nq)[5]
    assert np.array_equal(proof, again)  # two runs, the same bytes
    if n_rows <= 256 or degree == 3:  # the interpreter behind the same LogUp kernel: the same bytes
        prover.set_option("quotient_impl", 1)
        try:
            other = _prove(prover, degree, n_rows, hasher, nq)[5]
        finally:
            prover.set_option("quotient_impl", 0)
        assert np.array_equal(proof, other)


def test_sixteen_looked_up_columns_at_degree_3(prover):
    """sixteen limbs in one table: eight helper batches of two, nA = 18 -- the pair mechanism holds at most two lookups at this degree"""
    air, blob, cfg, trace, pis, proof = _prove(prover, 3, 64, S.HASHER_POSEIDON, 3, m=16, n_lookups=1)
    assert S.air_logups(air) == 1 and S.air_logup_polys(air) == 18 == int(proof[14])
    S.verify_stark_proof(air, cfg, proof)
    R.verify_or_raise(blob, cfg, proof, S.HASHER_POSEIDON)
    assert prover.verify_batch([(air, cfg, proof)]) == [0]


def test_every_upload_form_gives_the_same_proof(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, 3, 256, S.HASHER_POSEIDON, 3)
    cm = np.ascontiguousarray(trace.T)
    assert np.array_equal(prover.prove(air, cfg, cm, pis, layout=1), proof)
    assert np.array_equal(prover.prove_columns(air, cfg, [cm[c].copy() for c in range(cm.shape[0])], pis), proof)
    noncanonical = R.make_trace(3, 3, 2, 256, 11, noncanonical=True)[0]
    assert (noncanonical >= np.uint64(P)).any()
    assert np.array_equal(prover.prove(air, cfg, noncanonical, pis), proof)
    prover.set_option("check_trace", 1)  # the check covers the AIR's own constraints only, and the proof is the same
    try:
        assert np.array_equal(prover.prove(air, cfg, trace, pis), proof)
    finally:
        prover.set_option("check_trace", 0)


def test_a_pools_proof_is_the_contexts(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, 3, 256, S.HASHER_POSEIDON, 3)
    pool = S.ProofPool(0, big_contexts=1, small_contexts=2, verify_proofs=True)  # the pool's own device verifier checks each before wait returns
    try:
        tickets = [pool.submit(air, cfg, trace, pis) for _ in range(3)]
        for t in tickets:
            assert np.array_equal(pool.wait(t)[0], proof)
        bad = logup_flips(proof)["aux_leaf"]
        assert pool.wait(pool.submit_verify(air, bad, config=cfg)) == S.ERR_VERIFY
        assert pool.wait(pool.submit_verify(air, proof, config=cfg)) == 0
    finally:
        pool.close()


def test_a_multi_device_handles_proof_is_the_contexts(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, 3, 256, S.HASHER_POSEIDON, 3)
    pool = S.ProofPool(big_contexts=1, small_contexts=2, devices=[0, 0])  # two pools of one handle, both on this device
    try:
        tickets = [pool.submit(air, cfg, trace, pis) for _ in range(4)]
        for t in tickets:
            assert np.array_equal(pool.wait(t)[0], proof)
    finally:
        pool.close()


def test_verify_batch_gives_the_cpu_verifiers_codes(prover):
    items = []
    for degree, n_rows, hasher in ((3, 32, 0), (3, 32, 1), (2, 256, 1), (5, 256, 0)):
        air, blob, cfg, trace, pis, proof = _prove(prover, degree, n_rows, hasher, 3)
        items.append((air, cfg, proof))
        for name, bad in logup_flips(proof).items():
            items.append((air, cfg, bad))
        t = proof.copy()
        t[14] = 0
        items.append((air, cfg, t))
    fib_cfg = S.StarkConfig.standard_fast_config()
    ft, fpis = S.trace_fibonacci(3, 5, 64)
    items.append((S.AIR_TEST_FIBONACCI, fib_cfg, prover.prove(S.AIR_TEST_FIBONACCI, fib_cfg, ft, fpis)))  # no middle matrix, beside the ones that have one
    want = [cpu_code(*it) for it in items]
    assert want.count(0) == 5 and want.count(S.ERR_VERIFY) == 20 and want.count(S.ERR_BAD_SHAPE) == 4
    assert prover.verify_batch(items) == want
    assert S.verify_batch_replay(items) == want


def test_wrong_frequencies_are_refused_and_the_context_goes_on(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, 3, 256, S.HASHER_POSEIDON, 3)
    _, lookups = R.split_program(blob)
    bad = trace.copy()
    bad[100, lookups[1][2]] = (int(bad[100, lookups[1][2]]) + 1) % P  # a frequencies cell: no constraint of the AIR itself reads it
    with pytest.raises(S.StarkhipError) as e:
        prover.prove(air, cfg, bad, pis)
    assert e.value.code == S.ERR_QUOTIENT_NOT_DIVISIBLE
    assert np.array_equal(prover.prove(air, cfg, trace, pis), proof)


def test_a_value_missing_from_the_table_is_refused_and_the_context_goes_on(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, 3, 256, S.HASHER_POSEIDON, 3)
    _, lookups = R.split_program(blob)
    bad = trace.copy()
    bad[17, lookups[0][0][1]] = 3  # the table's values are 5 k + 11: 3 is none of them
    assert 3 not in set(int(x) for x in trace[:, lookups[0][1]])
    with pytest.raises(S.StarkhipError) as e:
        prover.prove(air, cfg, bad, pis)
    assert e.value.code == S.ERR_QUOTIENT_NOT_DIVISIBLE
    assert np.array_equal(prover.prove(air, cfg, trace, pis), proof)


def test_golden_proofs_are_regenerated():
    air, blob, cfg, trace, pis = golden_case()
    assert GOLDEN_DEGREE == 3
    committed = load_golden()
    p = S.Prover(0)
    try:
        for hasher in (S.HASHER_POSEIDON, S.HASHER_KECCAK):
            p.set_option("hasher", hasher)
            assert np.array_equal(p.prove(air, cfg, trace, pis), committed[hasher]), hasher
    finally:
        p.close()
