"""Permutation arguments of registered AIRs on the GPU (COMPAT.md P1 - P8): the Z kernels of csrc/kernels_permutation.hip against the
Python reference of tests/permutation_ref.py, byte for byte, and whole proofs of AIRs with permutation pairs -- degree 2, 3 and 5
(B = 1, 2, 4), both hashers, both quotient evaluators, a pool -- through the product's CPU verifier, its device verifier and the
Python mini-verifier.  Every shape is at most 2^14 rows x 8 columns."""
import os
import subprocess
import sys

import numpy as np
import pytest

import permutation_ref as R
import starky_bls12_381_amd as S
from permutation_util import GOLDEN_DEGREE, cpu_code, golden_case, load_golden, perm_air, perm_config, perm_flips

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
# csrc/kernels_permutation.h: PERM_SPAN_ROWS = 1024 rows per workgroup of the prefix product -- 4096 rows cross four workgroups, 2^14
# sixteen; 2048 two (one boundary), 64 and 128 stay inside one (one and two waves), 2 inside a wave
ZS_ROWS = [2, 64, 128, 2048, 4096, 1 << 14]
_REF = {}


def _zs_case(degree, n_rows):
    """(air, trace with some cells >= p, challenges, the reference's zs and closing products), computed once"""
    key = (degree, n_rows)
    if key not in _REF:
        air, blob = perm_air(degree, 8)
        _, pairs = R.split_program(blob)
        trace, _ = R.make_trace(degree, n_rows, seed=3 * n_rows + degree, n_cols=8, noncanonical=True)
        assert (trace >= np.uint64(P)).any()
        rng = np.random.default_rng(n_rows + degree)
        ch = [int(x) for x in rng.integers(0, P, 4 * max(1, degree - 1), dtype=np.uint64)]
        zs, closing = R.zs_and_closing(pairs, degree, trace.tolist(), ch)
        _REF[key] = (air, trace, ch, np.array(zs, dtype=np.uint64), np.array(closing, dtype=np.uint64))
    return _REF[key]


@pytest.mark.parametrize("n_rows", ZS_ROWS)
def test_zs_are_the_references(prover, n_rows):
    air, trace, ch, ref_zs, ref_closing = _zs_case(3, n_rows)
    assert (ref_closing == 1).all()
    for layout, t in ((0, trace), (1, np.ascontiguousarray(trace.T))):
        zs, closing = prover.permutation_zs(air, t, ch, layout=layout)
        assert np.array_equal(zs, ref_zs) and np.array_equal(closing, ref_closing), (n_rows, layout)


@pytest.mark.parametrize("degree,n_rows", [(2, 128), (5, 2048), (5, 2)])
def test_zs_of_other_batch_sizes(prover, degree, n_rows):
    air, trace, ch, ref_zs, ref_closing = _zs_case(degree, n_rows)
    zs, closing = prover.permutation_zs(air, trace, ch)
    assert np.array_equal(zs, ref_zs) and np.array_equal(closing, ref_closing)


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import permutation_ref as R
import starky_bls12_381_amd as S
from permutation_util import perm_air, perm_config
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
pv = S.Prover(0)
air, blob = perm_air(3, 8)
rng = np.random.default_rng(9)
ch = [int(x) for x in rng.integers(0, R.P, 8, dtype=np.uint64)]
for n in (128, 4096):
    trace = R.make_trace(3, n, seed=n, n_cols=8, noncanonical=True)[0]
    want = S.permutation_zs_replay(air, trace, ch)
    for layout, t in ((0, dev(trace)), (1, dev(trace.T))):
        torch.cuda.synchronize()
        zs, closing = pv.permutation_zs_device(air, t.data_ptr(), n, ch, layout=layout)
        assert np.array_equal(zs, want[0]) and np.array_equal(closing, want[1]) and (closing == 1).all(), (n, layout)
cfg = perm_config(3, 3)
trace, pis = R.make_trace(3, 256, 11, n_cols=8)
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


def test_a_changed_cell_shows_in_the_closing_products(prover):
    air, trace, ch, _, _ = _zs_case(3, 2048)
    bad = trace.copy()
    bad[1500, 4] = (int(bad[1500, 4]) + 1) % P
    zs, closing = prover.permutation_zs(air, bad, ch)
    rz, rc = S.permutation_zs_replay(air, bad, ch)
    assert np.array_equal(zs, rz) and np.array_equal(closing, rc)
    assert closing[0] != 1 and closing[1] != 1


# ------------------------------------------------------------------------------------------------ whole proofs
def _prove(prover, degree, n_rows, hasher, nq, seed=11):
    air, blob = perm_air(degree)
    cfg = perm_config(degree, nq)
    trace, pis = R.make_trace(degree, n_rows, seed)
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
    assert S.proof_hasher(proof) == hasher and int(proof[13]) == S.air_permutation_zs(air)
    S.verify_stark_proof(air, cfg, proof)
    if n_rows <= 256:
        R.verify_or_raise(blob, cfg, proof, hasher)
    again = _prove(prover, degree, n_rows, hasher, nq)[5]
    assert np.array_equal(proof, again)  # two runs, the same bytes
    if n_rows <= 256 or degree == 3:  # the interpreter behind the same permutation kernel: the same bytes
        prover.set_option("quotient_impl", 1)
        try:
            other = _prove(prover, degree, n_rows, hasher, nq)[5]
        finally:
            prover.set_option("quotient_impl", 0)
        assert np.array_equal(proof, other)


def test_every_upload_form_gives_the_same_proof(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, 3, 256, S.HASHER_POSEIDON, 3)
    cm = np.ascontiguousarray(trace.T)
    assert np.array_equal(prover.prove(air, cfg, cm, pis, layout=1), proof)
    assert np.array_equal(prover.prove_columns(air, cfg, [cm[c].copy() for c in range(cm.shape[0])], pis), proof)
    noncanonical = R.make_trace(3, 256, 11, noncanonical=True)[0]
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
        bad = perm_flips(proof)["zs_leaf"]
        assert pool.wait(pool.submit_verify(air, bad, config=cfg)) == S.ERR_VERIFY
        assert pool.wait(pool.submit_verify(air, proof, config=cfg)) == 0
    finally:
        pool.close()


def test_verify_batch_gives_the_cpu_verifiers_codes(prover):
    items = []
    for degree, n_rows, hasher in ((3, 32, 0), (3, 32, 1), (2, 256, 1), (5, 256, 0)):
        air, blob, cfg, trace, pis, proof = _prove(prover, degree, n_rows, hasher, 3)
        items.append((air, cfg, proof))
        for name, bad in perm_flips(proof).items():
            items.append((air, cfg, bad))
        t = proof.copy()
        t[13] = 0
        items.append((air, cfg, t))
    fib_cfg = S.StarkConfig.standard_fast_config()
    ft, fpis = S.trace_fibonacci(3, 5, 64)
    for hasher in (S.HASHER_POSEIDON, S.HASHER_KECCAK):  # the two built-in toy proofs: no Zs, beside the ones that have them
        prover.set_option("hasher", hasher)
        try:
            items.append((S.AIR_TEST_FIBONACCI, fib_cfg, prover.prove(S.AIR_TEST_FIBONACCI, fib_cfg, ft, fpis)))
        finally:
            prover.set_option("hasher", S.HASHER_POSEIDON)
    want = [cpu_code(*it) for it in items]
    assert want.count(0) == 6 and S.ERR_VERIFY in want and S.ERR_BAD_SHAPE in want
    assert prover.verify_batch(items) == want
    assert S.verify_batch_replay(items) == want


def test_a_trace_whose_rhs_is_no_permutation_is_refused_and_the_context_goes_on(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, 3, 256, S.HASHER_POSEIDON, 3)
    bad = trace.copy()
    bad[100, 4] = (int(bad[100, 4]) + 1) % P  # an rhs cell no constraint of the AIR itself reads
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
