"""User-defined AIRs on the GPU: registered programs proven byte-identically to the CPU oracle through every proving path, and the
device trace checker (starkhip_check_trace) against oracle_check_trace on custom and real traces."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from bls_util import fp_arr, random_fp12
from random_air import CASES, random_air
from test_gpu_airs import _bls

pytestmark = pytest.mark.gpu


def _pow(proof):
    return int(proof[int(S.proof_layout(proof).off_pow_witness)])


def _miller_loop_trace():
    b = _bls()
    return S.trace_miller_loop(fp_arr(b["gx"]), fp_arr(b["gy"]), fp_arr(b["s_x1"], b["s_x2"]), fp_arr(b["s_y1"], b["s_y2"]),
                               fp_arr(b["s_z1"], b["s_z2"]))


def test_fp12_mul_under_a_registered_id_proves_the_same_bytes(prover):
    air = S.register_air(S.air_program(S.AIR_FP12_MUL), name="FP12MulCopy", default_rows=16)
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED7000), random_fp12(0x5EED7001))
    cfg = S.StarkConfig.for_air(air)
    proof = prover.prove(air, cfg, t, pis)
    assert np.array_equal(proof, prover.prove(S.AIR_FP12_MUL, S.StarkConfig.for_air(S.AIR_FP12_MUL), t, pis))
    assert np.array_equal(proof, O.prove(S.air_program(air), cfg, S.trace_rows_to_poly_values(t), pis, _pow(proof)))
    S.verify_stark_proof(air, cfg, proof)


@pytest.mark.parametrize("seed,cols,degree,rows", CASES)
def test_random_air_gpu_proof_is_the_oracles(prover, seed, cols, degree, rows):
    blob, trace, pis = random_air(seed, cols, degree, rows)
    air = S.register_air(blob, name=f"random{seed}", default_rows=rows)
    cfg = S.StarkConfig.for_air(air)
    proof = prover.prove(air, cfg, trace, pis)
    ref = O.prove(blob, cfg, trace.T.copy(), pis, _pow(proof))
    assert proof.size == ref.size and np.array_equal(proof, ref)
    S.verify_stark_proof(air, cfg, proof)
    tampered = proof.copy()
    tampered[int(S.proof_layout(proof).off_final_poly)] ^= np.uint64(1)
    assert prover.verify_batch([(air, cfg, proof), (air, cfg, tampered)]) == [0, S.ERR_VERIFY]
    # column-major and the literal Vec<PolynomialValues> argument give the same bytes
    assert np.array_equal(prover.prove(air, cfg, trace.T.copy(), pis, layout=1), proof)
    assert np.array_equal(prover.prove_columns(air, cfg, [c.copy() for c in trace.T], pis), proof)
    assert prover.check_trace(air, trace, pis) == (0, (0, 0, 0))
    assert prover.check_trace(air, trace.T.copy(), pis, layout=1) == (0, (0, 0, 0))


def test_random_airs_in_a_verifying_pool_and_a_one_device_multipool():
    cases = [random_air(*c) for c in CASES[:6]]
    airs = [S.register_air(b) for b, _, _ in cases]
    cfgs = [S.StarkConfig.for_air(a) for a in airs]
    refs = [O.prove(b, cfg, t.T.copy(), p) for (b, t, p), cfg in zip(cases, cfgs)]
    pool = S.ProofPool(0, big_contexts=1, small_contexts=3, verify_proofs=True)
    try:
        tickets = [pool.submit(a, cfg, t, p) for a, cfg, (_, t, p) in zip(airs, cfgs, cases)]
        for tk, ref in zip(tickets, refs):
            assert np.array_equal(pool.wait(tk)[0], ref)
        # a registered AIR has no trace generator
        ops = (C.c_uint32 * 4)()
        tk = C.c_uint64()
        assert S.lib.starkhip_pool_submit_witness(pool._h, airs[0], None, ops, 4, S.POW_SEARCH, C.byref(tk)) == S.ERR_BAD_AIR
        vt = [pool.submit_verify(a, ref, config=cfg) for a, cfg, ref in zip(airs, cfgs, refs)]
        assert [pool.wait(t) for t in vt] == [0] * len(vt)
    finally:
        pool.close()
    mp = S.ProofPool(0, big_contexts=1, small_contexts=2, devices=[0])
    try:
        tickets = [mp.submit(a, cfg, t, p) for a, cfg, (_, t, p) in zip(airs, cfgs, cases)]
        for tk, ref in zip(tickets, refs):
            assert np.array_equal(mp.wait(tk)[0], ref)
    finally:
        mp.close()


def test_check_trace_counts_violations_as_the_oracle(prover):
    for seed, cols, degree, rows in CASES[2:]:
        blob, trace, pis = random_air(seed, cols, degree, rows)
        air = S.register_air(blob)
        rng = np.random.default_rng(seed)
        for _ in range(4):
            bad = trace.copy()
            r, c = int(rng.integers(0, rows)), int(rng.integers(0, cols))
            bad[r, c] = np.uint64((int(bad[r, c]) + 1 + int(rng.integers(0, 1000))) % S.P)
            got, want = prover.check_trace(air, bad, pis), O.check_trace(blob, bad, pis)
            assert got[0] == want[0]
            if want[0]:
                assert got[1][0] == want[1][0]
                assert got[1][2] == O.eval_frame(blob, bad[got[1][1]], bad[(got[1][1] + 1) % rows], pis, [1, 1, 1, 1])[got[1][0]]
                rows_of_k = [row for row in range(rows)
                             if O.eval_frame(blob, bad[row], bad[(row + 1) % rows], pis, [1, 1, 1, 1])[got[1][0]] != 0]
                assert got[1][1] in rows_of_k
                if len(rows_of_k) == 1:  # the oracle's row is deterministic only then
                    assert got[1] == want[1]
        if len(pis):
            wrong = pis.copy()
            wrong[0] = np.uint64((int(wrong[0]) + 1) % S.P)
            got, want = prover.check_trace(air, trace, wrong), O.check_trace(blob, trace, wrong)
            assert got[0] == want[0] and got[0] > 0 and got[1][0] == want[1][0]


def test_check_trace_on_real_traces(prover):
    t, pis = _miller_loop_trace()
    air = S.AIR_MILLER_LOOP
    blob = S.air_program(air)
    assert prover.check_trace(air, t, pis) == (0, (0, 0, 0))
    custom = S.register_air(blob)
    assert prover.check_trace(custom, t, pis) == (0, (0, 0, 0))
    broken = 0
    for col in (1234, 5000, 20011, 48000, 77777, 97000, 3, 64):  # one corrupted cell; not every cell is constrained on every row
        bad = t.copy()
        bad[517, col] = np.uint64((int(bad[517, col]) + 3) % S.P)
        got, want = prover.check_trace(air, bad, pis), O.check_trace(blob, bad, pis)
        assert got[0] == want[0] and got[1][0] == want[1][0]
        broken += want[0] > 0
    assert broken > 0
    wrong = pis.copy()
    wrong[7] = np.uint64((int(wrong[7]) + 1) % S.P)
    got, want = prover.check_trace(air, t, wrong), O.check_trace(blob, t, wrong)
    assert got[0] == want[0] > 0 and got[1][0] == want[1][0]
    del t, bad
    b = _bls()
    t, pis = S.trace_pairing_precomp(fp_arr(b["hm_x1"], b["hm_x2"]), fp_arr(b["hm_y1"], b["hm_y2"]), fp_arr(b["hm_z1"], b["hm_z2"]))
    assert prover.check_trace(S.AIR_PAIRING_PRECOMP, t, pis) == (0, (0, 0, 0))
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED7100), random_fp12(0x5EED7101))
    assert prover.check_trace(S.AIR_FP12_MUL, t, pis) == (0, (0, 0, 0))


def test_check_trace_on_a_final_exp_trace(prover):
    from bls_util import native_vectors
    aa = fp_arr(*[int(s) for s in native_vectors()["final_exp_input_aa"]])
    t, pis = S.trace_final_exp(aa)
    assert prover.check_trace(S.AIR_FINAL_EXP, t, pis) == (0, (0, 0, 0))
    t[4000] = np.where(t[4000] == np.uint64(S.P - 1), np.uint64(0), t[4000] + np.uint64(1))
    got = prover.check_trace(S.AIR_FINAL_EXP, t, pis)
    assert got[0] > 0
    k, row, value = got[1]
    assert row in (3999, 4000) and value != 0


def test_unsatisfiable_trace_fails_to_prove_and_the_checker_names_the_constraint(prover):
    # degree 4: the quotient is computed on 4n points for 3n coefficients, so the spare ones are checked (starky's trim_to_len)
    blob, trace, pis = random_air(41, 30, 4, 64)
    air = S.register_air(blob)
    cfg = S.StarkConfig.for_air(air)
    bad = pis.copy()
    bad[-1] = np.uint64((int(bad[-1]) + 5) % S.P)  # pins a last-row constraint: one violation, on row 63
    with pytest.raises(S.StarkhipError) as e:
        prover.prove(air, cfg, trace, bad)
    assert e.value.code == S.ERR_QUOTIENT_NOT_DIVISIBLE
    n, (k, row, value) = prover.check_trace(air, trace, bad)
    want = O.check_trace(blob, trace, bad)
    assert n == want[0] == 1 and (k, row, value) == want[1] and row == 63
