"""A proof pool under the Keccak hasher: "hasher" = 1 is read at submit, a Keccak proof's trace commitment is its context's own launch
(the commitment scheduler's counters do not move), the pool's verifier takes each proof's hasher from its header, and switching back to 0
gives the Poseidon proof the oracle makes."""
import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from keccak_util import flips

pytestmark = pytest.mark.gpu


def test_pool_proves_and_verifies_under_keccak_then_poseidon_again():
    from bls_util import random_fp12
    fp12_ops = [(random_fp12(0x6B10 + 2 * k), random_fp12(0x6B11 + 2 * k)) for k in range(2)]
    fib_air, fp_air = S.AIR_TEST_FIBONACCI, S.AIR_FP12_MUL
    cfg = S.StarkConfig.standard_fast_config()
    # what a lone context makes
    lone = S.Prover(0)
    try:
        lone.set_option("hasher", S.HASHER_KECCAK)
        fib_traces = [S.trace_fibonacci(3 + k, 5, 64) for k in range(8)]
        want_fib = [lone.prove(fib_air, cfg, t, pis) for t, pis in fib_traces]
        want_fp = [lone.prove(fp_air, S.StarkConfig.for_air(fp_air), *S.trace_fp12_mul(x, y)) for x, y in fp12_ops]
    finally:
        lone.close()
    pool = S.ProofPool(0, big_contexts=1, small_contexts=4, verify_proofs=True)
    try:
        pool.set_option("hasher", S.HASHER_KECCAK)
        before = pool.stats()
        tickets = [pool.submit(fib_air, cfg, t, pis) for t, pis in fib_traces]
        tickets += [pool.submit_witness(fp_air, x, y) for x, y in fp12_ops]
        got = [pool.wait(t) for t in tickets]  # "verify_proofs": every wait returned OK
        after = pool.stats()
        for (proof, info), want in zip(got, want_fib + want_fp):
            assert np.array_equal(proof, want)
            assert S.proof_hasher(proof) == S.HASHER_KECCAK
            assert info["leaf_hash_form_id"] == S.LEAF_HASH_FORM_KECCAK == 6 and info["leaf_hash_form"] == "keccak"
        assert after["small_commit_requests"] == before["small_commit_requests"]
        assert after["big_commit_launches"] == before["big_commit_launches"]
        assert pool.verify_stats()["proofs_checked"] == 10
        # a verify job of a tampered Keccak proof
        bad = flips(want_fib[0])["cap"]
        assert pool.wait(pool.submit_verify(fib_air, bad, cfg)) == S.ERR_VERIFY
        assert pool.wait(pool.submit_verify(fib_air, want_fib[0], cfg)) == 0
        # back to Poseidon: the oracle's proof
        pool.set_option("hasher", S.HASHER_POSEIDON)
        t, pis = fib_traces[0]
        proof, info = pool.wait(pool.submit(fib_air, cfg, t, pis))
        assert S.proof_hasher(proof) == S.HASHER_POSEIDON and info["leaf_hash_form_id"] != 6
        w = int(proof[int(S.proof_layout(proof).off_pow_witness)])
        assert np.array_equal(proof, O.prove(S.air_program(fib_air), cfg, t.T.copy(), pis, w))
        with pytest.raises(S.StarkhipError):
            pool.set_option("hasher", 2)
    finally:
        pool.close()
