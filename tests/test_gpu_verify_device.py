"""The device verifier (starkhip_verify_batch) on the MI355X: for GPU proofs of every AIR, oracle proofs, tampered and malformed
proofs, its code per proof is exactly the CPU verifier's (starkhip_verify); a whole batch of eight signatures (48 proofs) goes in
one call, in one chunk or several, at a fraction of the CPU verifier's wall time and host CPU time."""
import time

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S

pytestmark = pytest.mark.gpu


def _cpu_code(air, cfg, proof):
    try:
        S.verify_stark_proof(air, cfg, proof)
        return 0
    except S.StarkhipError as e:
        return e.code


def _bump(proof, pos):
    bad = proof.copy()
    bad[pos] = (int(bad[pos]) + 1) % S.P
    return bad


@pytest.fixture(scope="module")
def signature_batch():
    """48 proofs of eight different signatures through the proof pool, as test_gpu_signature.py makes them: [(air, cfg, proof)]"""
    from bls_util import native_vectors
    from starky_bls12_381_amd import signature as G
    batch = 8
    sigs = G.synthetic_signatures(batch, native_vectors()["bls_signature"], seed=0x8516)
    mine = G.plan_batch(batch, 1)[0]
    pool = S.ProofPool(0, big_contexts=6, small_contexts=12, stream_priority=1, warm_up=1)
    try:
        _, results, _, _, _ = G.one_step(None, batch, pool, mine, sigs)
    finally:
        pool.close()
    out = [(air, cfg, proof) for _, (air, proof, cfg) in sorted(results.items())]
    assert len(out) == 48
    return out


@pytest.fixture(scope="module")
def small_proofs(prover):
    """GPU proofs of the toy AIR, FP12Mul and ECCAgg, and an oracle proof of the toy AIR"""
    from test_ecc_aggregate_cpu import pack, reference_vector
    from bls_util import random_fp12
    out = []
    cfg = S.StarkConfig.standard_fast_config()
    t, pis = S.trace_fibonacci(3, 5, 256)
    out.append((S.AIR_TEST_FIBONACCI, cfg, prover.prove(S.AIR_TEST_FIBONACCI, cfg, t, pis)))
    out.append((S.AIR_TEST_FIBONACCI, cfg, O.prove(S.air_program(S.AIR_TEST_FIBONACCI), cfg, S.trace_rows_to_poly_values(t), pis)))
    air = S.AIR_FP12_MUL
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED3000), random_fp12(0x5EED3001))
    cfg = S.StarkConfig.for_air(air)
    proof = prover.prove(air, cfg, t, pis)
    out.append((air, cfg, proof))
    out.append((air, cfg, O.prove(S.air_program(air), cfg, S.trace_rows_to_poly_values(t), pis)))
    air = S.AIR_ECC_AGGREGATE
    pts, bits, _ = reference_vector()
    arr, b = pack(pts, bits)
    t, pis = S.trace_ecc_aggregate(arr, b)
    cfg = S.StarkConfig.for_air(air)
    out.append((air, cfg, prover.prove(air, cfg, t, pis)))
    return out


def test_device_verifier_accepts_gpu_and_oracle_proofs_of_every_air(prover, small_proofs, signature_batch):
    one_each = {}
    for air, cfg, proof in signature_batch:
        one_each.setdefault(air, (air, cfg, proof))
    items = small_proofs + list(one_each.values())
    assert {a for a, _, _ in items} == {S.AIR_TEST_FIBONACCI, S.AIR_FP12_MUL, S.AIR_ECC_AGGREGATE, S.AIR_FINAL_EXP, S.AIR_MILLER_LOOP,
                                        S.AIR_PAIRING_PRECOMP}
    assert [_cpu_code(*it) for it in items] == [0] * len(items)
    assert prover.verify_batch(items) == [0] * len(items)
    for it in items[:3]:
        prover.verify_stark_proof_device(*it)


def _sweep(air, cfg, proof):
    """tamper positions: header, both caps, openings, trace-leaf words of a first, middle and last query, a Merkle sibling, a
    quotient-leaf word, a FRI evaluation and a FRI sibling of every layer, the final polynomial, the PoW nonce, a public input"""
    L = S.proof_layout(proof)
    g = lambda f: int(getattr(L, f))  # noqa: E731
    q0, qw, nq = g("off_query_rounds"), g("query_round_words"), g("n_query_rounds")
    pos = [3, g("off_trace_cap") + 2, g("off_quotient_cap") + 5, g("off_local_values") + 11, g("off_next_values") + 7,
           g("off_quotient_openings") + 1]
    for r in (0, nq // 2, nq - 1):
        base = q0 + r * qw
        pos += [base + g("q_trace_leaf"), base + g("q_trace_leaf") + g("n_columns") - 1]
    base = q0 + 5 * qw
    pos += [base + g("q_trace_siblings") + 3, base + g("q_quotient_leaf"), base + g("q_quotient_siblings")]
    for l in range(g("n_fri_layers")):
        pos += [base + int(L.q_step_evals[l]) + 1, base + int(L.q_step_siblings[l]) + 2]
    pos += [g("off_fri_caps") + 1] if g("n_fri_layers") else []
    pos += [g("off_final_poly"), g("off_pow_witness"), g("off_public_inputs")]
    items = [(air, cfg, _bump(proof, p)) for p in pos]
    items[0] = (air, cfg, _bump(proof, 0))  # the magic
    items.append((air, cfg, proof[:-1]))
    bad = proof.copy()
    bad[q0 + qw + 4] = S.P  # a word >= p in a query round
    items.append((air, cfg, bad))
    return items


def test_tamper_sweep_gives_the_cpu_verifiers_codes(prover, small_proofs, signature_batch):
    fp12 = next(it for it in small_proofs if it[0] == S.AIR_FP12_MUL)
    fexp = next(it for it in signature_batch if it[0] == S.AIR_FINAL_EXP)
    for air, cfg, proof in (fp12, fexp):
        items = _sweep(air, cfg, proof) + [(air, cfg, proof)]
        want = [_cpu_code(*it) for it in items]
        assert want[-1] == 0 and all(w != 0 for w in want[:-1])
        assert prover.verify_batch(items) == want


def _batch_with_tampered(signature_batch):
    items = list(signature_batch)
    for k, i in enumerate((1, 9, 17, 25, 33, 41)):
        air, cfg, proof = signature_batch[i]
        L = S.proof_layout(proof)
        pos = int(L.off_query_rounds) + (k * 13 + 1) * int(L.query_round_words) + k  # a trace-leaf word of a different query each time
        items.insert(i + k + 1, (air, cfg, _bump(proof, pos)))
    return items


def test_signature_batch_with_tampered_copies_in_one_or_several_chunks(prover, signature_batch):
    items = _batch_with_tampered(signature_batch)
    want = [_cpu_code(*it) for it in items]
    assert want.count(0) == 48 and want.count(S.ERR_VERIFY) == 6
    assert prover.verify_batch(items) == want
    small = S.Prover(0)
    try:
        small.set_option("verify_chunk_mb", 200)  # several proofs' worth of query rounds per chunk at most
        assert small.verify_batch(items) == want
    finally:
        small.close()


def test_null_context_and_malformed_proof():
    import ctypes as C
    from starky_bls12_381_amd.api import lib, StarkConfig
    airs = (C.c_int * 1)(S.AIR_TEST_FIBONACCI)
    cfgs = (StarkConfig * 1)(S.StarkConfig.standard_fast_config())
    res = (C.c_int * 1)()
    words = (C.c_size_t * 1)(0)
    ptrs = (C.POINTER(C.c_uint64) * 1)()
    assert lib.starkhip_verify_batch(None, 1, airs, cfgs, ptrs, words, res) == S.ERR_NO_DEVICE
    p = S.Prover(0)
    try:
        assert p.verify_batch([(S.AIR_TEST_FIBONACCI, S.StarkConfig.standard_fast_config(), np.zeros(40, dtype=np.uint64))]) == [S.ERR_BAD_SHAPE]
        with pytest.raises(S.StarkhipError):
            p.verify_stark_proof_device(S.AIR_TEST_FIBONACCI, S.StarkConfig.standard_fast_config(), np.zeros(40, dtype=np.uint64))
    finally:
        p.close()


def test_device_verifier_takes_a_quarter_of_the_cpu_verifiers_time(prover, signature_batch):
    prover.verify_batch(signature_batch[:2])  # first-call costs (code objects, tables) out of the measurement
    c0, t0 = time.process_time(), time.perf_counter()
    for it in signature_batch:
        S.verify_stark_proof(*it)
    cpu_wall, cpu_cpu = time.perf_counter() - t0, time.process_time() - c0
    t0 = time.perf_counter()
    assert prover.verify_batch(signature_batch) == [0] * 48
    dev_wall = time.perf_counter() - t0
    tm = prover.last_verify_timings()
    print("cpu verifier %.3f s wall %.2f CPU-s; device %.3f s wall %.2f CPU-s %s" % (cpu_wall, cpu_cpu, dev_wall, tm["cpu_s"], tm))
    assert dev_wall <= cpu_wall / 4
    assert tm["cpu_s"] <= cpu_cpu / 4
