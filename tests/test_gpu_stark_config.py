"""StarkConfigs other than standard_fast on the GPU: proofs byte-identical to the CPU oracle's at a grid of configs (every FRI
arity, cap height, rate, query count and proof-of-work setting of tests/config_cases.py) through every proving path, a mixed
device-verify batch with tampered copies, one verifying pool proving one AIR at several configs, and refused configs."""
import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from config_cases import CASES, bump, case_air, case_config, case_id, make_config, small_cell_air, sweep_positions

pytestmark = pytest.mark.gpu


def _pow(proof):
    return int(proof[int(S.proof_layout(proof).off_pow_witness)])


def _code(air, cfg, proof):
    try:
        S.verify_stark_proof(air, cfg, proof)
        return 0
    except S.StarkhipError as e:
        return e.code


def _first_difference(proof, ref):
    """the section of the first word where two proofs differ (a readable failure)"""
    if proof.size != ref.size:
        return f"sizes {proof.size} != {ref.size}"
    i = int(np.flatnonzero(proof != ref)[0])
    L = S.proof_layout(ref)
    names = ["off_trace_cap", "off_quotient_cap", "off_local_values", "off_next_values", "off_quotient_openings", "off_fri_caps",
             "off_query_rounds", "off_final_poly", "off_pow_witness", "off_public_inputs"]
    sec = [n for n in names if int(getattr(L, n)) <= i][-1] if i >= 16 else "header"
    if sec == "off_query_rounds":
        q, w = divmod(i - int(L.off_query_rounds), int(L.query_round_words))
        return f"word {i}: query round {q}, word {w} of the round"
    return f"word {i}: {sec}"


_GPU = {}


def _gpu_proof(prover, case):
    if case not in _GPU:
        air, _, t, pis, _ = case_air(case)
        _GPU[case] = prover.prove(air, case_config(case), t, pis)
    return _GPU[case]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_gpu_proof_at_config_is_the_oracles(prover, case):
    air, blob, t, pis, _ = case_air(case)
    cfg = case_config(case)
    proof = _gpu_proof(prover, case)
    ref = O.prove(blob, cfg, t.T.copy(), pis, _pow(proof))
    assert proof.size == ref.size and np.array_equal(proof, ref), _first_difference(proof, ref)
    S.verify_stark_proof(air, cfg, proof)
    w = _pow(proof)
    assert np.array_equal(prover.prove(air, cfg, t.T.copy(), pis, pow_witness=w, layout=1), proof)
    assert np.array_equal(prover.prove_columns(air, cfg, [c.copy() for c in t.T], pis, pow_witness=w), proof)


# wide traces recorded as write logs, at R = 8 and 32 (the trace parked inside the LDE buffer) and at rate 0 (a buffer of its own)
LOG_CASES = [(300, 5, 3, make_config(3, 0, 1, 0, 2, 0)), (300, 4, 7, make_config(5, 4, 3, 2, 28, 1)),
             (130, 2, 8, make_config(3, 2, 5, 0, 2, 8)), (5, 2, 8, make_config(0, 0, 2, 0, 2, 0))]


@pytest.mark.parametrize("cols,degree,log_n,cfg", LOG_CASES, ids=[f"c{c}d{d}-n{n}-r{g.rate_bits}" for c, d, n, g in LOG_CASES])
def test_gpu_proof_of_a_trace_log_at_config_is_the_oracles(prover, cols, degree, log_n, cfg):
    blob, t, pis = small_cell_air(cols, degree, log_n, seed=cols + log_n)
    air = S.register_air(blob, name=f"cells{cols}d{degree}")
    r_idx, c_idx = np.nonzero(t)
    order = np.lexsort((r_idx, c_idx))
    log = S.trace_from_writes(t.shape[0], cols, [(int(r), int(c), 1) for r, c in zip(r_idx[order], c_idx[order])])
    proof = prover.prove(air, cfg, log, pis)
    ref = O.prove(blob, cfg, t.T.copy(), pis, _pow(proof))
    assert proof.size == ref.size and np.array_equal(proof, ref), _first_difference(proof, ref)
    assert np.array_equal(prover.prove(air, cfg, t, pis, pow_witness=_pow(proof)), proof)
    S.verify_stark_proof(air, cfg, proof)


def test_mixed_config_verify_batch_gives_the_cpu_verifiers_codes(prover):
    """One batch: the Fibonacci AIR's GPU proofs at all of its grid configs, other AIRs' between them, and tampered copies of a
    proof at arity 1 and one at arity 5 -- every code equals the CPU verifier's."""
    fib = [c for c in CASES if c[0] == "fib"]
    others = [c for c in CASES if c[0] != "fib"][:6]
    items = [(case_air(c)[0], case_config(c), _gpu_proof(prover, c)) for c in fib + others]
    for c in (next(c for c in fib if c[4] == 1), CASES[26]):  # arity 1 and arity 5, each with query rounds
        air, cfg, proof = case_air(c)[0], case_config(c), _gpu_proof(prover, c)
        items += [(air, cfg, bump(proof, p)) for p in sweep_positions(proof)]
    want = [_code(*it) for it in items]
    n_good = len(fib) + len(others)
    assert want[:n_good] == [0] * n_good and all(w != 0 for w in want[n_good:])
    assert prover.verify_batch(items) == want


def test_one_air_at_three_configs_in_a_verifying_pool():
    """The same AIR and trace at rate 1, rate 3 and arity 2 in one burst: the small-commitment merge groups by (columns, rows,
    rate), so two of them may share a launch and the third may not; every result must still be the oracle's bytes, verified."""
    t, pis = S.trace_fibonacci(3, 5, 256)
    air, blob = S.AIR_TEST_FIBONACCI, S.air_program(S.AIR_TEST_FIBONACCI)
    cfgs = [make_config(1, 4, 4, 5, 28, 8), make_config(3, 3, 3, 0, 28, 8), make_config(1, 0, 2, 2, 28, 8)] * 2
    pool = S.ProofPool(0, big_contexts=1, small_contexts=3, verify_proofs=True)
    try:
        tickets = [pool.submit(air, cfg, t, pis) for cfg in cfgs]
        proofs = [pool.wait(tk)[0] for tk in tickets]
        stats = pool.verify_stats()
    finally:
        pool.close()
    for cfg, proof in zip(cfgs, proofs):
        assert np.array_equal(proof, O.prove(blob, cfg, t.T.copy(), pis, _pow(proof)))
    assert stats["proofs_checked"] >= len(cfgs) and stats["rejected"] == 0


def test_refused_configs_are_bad_shape_on_the_gpu_paths(prover):
    t, pis = S.trace_fibonacci(3, 5, 128)
    air = S.AIR_TEST_FIBONACCI
    good = make_config(2, 3, 2, 0, 28, 8)
    proof = prover.prove(air, good, t, pis)
    refused = [make_config(2, 0, 2, 0, 28, 8),   # 7 -> 5 -> 3 -> 1, then a layer of arity 2: plonky2's assert
               make_config(2, 3, 0, 0, 28, 8), make_config(2, 3, 9, 0, 28, 8), make_config(2, 10, 2, 0, 28, 8),
               make_config(0, 0, 2, 0, 28, 0),   # rate 0 below the Fibonacci AIR's quotient degree
               make_config(9, 3, 2, 0, 28, 8), make_config(2, 17, 2, 0, 28, 8), make_config(2, 3, 2, 0, 28, 65),
               make_config(2, 3, 2, 0, 28, 8, challenges=3)]
    for cfg in refused:
        with pytest.raises(S.StarkhipError) as e:
            prover.prove(air, cfg, t, pis)
        assert e.value.code == S.ERR_BAD_SHAPE
    assert prover.verify_batch([(air, cfg, proof) for cfg in refused] + [(air, good, proof)]) == [S.ERR_BAD_SHAPE] * len(refused) + [0]
    for devices in (None, [0]):
        pool = S.ProofPool(0, big_contexts=1, small_contexts=1, **({"devices": devices} if devices else {"verify_proofs": True}))
        try:
            for cfg in refused:
                with pytest.raises(S.StarkhipError) as e:
                    pool.wait(pool.submit(air, cfg, t, pis))
                assert e.value.code == S.ERR_BAD_SHAPE
            if devices is None:
                assert [pool.wait(pool.submit_verify(air, proof, config=cfg)) for cfg in refused[:3]] == [S.ERR_BAD_SHAPE] * 3
            assert np.array_equal(pool.wait(pool.submit(air, good, t, pis))[0], proof)
        finally:
            pool.close()
    # the context still proves after every refusal
    assert np.array_equal(prover.prove(air, good, t, pis), proof)
    S.verify_stark_proof(air, good, proof)
