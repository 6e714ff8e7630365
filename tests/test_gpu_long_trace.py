"""Registered AIRs on traces of more than 8192 rows: the multi-workgroup transform (csrc/kernels_lde_long.hip) against the oracle's LDE
bit for bit, whole proofs byte for byte against the oracle's, the trace checker, a pool, the batch verifier, and the rule itself
(registered AIRs up to 2^MAX_LOG_ROWS rows, built-in ones 8192)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from random_air import random_air

pytestmark = pytest.mark.gpu

P = S.P


def _cols(seed, n_cols, n):
    return np.random.default_rng(seed).integers(0, P, size=(n_cols, n), dtype=np.uint64)


def _check_lde(prover, vals, rate_bits):
    coeffs, lde = prover.lde_batch(vals, rate_bits)
    ocoeffs, olde_rows = O.lde_rows(vals, rate_bits)
    assert np.array_equal(coeffs, ocoeffs)
    assert np.array_equal(lde, olde_rows.T)


@pytest.mark.parametrize("log_n", range(14, 21))
def test_lde_of_every_long_size_is_the_oracles(prover, log_n):
    _check_lde(prover, _cols(100 + log_n, 3, 1 << log_n), 1)


@pytest.mark.parametrize("log_n", [14, 15])  # an even and an odd split of the index
@pytest.mark.parametrize("rate_bits", [0, 2, 3])
@pytest.mark.parametrize("n_cols", [1, 2, 65])
def test_lde_rates_and_column_counts(prover, log_n, rate_bits, n_cols):
    _check_lde(prover, _cols(1000 * log_n + 10 * rate_bits + n_cols, n_cols, 1 << log_n), rate_bits)


@pytest.mark.parametrize("log_n", [14, 15])
def test_lde_of_special_columns(prover, log_n):
    n = 1 << log_n
    b = log_n - log_n // 2  # n = 2^a 2^b, the contiguous factor
    vals = np.zeros((7, n), dtype=np.uint64)
    vals[1] = 0x123456789ABCDEF % P
    vals[2, 0] = 1
    vals[3, n - 1] = 1
    vals[4, 1 << b] = 1
    vals[5] = P - 1
    vals[6] = _cols(7, 1, n)[0]
    _check_lde(prover, vals, 1)


@pytest.mark.parametrize("log_len", [21, 22, 23])  # splits 10 + 11, 11 + 11, 11 + 12: tiles of 16 and 8, 8 and 8, 8 and 4 words
def test_vectors_longer_than_a_column(prover, log_len):
    """what a 2^20-row proof transforms beside its columns (the quotient's n 2^qdb values, the FRI polynomial's N), both directions"""
    values = _cols(200 + log_len, 1, 1 << log_len)
    coeffs, same = O.lde_rows(values, 0)  # coefficients, and (rate_bits 0) their values on the coset 7 <w_n>
    assert np.array_equal(prover.ntt_long(values, inverse=True), coeffs)
    assert np.array_equal(prover.ntt_long(coeffs), values)
    with pytest.raises(S.StarkhipError) as e:
        prover.ntt_long(values[:, :1 << 15])
    assert e.value.code == S.ERR_BAD_SHAPE


# seed, columns, degree, rows, rate_bits
PROOF_CASES = [(21, 5, 3, 1 << 14, 1), (24, 9, 5, 1 << 15, 2), (22, 12, 3, 1 << 16, 1), (25, 70, 4, 1 << 14, 2)]


def _config(air, rate_bits):
    cfg = S.StarkConfig.for_air(air)
    assert cfg.rate_bits <= rate_bits
    cfg.rate_bits = rate_bits
    return cfg


def _pow(proof):
    return int(proof[int(S.proof_layout(proof).off_pow_witness)])


@functools.lru_cache(maxsize=None)
def _case(i):
    """(air, cfg, row-major trace, public inputs, blob) of PROOF_CASES[i], built once"""
    seed, cols, degree, rows, rate_bits = PROOF_CASES[i]
    blob, trace, pis = random_air(seed, cols, degree, rows)
    air = S.register_air(blob, name=f"long{seed}", default_rows=rows)
    return air, _config(air, rate_bits), trace, pis, blob


_proofs = {}


def _proof(prover, i):
    """the GPU proof of case i, checked against the oracle's once"""
    if i not in _proofs:
        air, cfg, trace, pis, blob = _case(i)
        proof = prover.prove(air, cfg, trace, pis)
        ref = O.prove(blob, cfg, trace.T.copy(), pis, _pow(proof))
        assert proof.size == ref.size and np.array_equal(proof, ref)
        _proofs[i] = proof
    return _proofs[i]


@pytest.mark.parametrize("i", range(len(PROOF_CASES)))
def test_long_proof_is_the_oracles_and_verifies(prover, i):
    air, cfg, trace, pis, _ = _case(i)
    proof = _proof(prover, i)
    S.verify_stark_proof(air, cfg, proof)
    # column-major and the literal Vec<PolynomialValues> argument give the same bytes
    assert np.array_equal(prover.prove(air, cfg, trace.T.copy(), pis, layout=1), proof)
    assert np.array_equal(prover.prove_columns(air, cfg, [c.copy() for c in trace.T], pis), proof)


def test_check_trace_on_32768_rows(prover):
    air, cfg, trace, pis, blob = _case(1)
    n = trace.shape[0]
    assert prover.check_trace(air, trace, pis) == (0, (0, 0, 0))
    rng = np.random.default_rng(5)
    r = int(rng.integers(8193, n))
    # a random AIR has free columns that no constraint reads: the cell is changed in the first column, in a random order, where the
    # oracle sees the change
    for c in rng.permutation(trace.shape[1]):
        bad = trace.copy()
        bad[r, c] = (int(bad[r, c]) + 1) % P
        want = O.check_trace(blob, bad, pis)
        if want[0] > 0:
            break
    assert want[0] > 0 and want[1][1] in (r - 1, r)
    assert prover.check_trace(air, bad, pis) == want
    assert prover.check_trace(air, bad.T.copy(), pis, layout=1) == want


def test_long_proof_through_a_verifying_pool(prover):
    air, cfg, trace, pis, _ = _case(0)
    proof = _proof(prover, 0)
    pool = S.ProofPool(0, big_contexts=1, small_contexts=1, verify_proofs=True)
    try:
        got = pool.wait(pool.submit(air, cfg, trace, pis, pow_witness=_pow(proof)))[0]
    finally:
        pool.close()
    assert np.array_equal(got, proof)


def test_verify_batch_over_the_long_proofs(prover):
    items = [(_case(i)[0], _case(i)[1], _proof(prover, i)) for i in range(len(PROOF_CASES))]
    tampered = items[2][2].copy()
    tampered[int(S.proof_layout(tampered).off_final_poly)] ^= np.uint64(1)
    items.append((items[2][0], items[2][1], tampered))
    want = []
    for air, cfg, proof in items:
        try:
            S.verify_stark_proof(air, cfg, proof)
            want.append(0)
        except S.StarkhipError as e:
            want.append(e.code)
    assert want == [0, 0, 0, 0, S.ERR_VERIFY]
    assert prover.verify_batch(items) == want


def test_the_row_rule(prover):
    n = 16384
    fib = S.register_air(S.air_program(S.AIR_TEST_FIBONACCI), name="FibonacciLong", default_rows=n)
    t, pis = S.trace_fibonacci(3, 5, n)
    cfg = S.StarkConfig.standard_fast_config()
    proof = prover.prove(fib, cfg, t, pis)
    S.verify_stark_proof(fib, cfg, proof)
    assert np.array_equal(proof, O.prove(S.air_program(fib), cfg, S.trace_rows_to_poly_values(t), pis, _pow(proof)))
    with pytest.raises(S.StarkhipError) as e:
        prover.prove(S.AIR_TEST_FIBONACCI, cfg, t, pis)
    assert e.value.code == S.ERR_BAD_SHAPE
    # 2^21 rows of a registered AIR: refused from the row count alone (the buffer is one row long and never read)
    n_cols = S.air_columns(fib)
    one_row = np.zeros(n_cols, dtype=np.uint64)
    out, words = C.POINTER(C.c_uint64)(), C.c_size_t()
    p = np.ascontiguousarray(pis, dtype=np.uint64)
    rc = S.lib.starkhip_prove(prover._ctx, fib, C.byref(cfg), one_row.ctypes.data_as(C.c_void_p), 1 << 21, n_cols, 0, 0,
                              p.ctypes.data_as(C.POINTER(C.c_uint64)), p.size, S.POW_SEARCH, C.byref(out), C.byref(words))
    assert rc == S.ERR_BAD_SHAPE
    assert S.MAX_LOG_ROWS == 20
