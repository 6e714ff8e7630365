"""The quotient by constraint class on the GPU ("quotient_cosets" = 0, the default: every constraint on the cosets its degree needs,
the classes' values recombined into coefficient chunks) against every constraint on every coset ("quotient_cosets" = 1) and the CPU
oracle: the three proofs are the same bytes.  The shapes are the smallest of every path the kernels take."""
import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from bls_util import random_fp12
from quotient_classes_util import class_air

pytestmark = pytest.mark.gpu


def _fp12_mul():
    air = S.AIR_FP12_MUL  # 16 rows: the kernel for fewer rows than a wave has lanes, two cosets in one 64-point block
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED7100), random_fp12(0x5EED7101))
    return air, S.StarkConfig.for_air(air), t, pis


def _ecc_aggregate():
    from test_ecc_aggregate_cpu import pack, reference_vector
    air = S.AIR_ECC_AGGREGATE  # degree 4: three chunks on four cosets, the spare coset checks them
    pts, bits, _ = reference_vector()
    t, pis = S.trace_ecc_aggregate(*pack(pts, bits))
    return air, S.StarkConfig.for_air(air), t, pis


def _registered(n, top, degree, rate_bits=None):
    blob, trace, pis = class_air(n, top=top, degree=degree)
    air = S.register_air(blob, name=f"classes{n}_{top}_{degree}", default_rows=n)
    cfg = S.StarkConfig.for_air(air)
    if rate_bits is not None:
        cfg.rate_bits = rate_bits
    return air, cfg, trace, pis


CASES = {
    "fp12_mul_16_rows": _fp12_mul,
    "ecc_aggregate_factor_3_on_4_cosets": _ecc_aggregate,
    "all_classes_and_kinds_64_rows": lambda: _registered(64, 4, 5),     # one 64-point block per coset
    "all_classes_and_kinds_128_rows": lambda: _registered(128, 4, 5),   # two blocks per coset
    "degree_3_at_rate_bits_3": lambda: _registered(64, 2, 3, 3),        # two quotient cosets among eight LDE cosets
    "empty_top_classes": lambda: _registered(64, 2, 5),                 # cosets 2 and 3 have no chunk at all
}


@pytest.mark.parametrize("case", list(CASES))
def test_proofs_by_class_and_on_every_coset_are_the_oracles_bytes(prover, case):
    air, cfg, trace, pis = CASES[case]()
    proofs = []
    try:
        for cosets in (0, 1):
            prover.set_option("quotient_cosets", cosets)
            proofs.append(prover.prove(air, cfg, trace, pis))
    finally:
        prover.set_option("quotient_cosets", 0)
    assert np.array_equal(proofs[0], proofs[1])
    pow_witness = int(proofs[0][int(S.proof_layout(proofs[0]).off_pow_witness)])
    ref = O.prove(S.air_program(air), cfg, S.trace_rows_to_poly_values(trace), pis, pow_witness)
    assert proofs[0].size == ref.size and np.array_equal(proofs[0], ref)
    S.verify_stark_proof(air, cfg, proofs[0])
