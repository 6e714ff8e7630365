"""Traces of more than 8192 rows without a GPU: the registration bound, the index model of the multi-workgroup transform
(tools/lde_long_model.py) against a plain NTT, and the host verifiers on an oracle-made proof of a registered AIR at 2^14 rows."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from random_air import random_air

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import lde_long_model as M  # noqa: E402


def test_default_rows_up_to_two_to_the_twenty():
    blob, _, _ = random_air(31, 4, 3, 16)
    air = S.register_air(blob, name="long_default_rows", default_rows=1 << 16)
    assert S.air_default_rows(air) == 1 << 16
    assert S.MAX_LOG_ROWS == 20
    blob2, _, _ = random_air(32, 4, 3, 16)
    assert S.air_default_rows(S.register_air(blob2, default_rows=1 << 20)) == 1 << 20
    blob3, _, _ = random_air(33, 4, 3, 16)
    for rows in (1 << 21, (1 << 16) + 1, 3 << 14):
        with pytest.raises(S.StarkhipError) as e:
            S.register_air(blob3, default_rows=rows)
        assert e.value.code == S.ERR_BAD_SHAPE


@pytest.mark.parametrize("log_n,rate_bits", [(log_n, 1) for log_n in range(14, 21)] + [(log_n, r) for log_n in (14, 15) for r in (0, 2, 3)])
def test_index_model_agrees_with_a_plain_ntt(log_n, rate_bits):
    found = M.check(log_n, rate_bits)
    assert found["out_of_bounds"] == 0
    assert found["read_conflicts"] == 0 and found["write_conflicts"] == 0
    assert found["lds_words"] * 8 <= 160 * 1024


def test_index_model_with_narrower_tiles():
    """2^21 words = 2^10 x 2^11: tiles of 16 and of 8 words.  The scattered LDS writes of 8-word rows are two-way conflicts, as
    csrc/kernels_lde_long.hip says; reads are conflict-free."""
    found = M.check_vector(21)
    assert found["tile_words"] == (16, 8)
    assert found["out_of_bounds"] == 0 and found["read_conflicts"] == 0
    assert found["lds_words"] * 8 <= 160 * 1024


def test_host_verifiers_on_an_oracle_proof_of_16384_rows():
    blob, trace, pis = random_air(21, 5, 3, 1 << 14)
    air = S.register_air(blob, name="long21", default_rows=1 << 14)
    cfg = S.StarkConfig.for_air(air)
    assert cfg.rate_bits == 1
    proof = O.prove(blob, cfg, trace.T.copy(), pis)
    S.verify_stark_proof(air, cfg, proof)
    tampered = proof.copy()
    tampered[int(S.proof_layout(proof).off_local_values)] ^= np.uint64(1)  # one word of the openings
    with pytest.raises(S.StarkhipError) as e:
        S.verify_stark_proof(air, cfg, tampered)
    assert e.value.code == S.ERR_VERIFY
    assert S.verify_batch_replay([(air, cfg, proof), (air, cfg, tampered)]) == [0, S.ERR_VERIFY]
