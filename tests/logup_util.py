"""What the LogUp tests (CPU and GPU) and the golden's maker share: the registered test AIRs, their configs, the golden case, the
tampered copies of a proof's new fields.  Test code."""
import json
import os

import numpy as np

import logup_ref as R
import starky_bls12_381_amd as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logup_small.json")
GOLDEN_ROWS, GOLDEN_SEED, GOLDEN_DEGREE, GOLDEN_M, GOLDEN_LOOKUPS = 16, 7, 3, 3, 2

_AIRS = {}


def logup_air(degree, m, n_lookups, extra=0):
    """(air id, blob) of logup_ref.make_air(degree, m, n_lookups, extra), registered once per process"""
    key = (degree, m, n_lookups, extra)
    if key not in _AIRS:
        blob = R.make_air(*key)
        _AIRS[key] = (S.register_air(blob, name="LogupTest_d%d_m%d_l%d_x%d" % key), blob)
    return _AIRS[key]


def m_cases(degree):
    """the three column counts of the tests: 1, a full batch, and a full batch plus a batch of one (at degree 2: 1 and two batches)"""
    return sorted({1, degree - 1, degree})


def logup_config(degree, num_query_rounds):
    """standard_fast with the smallest rate_bits the degree admits (what starkhip_config_for_air gives a registered AIR)"""
    cfg = S.StarkConfig.standard_fast_config()
    while (1 << cfg.rate_bits) + 1 < degree:
        cfg.rate_bits += 1
    cfg.num_query_rounds = num_query_rounds
    return cfg


def golden_case():
    """(air, blob, config, trace, public inputs) of the golden proofs: degree 3, two lookups of three columns (a batch of two and a
    batch of one each: nA = 12), 16 rows, 3 query rounds"""
    air, blob = logup_air(GOLDEN_DEGREE, GOLDEN_M, GOLDEN_LOOKUPS)
    trace, pis = R.make_trace(GOLDEN_DEGREE, GOLDEN_M, GOLDEN_LOOKUPS, GOLDEN_ROWS, GOLDEN_SEED)
    return air, blob, logup_config(GOLDEN_DEGREE, 3), trace, pis


def load_golden():
    """{hasher id: proof} of tests/golden/logup_small.json (tests/make_logup_golden.py wrote it on the GPU)"""
    with open(GOLDEN) as f:
        d = json.load(f)
    return {int(h): np.array([int(x, 16) for x in words], dtype=np.uint64) for h, words in d["proofs_hex"].items()}


def logup_flips(proof):
    """{name: tampered copy}: one word raised by one mod p in each field a proof gains with nA > 0 -- the auxiliary cap, an auxiliary
    opening, an auxiliary-next opening, a word of a query round's auxiliary leaf and one of its siblings"""
    L = S.proof_layout(proof)
    g = lambda f: int(getattr(L, f))  # noqa: E731
    assert g("n_logup_polys") > 0 and g("n_permutation_zs") == 0 and g("n_query_rounds") > 0 and g("initial_sibling_count") > 0
    rnd = g("off_query_rounds") + (g("n_query_rounds") // 2) * g("query_round_words")
    pos = {"aux_cap": g("off_permutation_zs_cap") + 1, "aux_opening": g("off_permutation_zs") + 2, "aux_next_opening": g("off_permutation_zs_next") + 1,
           "aux_leaf": rnd + g("q_permutation_zs_leaf") + 1, "aux_sibling": rnd + g("q_permutation_zs_siblings") + 2}
    out = {}
    for name, p in pos.items():
        bad = np.array(proof, dtype=np.uint64, copy=True)
        bad[p] = (int(bad[p]) + 1) % S.P
        out[name] = bad
    return out


def cpu_code(air, cfg, proof):
    try:
        S.verify_stark_proof(air, cfg, proof)
        return 0
    except S.StarkhipError as e:
        return e.code
