"""What the permutation tests (CPU and GPU) and the golden's maker share: the golden AIR, trace and config, the registered test
AIRs, the tampered copies of a proof's new fields.  Test code."""
import json
import os

import numpy as np

import permutation_ref as R
import starky_bls12_381_amd as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "permutation_small.json")
GOLDEN_ROWS, GOLDEN_SEED, GOLDEN_DEGREE = 32, 7, 3

_AIRS = {}


def perm_air(degree, n_cols=6):
    """(air id, blob) of permutation_ref.make_air(degree, n_cols), registered once per process"""
    key = (degree, n_cols)
    if key not in _AIRS:
        blob = R.make_air(degree, n_cols)
        _AIRS[key] = (S.register_air(blob, name="PermTest_d%d_c%d" % key), blob)
    return _AIRS[key]


def perm_config(degree, num_query_rounds):
    """standard_fast with the smallest rate_bits the degree admits (what starkhip_config_for_air gives a registered AIR)"""
    cfg = S.StarkConfig.standard_fast_config()
    while (1 << cfg.rate_bits) + 1 < degree:
        cfg.rate_bits += 1
    cfg.num_query_rounds = num_query_rounds
    return cfg


def golden_case():
    """(air, blob, config, trace, public inputs) of the golden proofs: degree 3 (B = 2), 6 columns, three pairs in two batches, 32 rows"""
    air, blob = perm_air(GOLDEN_DEGREE)
    trace, pis = R.make_trace(GOLDEN_DEGREE, GOLDEN_ROWS, GOLDEN_SEED)
    return air, blob, perm_config(GOLDEN_DEGREE, 4), trace, pis


def load_golden():
    """{hasher id: proof} of tests/golden/permutation_small.json (tests/make_permutation_golden.py wrote it on the GPU)"""
    with open(GOLDEN) as f:
        d = json.load(f)
    return {int(h): np.array([int(x, 16) for x in words], dtype=np.uint64) for h, words in d["proofs_hex"].items()}


def perm_flips(proof):
    """{name: tampered copy}: one word raised by one mod p in each field a proof gains with nZ > 0 -- the Z cap, a Z opening, a Z-next
    opening, a word of a query round's Z leaf and one of its siblings"""
    L = S.proof_layout(proof)
    g = lambda f: int(getattr(L, f))  # noqa: E731
    assert g("n_permutation_zs") > 0 and g("n_query_rounds") > 0 and g("initial_sibling_count") > 0
    rnd = g("off_query_rounds") + (g("n_query_rounds") // 2) * g("query_round_words")
    pos = {"zs_cap": g("off_permutation_zs_cap") + 1, "zs_opening": g("off_permutation_zs") + 2, "zs_next_opening": g("off_permutation_zs_next") + 1,
           "zs_leaf": rnd + g("q_permutation_zs_leaf") + 1, "zs_sibling": rnd + g("q_permutation_zs_siblings") + 2}
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
