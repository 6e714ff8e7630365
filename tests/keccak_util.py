"""What the Keccak hasher's CPU and GPU tests share: the five flips of a proof and the three verifiers' verdicts.  Test code."""
import json
import os

import numpy as np

import keccak_ref as K
import starky_bls12_381_amd as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keccak_fibonacci_2e6.json")


def flips(proof):
    """{name: tampered copy}: one cap word, one opening, one sibling (where the proof has one), one final-polynomial word and the
    proof-of-work witness, each raised by one mod p."""
    L = S.proof_layout(proof)
    g = lambda f: int(getattr(L, f))  # noqa: E731
    pos = {"cap": g("off_trace_cap") + 1, "opening": g("off_local_values"), "final_poly": g("off_final_poly"),
           "witness": g("off_pow_witness")}
    if g("n_query_rounds") and g("initial_sibling_count"):
        pos["sibling"] = g("off_query_rounds") + (g("n_query_rounds") // 2) * g("query_round_words") + g("q_trace_siblings") + 2
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


def replay_code(air, cfg, proof):
    return S.verify_batch_replay([(air, cfg, proof)])[0]


def mini_ok(blob, cfg, proof, hasher):
    return K.verify(blob, cfg, proof, hasher)


def load_golden():
    """(config, proof) of tests/golden/keccak_fibonacci_2e6.json (tests/make_keccak_golden.py wrote it on the GPU)."""
    with open(GOLDEN) as f:
        d = json.load(f)
    cfg = S.StarkConfig.standard_fast_config()
    for name, v in d["config"].items():
        setattr(cfg, name, v)
    return cfg, np.array([int(x, 16) for x in d["proof_hex"]], dtype=np.uint64)
