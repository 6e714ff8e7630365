"""Writes tests/golden/keccak_fibonacci_2e6.json: a Fibonacci proof of 2^6 rows under the Keccak hasher (num_query_rounds 4), proved on
GPU 0 and accepted by the CPU verifier, the device verifier's replay and the Python mini-verifier before it is written.
Run from the repository root on a machine with a GPU:  python tests/make_keccak_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import keccak_ref as K  # noqa: E402
import starky_bls12_381_amd as S  # noqa: E402
from keccak_util import GOLDEN  # noqa: E402


def main(out_path=GOLDEN):
    air = S.AIR_TEST_FIBONACCI
    cfg = S.StarkConfig.standard_fast_config()
    cfg.num_query_rounds = 4
    t, pis = S.trace_fibonacci(3, 5, 64)
    prover = S.Prover(0)
    prover.set_option("hasher", S.HASHER_KECCAK)
    proof = prover.prove(air, cfg, t, pis)
    again = prover.prove(air, cfg, t, pis)
    prover.close()
    assert (proof == again).all()
    assert S.proof_hasher(proof) == S.HASHER_KECCAK
    S.verify_stark_proof(air, cfg, proof)
    assert S.verify_batch_replay([(air, cfg, proof)]) == [0]
    K.verify_or_raise(S.air_program(air), cfg, proof, K.KECCAK)
    doc = {"air": "fibonacci", "rows": 64, "x0": 3, "x1": 5, "hasher": 1,
           "config": {n: int(getattr(cfg, n)) for n, _ in S.StarkConfig._fields_},
           "proof_hex": ["%x" % int(w) for w in proof]}
    with open(out_path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out_path, proof.size, "words")


if __name__ == "__main__":
    main(*sys.argv[1:2])
