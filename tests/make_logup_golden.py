"""Writes tests/golden/logup_small.json: one proof per hasher of the LogUp test AIR of degree 3 (two lookups of three columns in one
table: a helper batch of two and one of one each, nA = 12) on 16 rows with num_query_rounds 3, proved on GPU 0 and accepted by the CPU
verifier, the device verifier's replay and the Python mini-verifier before it is written.
Run from the repository root on a machine with a GPU:  python tests/make_logup_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import logup_ref as R  # noqa: E402
import starky_bls12_381_amd as S  # noqa: E402
from logup_util import GOLDEN, GOLDEN_DEGREE, GOLDEN_LOOKUPS, GOLDEN_M, GOLDEN_ROWS, GOLDEN_SEED, golden_case  # noqa: E402


def main(out_path=GOLDEN):
    air, blob, cfg, trace, pis = golden_case()
    prover = S.Prover(0)
    proofs = {}
    for hasher in (S.HASHER_POSEIDON, S.HASHER_KECCAK):
        prover.set_option("hasher", hasher)
        proof = prover.prove(air, cfg, trace, pis)
        again = prover.prove(air, cfg, trace, pis)
        assert (proof == again).all()
        assert S.proof_hasher(proof) == hasher and int(proof[13]) == 0 and int(proof[14]) == S.air_logup_polys(air) == 12
        S.verify_stark_proof(air, cfg, proof)
        assert S.verify_batch_replay([(air, cfg, proof)]) == [0]
        R.verify_or_raise(blob, cfg, proof, hasher)
        proofs[str(hasher)] = ["%x" % int(w) for w in proof]
        print("hasher", hasher, proof.size, "words")
    prover.close()
    doc = {"air": "logup_ref.make_air(%d, %d, %d)" % (GOLDEN_DEGREE, GOLDEN_M, GOLDEN_LOOKUPS), "rows": GOLDEN_ROWS, "seed": GOLDEN_SEED,
           "config": {n: int(getattr(cfg, n)) for n, _ in S.StarkConfig._fields_}, "proofs_hex": proofs}
    with open(out_path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main(*sys.argv[1:2])
