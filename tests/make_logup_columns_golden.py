"""Writes tests/golden/logup_columns_small.json: one proof per hasher of the case "mixed" of tests/logup_columns_ref.py (one lookup of
three Columns at degree 3: a next-row term with coefficient p - 1, a selector filter, a constant Column under a product filter that is
0 on every row) on 32 rows with num_query_rounds 3, proved on GPU 0 and accepted by the CPU verifier, the device verifier's replay and
the Python mini-verifier before it is written.
Run from the repository root on a machine with a GPU:  python tests/make_logup_columns_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import logup_columns_ref as G  # noqa: E402
import starky_bls12_381_amd as S  # noqa: E402
from logup_columns_util import GOLDEN, GOLDEN_CASE, GOLDEN_ROWS, GOLDEN_SEED, golden_case  # noqa: E402


def main(out_path=GOLDEN):
    air, blob, cfg, trace, pis = golden_case()
    prover = S.Prover(0)
    proofs = {}
    for hasher in (S.HASHER_POSEIDON, S.HASHER_KECCAK):
        prover.set_option("hasher", hasher)
        proof = prover.prove(air, cfg, trace, pis)
        again = prover.prove(air, cfg, trace, pis)
        assert (proof == again).all()
        assert S.proof_hasher(proof) == hasher and int(proof[13]) == 0 and int(proof[14]) == S.air_logup_polys(air) == 6 and int(proof[15]) == 0
        S.verify_stark_proof(air, cfg, proof)
        assert S.verify_batch_replay([(air, cfg, proof)]) == [0]
        G.verify_or_raise(blob, cfg, proof, hasher)
        proofs[str(hasher)] = ["%x" % int(w) for w in proof]
        print("hasher", hasher, proof.size, "words")
    prover.close()
    doc = {"air": "logup_columns_ref.CASES[%r]" % GOLDEN_CASE, "rows": GOLDEN_ROWS, "seed": GOLDEN_SEED,
           "config": {n: int(getattr(cfg, n)) for n, _ in S.StarkConfig._fields_}, "proofs_hex": proofs}
    with open(out_path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main(*sys.argv[1:2])
