"""Writes tests/golden/ctl_small.json: per hasher one system proof of the case "range" of tests/ctl_ref.py (32 rows look one column up,
under a selector filter, in a 16-row table whose filter is its multiplicity column) with num_query_rounds 3 (and of the case "two_lookers" at 16, 8 and 8 rows: `two_lookers_proofs_hex`), proved on GPU 0 and accepted by
the CPU system verifier and the Python mini-verifier before it is written -- and per hasher a second system proof of the same looking trace
beside a table trace whose own columns differ (`other_proofs_hex`: what the test of a table proof taken from another run splices from).
Run from the repository root on a machine with a GPU:  python tests/make_ctl_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import ctl_ref as X  # noqa: E402
import starky_bls12_381_amd as S  # noqa: E402
from ctl_util import GOLDEN, GOLDEN_CASE, GOLDEN_ROWS, GOLDEN_SEED, GOLDEN_TWO_CASE, GOLDEN_TWO_ROWS, golden_case, golden_two_case  # noqa: E402


def other_run(case, traces):
    """the same traces, but for the own columns (and public input) of the looked table: every CTL still balances"""
    t, _ = traces[1]
    rows, start = X.own_rows(case.tables[1], t.shape[0], np.random.default_rng(GOLDEN_SEED + 1))
    t = t.copy()
    t[:, :3] = np.array(rows, dtype=np.uint64)[:, :3]
    return [traces[0], (t, np.array([start], dtype=np.uint64))]


def main(out_path=GOLDEN):
    system, blobs, case, cfgs, traces = golden_case()
    prover = S.SystemProver(system, 0)
    proofs, others = {}, {}
    for hasher in (S.HASHER_POSEIDON, S.HASHER_KECCAK):
        prover.set_option("hasher", hasher)
        for dst, trs in ((proofs, traces), (others, other_run(case, traces))):
            proof = prover.prove(cfgs, [t for t, _ in trs], [p for _, p in trs])
            again = prover.prove(cfgs, [t for t, _ in trs], [p for _, p in trs])
            assert (proof == again).all()
            S.verify_system_proof(system, cfgs, proof)
            X.verify_system_or_raise(blobs, case.ctls, cfgs, proof, hasher)
            dst[str(hasher)] = ["%x" % int(w) for w in proof]
            print("hasher", hasher, proof.size, "words")
    prover.close()
    system2, blobs2, case2, cfgs2, traces2 = golden_two_case()
    prover2 = S.SystemProver(system2, 0)
    two = {}
    for hasher in (S.HASHER_POSEIDON, S.HASHER_KECCAK):
        prover2.set_option("hasher", hasher)
        proof = prover2.prove(cfgs2, [t for t, _ in traces2], [p for _, p in traces2])
        S.verify_system_proof(system2, cfgs2, proof)
        X.verify_system_or_raise(blobs2, case2.ctls, cfgs2, proof, hasher)
        two[str(hasher)] = ["%x" % int(w) for w in proof]
        print(GOLDEN_TWO_CASE, "hasher", hasher, proof.size, "words")
    prover2.close()
    doc = {"case": "ctl_ref.CASES[%r]" % GOLDEN_CASE, "rows": list(GOLDEN_ROWS), "seed": GOLDEN_SEED,
           "configs": [{n: int(getattr(cfg, n)) for n, _ in S.StarkConfig._fields_} for cfg in cfgs], "proofs_hex": proofs, "other_proofs_hex": others,
           "two_lookers": {"case": "ctl_ref.CASES[%r]" % GOLDEN_TWO_CASE, "rows": list(GOLDEN_TWO_ROWS), "seed": GOLDEN_SEED}, "two_lookers_proofs_hex": two}
    with open(out_path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main(*sys.argv[1:2])
