"""A/B of the two hashers on one device, same build, same process: the FinalExp proof alone on one context, and a proof pool with
eight FinalExp-class contexts fed from operands the way bench.py feeds it.  Hasher 0 (Poseidon) and hasher 1 (Keccak) alternate,
`--rounds` rounds each after a warm-up round of each; the baseline is hasher 0 of the same run.  Reports the median and the range of
the whole proof, the trace commitment's leaf-hash kernel (starkhip_last_kernel_timings[1]) and the host's Fiat-Shamir time
(starkhip_last_host_timings[0]), and for the pool proofs per second.  One JSON document on stdout and in --out.

    python tools/hasher_ab.py --out profiles/keccak_hasher_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import starky_bls12_381_amd as S  # noqa: E402
from bls_util import random_fp12  # noqa: E402

NAMES = {0: "poseidon", 1: "keccak"}


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def lone(device, rounds):
    air = S.AIR_FINAL_EXP
    cfg = S.StarkConfig.for_air(air)
    trace, pis = S.trace_final_exp(random_fp12(0x5EED0001), compact=True)
    prover = S.Prover(device)
    samples = {h: {"proof_wall_ms": [], "proof_device_ms": [], "commit_leaf_hash_ms": [], "trace_merkle_phase_ms": [], "fiat_shamir_host_ms": [], "pow_phase_ms": []}
               for h in (0, 1)}
    try:
        for r in range(rounds + 1):  # round 0 warms both up (buffers, tables, plans, code objects)
            for h in (0, 1):
                prover.set_option("hasher", h)
                t0 = time.perf_counter()
                proof = prover.prove(air, cfg, trace, pis)
                wall = (time.perf_counter() - t0) * 1e3
                assert S.proof_hasher(proof) == h
                if r == 0:
                    S.verify_stark_proof(air, cfg, proof)
                    continue
                ph = prover.last_timings()
                s = samples[h]
                s["proof_wall_ms"].append(wall)
                s["proof_device_ms"].append(ph["total"])
                s["trace_merkle_phase_ms"].append(ph["trace_merkle"])
                s["pow_phase_ms"].append(ph["pow"])
                s["commit_leaf_hash_ms"].append(prover.last_kernel_timings()["leaf_hash"])
                s["fiat_shamir_host_ms"].append(prover.last_host_timings()["fiat_shamir"])
    finally:
        prover.set_option("hasher", 0)
        prover.close()
    return {NAMES[h]: {k: summary(v) for k, v in samples[h].items()} for h in (0, 1)}


def pooled(device, rounds, inflight, proofs_per_round):
    air = S.AIR_FINAL_EXP
    inputs = [random_fp12(0x5EED0100 + i) for i in range(inflight)]
    pool = S.ProofPool(device, big_contexts=inflight, small_contexts=1, warm_up=1)
    samples = {h: {"proofs_per_s": [], "commit_leaf_hash_ms": [], "fiat_shamir_host_ms": [], "proof_device_ms": []} for h in (0, 1)}
    forms = {0: set(), 1: set()}
    try:
        for r in range(rounds + 1):
            for h in (0, 1):
                pool.set_option("hasher", h)
                t0 = time.perf_counter()
                tickets = [pool.submit_witness(air, inputs[i % inflight]) for i in range(proofs_per_round)]
                infos = []
                for t in tickets:
                    proof, info = pool.wait(t)
                    assert S.proof_hasher(proof) == h
                    infos.append(info)
                    del proof
                dt = time.perf_counter() - t0
                if r == 0:
                    continue
                s = samples[h]
                s["proofs_per_s"].append(proofs_per_round / dt)
                s["commit_leaf_hash_ms"].append(statistics.median(i["kernel_ms"]["leaf_hash"] for i in infos))
                s["fiat_shamir_host_ms"].append(statistics.median(i["host_ms"]["fiat_shamir"] for i in infos))
                s["proof_device_ms"].append(statistics.median(i["phase_ms"]["total"] for i in infos))
                forms[h] |= {i["leaf_hash_form"] for i in infos}
    finally:
        pool.set_option("hasher", 0)
        pool.close()
    out = {NAMES[h]: {k: summary(v) for k, v in samples[h].items()} for h in (0, 1)}
    for h in (0, 1):
        out[NAMES[h]]["leaf_hash_forms"] = sorted(forms[h])
    out["in_flight"], out["proofs_per_round"] = inflight, proofs_per_round
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=8)
    ap.add_argument("--proofs-per-round", type=int, default=16)
    ap.add_argument("--skip-pool", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    doc = {"what": "FinalExp proofs under hasher 0 (Poseidon) and hasher 1 (Keccak), alternating in one process; per-round figures, "
                   "median / min / max over the rounds after one warm-up round of each",
           "air": "FinalExponentiateStark", "columns": S.air_columns(S.AIR_FINAL_EXP), "rows": S.air_default_rows(S.AIR_FINAL_EXP),
           "rounds": args.rounds, "lone_context": lone(args.device, args.rounds)}
    if not args.skip_pool:
        doc["pool"] = pooled(args.device, args.rounds, args.inflight, args.proofs_per_round)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
