"""Measurements behind DESIGN.md's device-verifier section (starkhip_verify_batch), one JSON object on stdout.

  python tools/verify_device_probe.py split      the CPU verifier's time per AIR split into prelude (the device path's prelude of
                                                 one proof on one thread) and queries (the rest), over the 48 proofs of 8 signatures,
                                                 then the whole batch on the CPU verifier and on the device
  python tools/verify_device_probe.py latency    chain latency per permutation of the row and the quad leaf-hash forms: one wave of
                                                 64 leaves of `--cols` words (merkle_cap with leaf_hash_form 2 / 1); run it under
                                                 rocprofv3 --kernel-trace --stats and divide the kernels' durations by cols / 8
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import starky_bls12_381_amd as S  # noqa: E402

NAMES = {S.AIR_PAIRING_PRECOMP: "PairingPrecomp", S.AIR_MILLER_LOOP: "MillerLoop", S.AIR_FP12_MUL: "FP12Mul", S.AIR_FINAL_EXP: "FinalExp"}


def signature_batch(batch):
    from bls_util import native_vectors
    from starky_bls12_381_amd import signature as G
    sigs = G.synthetic_signatures(batch, native_vectors()["bls_signature"], seed=0x8516)
    mine = G.plan_batch(batch, 1)[0]
    pool = S.ProofPool(0, big_contexts=6, small_contexts=12, stream_priority=1, warm_up=1)
    try:
        _, results, _, _, _ = G.one_step(None, batch, pool, mine, sigs)
    finally:
        pool.close()
    return [(air, cfg, proof) for _, (air, proof, cfg) in sorted(results.items())]


def split(args):
    items = signature_batch(args.batch)
    prover = S.Prover(0)
    prover.verify_batch(items[:1])
    per_air = {}
    for air, cfg, proof in items:
        t0 = time.perf_counter()
        S.verify_stark_proof(air, cfg, proof)
        total = (time.perf_counter() - t0) * 1e3
        assert prover.verify_batch([(air, cfg, proof)]) == [0]
        pre = prover.last_verify_timings()["prelude_ms"]
        d = per_air.setdefault(NAMES[air], {"proofs": 0, "cpu_verify_ms": 0.0, "prelude_ms": 0.0})
        d["proofs"] += 1
        d["cpu_verify_ms"] += total
        d["prelude_ms"] += pre
    for d in per_air.values():
        for k in ("cpu_verify_ms", "prelude_ms"):
            d[k] = round(d[k] / d["proofs"], 2)
        d["queries_ms"] = round(d["cpu_verify_ms"] - d["prelude_ms"], 2)
    c0, t0 = time.process_time(), time.perf_counter()
    for it in items:
        S.verify_stark_proof(*it)
    cpu = {"wall_s": round(time.perf_counter() - t0, 3), "cpu_s": round(time.process_time() - c0, 2)}
    t0 = time.perf_counter()
    assert prover.verify_batch(items) == [0] * len(items)
    dev = {"wall_s": round(time.perf_counter() - t0, 3)}
    dev.update({k: round(v, 3) for k, v in prover.last_verify_timings().items()})
    prover.close()
    print(json.dumps({"proofs": len(items), "per_air": per_air, "cpu_verifier_batch": cpu, "device_verifier_batch": dev}))


def latency(args):
    prover = S.Prover(0)
    rng = np.random.default_rng(7)
    lde = rng.integers(0, S.P, size=(args.cols, 64), dtype=np.uint64)  # 64 leaves (log N = 6) of `cols` words: one chain per leaf
    caps = {}
    for form, name in ((2, "row"), (1, "quad"), (2, "row"), (1, "quad")):
        prover.set_option("leaf_hash_form", form)
        t0 = time.perf_counter()
        caps[name] = prover.merkle_cap(lde, 0)
        caps[name + "_wall_ms"] = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(caps["row"], caps["quad"])
    prover.close()
    print(json.dumps({"cols": args.cols, "permutations_per_chain": (args.cols + 7) // 8, "row_wall_ms": round(caps["row_wall_ms"], 3),
                      "quad_wall_ms": round(caps["quad_wall_ms"], 3)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("split", "latency"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--cols", type=int, default=16384)
    a = ap.parse_args()
    split(a) if a.mode == "split" else latency(a)
