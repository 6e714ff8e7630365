"""Measurements of long traces on one GPU -> JSON (`python tools/experiments/long_trace_measure.py profiles/long_trace_lde_and_phases.json`
regenerates that file; the recorded one holds the wave-kernel row and the 2^16 and 2^18 proofs only): starkhip_lde_bench at 512 x 2^13 through
both resident kernels and at 64 x 2^16 and 64 x 2^20 through the multi-workgroup transform (three warm launches, ten timed ones, each
shape twice in alternation), then the phase and host times of whole proofs of random AIRs at 2^16, 2^18 and 2^20 rows (the last: vectors
of 2^21 words), each proved three times on a warm context and accepted by starkhip_verify."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import starky_bls12_381_amd as S  # noqa: E402
from random_air import random_air  # noqa: E402


def main(out_path):
    out = {"lde_bench": [], "proofs": []}
    p = S.Prover(0)
    shapes = ((512, 13, "lde_columns_v2_kernel", 1), (512, 13, "lde_columns_wave_kernel", 0), (64, 16, "long 8 + 8", 0), (64, 20, "long 10 + 10", 0))
    for cols, log_n, kernel, impl in shapes * 2:
        p.set_option("lde_impl", impl)
        p.lde_bench(cols, log_n, 1, reps=3)  # warm: tables, buffers, clocks
        each = p.lde_bench(cols, log_n, 1, reps=10, each=True)
        out["lde_bench"].append({"cols": cols, "log_n": log_n, "rate_bits": 1, "kernel": kernel, "ms_each": each, "median_ms": statistics.median(each),
                                 "min_ms": min(each), "max_ms": max(each), "ns_per_input_word": statistics.median(each) * 1e6 / (cols << log_n)})
        print(out["lde_bench"][-1], flush=True)
    p.set_option("lde_impl", 0)
    for seed, cols, deg, rows in ((22, 12, 3, 1 << 16), (22, 12, 3, 1 << 18), (21, 5, 3, 1 << 20)):
        blob, trace, pis = random_air(seed, cols, deg, rows)
        air = S.register_air(blob, default_rows=rows)
        cfg = S.StarkConfig.for_air(air)
        runs = []
        for _ in range(3):
            proof = p.prove(air, cfg, trace, pis)
            runs.append({"call_s": p.last_call_s, "phases_ms": p.last_timings(), "host_ms": p.last_host_timings(), "kernels_ms": p.last_kernel_timings()})
        S.verify_stark_proof(air, cfg, proof)
        out["proofs"].append({"seed": seed, "cols": cols, "degree": deg, "rows": rows, "rate_bits": cfg.rate_bits, "verified": True, "runs": runs})
        print(json.dumps(runs[-1]), flush=True)
    p.close()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
