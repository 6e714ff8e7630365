"""End to end, host rows in and proof out, for an AIR of WIDTH columns with eight 16-bit range checks, at 2^12 and 2^16 rows under
standard_fast (rate_bits raised to what the degree needs) -- the same trace columns, declared five ways:
  logup_d3 / logup_d5   one LogUp lookup of the eight columns in the table column (AirBuilder.logup), frequencies from numpy;
  plain_d3 / plain_d5   the same AIR without the range checks;
  pairs_d5_fill         the eight checks as permutation-pair lookups (AirBuilder.lookup: 16 pairs, 16 witness columns) with
                        "fill_lookups" -- degree 5 is the least that holds them (four batches of four pairs).
One warm-up of each case per shape, then REPS rounds with the cases alternating inside a round; wall time from Python around prove()
(it ends in the library's wait for its stream), the median, and the per-phase split of starkhip_last_timings (median per phase).
Prints one JSON document and, with an argument, writes it to that file.  (profiles/logup.json also holds "terms_kernel": the quotient
phase of logup_d3 and the wall time of starkhip_logup_polys with one inversion per (row, challenge, lookup) against one per
denominator, taken in the same session from a build that still had both kernels; the slower one was then removed.)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402

import starky_bls12_381_amd as S  # noqa: E402
from starky_bls12_381_amd.air_builder import AirBuilder  # noqa: E402

REPS = 5
WIDTH = 300
INPUTS, TABLE, FREQ, WITNESS = list(range(2, 10)), 10, 11, 12  # eight range-checked columns, the table, the multiplicities; 16 witness columns of the pairs


def median(ts):
    return sorted(ts)[len(ts) // 2]


def make_air(kind, degree):
    b = AirBuilder(WIDTH, 0, degree)
    b.constraint(b.L(1) - b.L(0) * b.L(0))
    b.transition(b.N(0) - b.L(0) - 1)
    if kind == "logup":
        b.logup(INPUTS, TABLE, FREQ)
    elif kind == "pairs":
        for q, c in enumerate(INPUTS):
            b.lookup(c, TABLE, WITNESS + 2 * q, WITNESS + 2 * q + 1)
    return S.register_air(b.finish(), name="LogupBench_%s_d%d" % (kind, degree), lookups=b.lookups if kind == "pairs" else None)


def make_trace(n, rng):
    t = rng.integers(1, 1 << 31, (n, WIDTH), dtype=np.uint64)
    t[:, 0] = np.arange(5, 5 + n, dtype=np.uint64)
    t[:, 1] = t[:, 0] * t[:, 0]
    table = rng.permutation(n).astype(np.uint64) % np.uint64(1 << 16)  # 16-bit values; every value of the table occurs n / 65536 times or once
    t[:, TABLE] = table
    picks = rng.integers(0, min(n, 1 << 16), (n, len(INPUTS)))
    first = np.full(1 << 16, -1, dtype=np.int64)  # a value's multiplicity goes to the first row that holds it
    order = np.arange(n)[::-1]
    first[table[order]] = order
    t[:, INPUTS[0]:INPUTS[-1] + 1] = picks.astype(np.uint64)
    t0 = time.perf_counter()
    t[:, FREQ] = np.bincount(first[picks.reshape(-1)], minlength=n).astype(np.uint64)
    freq_ms = (time.perf_counter() - t0) * 1e3
    return t, freq_ms


def main():
    rng = np.random.default_rng(29)
    cases = [("logup_d3", "logup", 3, 0), ("plain_d3", "plain", 3, 0), ("logup_d5", "logup", 5, 0), ("plain_d5", "plain", 5, 0), ("pairs_d5_fill", "pairs", 5, 1)]
    airs = {name: make_air(kind, degree) for name, kind, degree, _ in cases}
    provers = {0: S.Prover(0), 1: S.Prover(0)}
    provers[1].set_option("fill_lookups", 1)
    runs = []
    for n in (1 << 12, 1 << 16):
        trace, freq_ms = make_trace(n, rng)
        ms = {name: [] for name, *_ in cases}
        phases = {name: [] for name, *_ in cases}
        for rep in range(REPS + 1):  # the first round is the warm-up
            for name, kind, degree, fill in cases:
                pv, air = provers[fill], airs[name]
                cfg = S.StarkConfig.for_air(air)
                t0 = time.perf_counter()
                proof = pv.prove(air, cfg, trace, [])
                wall = (time.perf_counter() - t0) * 1e3
                if rep == 0:
                    S.verify_stark_proof(air, cfg, proof)
                else:
                    ms[name].append(wall)
                    phases[name].append(pv.last_timings())
        out = {"rows": n, "columns": WIDTH, "range_checks": len(INPUTS), "reps": REPS, "proofs_verified": True,
               "numpy_frequencies_ms": round(freq_ms, 3),
               "ms_median": {k: round(median(v), 3) for k, v in ms.items()}, "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
               "phase_ms_median": {k: {p: round(median([x[p] for x in v]), 3) for p in v[0]} for k, v in phases.items()}}
        m = out["ms_median"]
        out["logup_d3_minus_plain_d3_ms"] = round(m["logup_d3"] - m["plain_d3"], 3)
        out["logup_d5_minus_plain_d5_ms"] = round(m["logup_d5"] - m["plain_d5"], 3)
        out["pairs_d5_fill_minus_plain_d5_ms"] = round(m["pairs_d5_fill"] - m["plain_d5"], 3)
        runs.append(out)
    for pv in provers.values():
        pv.close()
    doc = {"what": "milliseconds from a host trace (row-major) to its proof in host memory, wall time from Python; one warm-up per case, then "
                   "the cases alternating; phases from starkhip_last_timings (the LogUp and permutation work is timed with the quotient phase, "
                   "the fill of the pairs' witness columns with the upload)", "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
