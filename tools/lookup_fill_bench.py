"""End to end, host rows in and proof out, for an AIR with five lookups (five inputs, two 16-bit range tables, degree 5, rate_bits 2)
at 2^16 and 2^20 rows -- three ways to get from a trace whose permuted columns are unfilled to its proof:
  (a) prove with "fill_lookups" on the AIR registered with its lookups: one upload, the fill on the prover's own copy;
  (b) Prover.lookup_columns on the host trace (columns up, columns back), then prove with the option off;
  (c) the numpy reference of tests/lookup_ref.py on the host, then prove with the option off.
One warm-up of each path per shape, then REPS rounds with the three paths alternating inside a round; wall time from Python around
each path (every path ends in the library's wait for its stream), the median, and for (a) the prover's phase 0 and the fill's own
split (starkhip_lookup_timings).  The three proofs of a shape are compared byte for byte.  Prints one JSON document and, with an
argument, writes it to that file."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import lookup_ref as R  # noqa: E402
import starky_bls12_381_amd as S  # noqa: E402
from starky_bls12_381_amd.air_builder import AirBuilder  # noqa: E402

REPS = 5
N_COLS = 17
LOOKUPS = [(q, 5 if q < 3 else 6, 7 + 2 * q, 8 + 2 * q) for q in range(5)]


def median(ts):
    return sorted(ts)[len(ts) // 2]


def make_trace(n, rng):
    t = rng.integers(1, 1 << 31, (n, N_COLS), dtype=np.uint64)
    t[:, :5] = rng.integers(0, 1 << 16, (n, 5), dtype=np.uint64)
    t[:, 5] = np.arange(n, dtype=np.uint64) % np.uint64(1 << 16)
    t[:, 6] = rng.permutation(t[:, 5])
    return t


def measure(filler, plain, air, cfg, n, rng, reps):
    trace = make_trace(n, rng)

    def path_a():
        return filler.prove(air, cfg, trace, [])

    def path_b():
        t = trace.copy()
        assert plain.lookup_columns(t, LOOKUPS, cap=0).failed == 0
        return plain.prove(air, cfg, t, [])

    def path_c():
        return plain.prove(air, cfg, R.fill(trace, LOOKUPS)[0], [])

    paths = (("a_fill_lookups_in_prove", path_a), ("b_lookup_columns_then_prove", path_b), ("c_numpy_reference_then_prove", path_c))
    proofs = [f() for _, f in paths]  # the warm-up
    assert all(np.array_equal(p, proofs[0]) for p in proofs)
    S.verify_stark_proof(air, cfg, proofs[0])
    ms = {name: [] for name, _ in paths}
    phase0, fill = [], []
    for _ in range(reps):
        for name, f in paths:
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            if name[0] == "a":
                phase0.append(filler.last_timings()["upload"])
                fill.append(filler.last_lookup_timings())
    out = {"rows": n, "columns": N_COLS, "lookups": len(LOOKUPS), "rate_bits": int(cfg.rate_bits), "reps": reps,
           "proofs_equal_and_verified": True,
           "ms_median": {k: round(median(v), 3) for k, v in ms.items()}, "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "a_phase0_upload_ms_median": round(median(phase0), 3),
           "a_fill_ms_median": {p: round(median([f[p] for f in fill]), 4) for p in ("upload", "sort", "place", "read_back")}}
    a = out["ms_median"]["a_fill_lookups_in_prove"]
    out["b_over_a"] = round(out["ms_median"]["b_lookup_columns_then_prove"] / a, 3)
    out["c_over_a"] = round(out["ms_median"]["c_numpy_reference_then_prove"] / a, 3)
    return out


def main():
    rng = np.random.default_rng(23)
    b = AirBuilder(N_COLS, 0, 5)
    for lk in LOOKUPS:
        b.lookup(*lk)
    air = S.register_air(b.finish(), name="LookupFillBench", default_rows=1 << 16, lookups=b.lookups)
    cfg = S.StarkConfig.for_air(air)
    filler, plain = S.Prover(0), S.Prover(0)
    filler.set_option("fill_lookups", 1)
    doc = {"what": "milliseconds from a host trace (row-major, permuted columns unfilled) to its proof in host memory, wall time from "
                   "Python; one warm-up per path, then the three paths alternating",
           "runs": [measure(filler, plain, air, cfg, n, rng, REPS if n < 1 << 20 else 3) for n in (1 << 16, 1 << 20)]}
    filler.close()
    plain.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
