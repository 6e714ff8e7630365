"""Times starkhip_lookup_columns (Prover.lookup_columns_device) on a device-resident, column-major trace: 2^16 and 2^20 rows, one lookup
and eight lookups (eight inputs, one shared 16-bit range table) per call.  Two warm-up calls per shape, then eleven: the library's
split of each call into upload / gather, sort, placement and read-back (starkhip_lookup_timings: events on the stream, summed over
the call's lookups), the median of each phase, and the median wall time of the call from Python (it ends in the library's wait for
the stream).  Beside it, from the same run on the same box:
  * starkhip_check_trace_permutations on the filled trace for the single pair (input, permuted_input): the same sort over the same
    number of items, then a classification instead of the placement -- the natural yardstick;
  * the numpy reference of tests/lookup_ref.py on the host, per lookup.
and the ratios.  The filled trace is compared with the reference at every shape.  Prints one JSON document and, with an argument,
writes it to that file."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (its HIP runtime has to be the process's first)

import lookup_ref as R  # noqa: E402
import starky_bls12_381_amd as S  # noqa: E402
from starky_bls12_381_amd.air_builder import AirBuilder  # noqa: E402

WARMUP, REPS = 2, 11
PHASES = ("upload", "sort", "place", "read_back")


def median(ts):
    return sorted(ts)[len(ts) // 2]


def make_trace(n, n_lookups, rng):
    """column-major [1 + 3 k][n]: k inputs, the table, then (permuted_input, permuted_table) per lookup"""
    k = n_lookups
    cols = np.zeros((1 + 3 * k, n), dtype=np.uint64)
    cols[:k] = rng.integers(0, 1 << 16, (k, n), dtype=np.uint64)
    cols[k] = np.arange(n, dtype=np.uint64) % np.uint64(1 << 16)
    return cols, [(q, k, k + 1 + 2 * q, k + 2 + 2 * q) for q in range(k)]


def pair_air(n_cols, lhs, rhs):
    b = AirBuilder(n_cols, 0, 2)
    b.constraint(b.L(0) - b.L(0))
    b.permutation_pair([(lhs, rhs)])
    return S.register_air(b.finish(), name="LookupBench_pair_%d" % n_cols)


def measure(pv, n, n_lookups, rng):
    cols, lookups = make_trace(n, n_lookups, rng)
    want = R.fill(cols, lookups, layout=1)[0]
    t0 = time.perf_counter()
    for (i, t, _, _) in lookups:
        R.reference(cols[i], cols[t])
    numpy_ms = (time.perf_counter() - t0) * 1e3
    dev = torch.from_numpy(cols.view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    calls, splits = [], []
    for it in range(WARMUP + REPS):
        rep = pv.lookup_columns_device(dev.data_ptr(), n, cols.shape[0], lookups, layout=1)
        assert rep.failed == 0
        if it >= WARMUP:
            calls.append(pv.last_call_s * 1e3)
            splits.append(rep.timings)
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), want)
    out = {"rows": n, "lookups": n_lookups, "columns": int(cols.shape[0]),
           "call_ms_median": round(median(calls), 4), "call_ms": [round(x, 4) for x in calls],
           "phase_ms_median": {p: round(median([s[p] for s in splits]), 4) for p in PHASES},
           "numpy_reference_on_the_host_ms": round(numpy_ms, 3)}
    device_ms = sum(out["phase_ms_median"].values())
    out["device_ms_median_sum_of_phases"] = round(device_ms, 4)
    out["numpy_over_call"] = round(numpy_ms / out["call_ms_median"], 2)
    out["place_over_sort"] = round(out["phase_ms_median"]["place"] / out["phase_ms_median"]["sort"], 3)
    if n_lookups == 1:
        air = pair_air(cols.shape[0], lookups[0][0], lookups[0][2])
        pcalls, psplits = [], []
        for it in range(WARMUP + REPS):
            prep = pv.check_trace_permutations_device(air, dev.data_ptr(), n, layout=1)
            assert prep.pairs_violated == 0
            if it >= WARMUP:
                pcalls.append(pv.last_call_s * 1e3)
                psplits.append(pv.last_perm_check_timings())
        out["check_trace_permutations_same_pair"] = {
            "call_ms_median": round(median(pcalls), 4),
            "phase_ms_median": {p: round(median([s[p] for s in psplits]), 4) for p in ("upload", "sort", "classify", "read_back")}}
        out["call_over_check_trace_permutations_call"] = round(out["call_ms_median"] / median(pcalls), 3)
    return out


def main():
    torch.cuda.set_device(0)
    rng = np.random.default_rng(17)
    pv = S.Prover(0)
    doc = {"what": "milliseconds of Prover.lookup_columns_device on a column-major trace in device memory: %d warm-up calls, then %d; "
                   "phase_ms: starkhip_lookup_timings (events on the stream, summed over the call's lookups; place = mark + scan + the two "
                   "placements), call_ms: wall time from Python around the call" % (WARMUP, REPS),
           "runs": [measure(pv, n, k, rng) for n in (1 << 16, 1 << 20) for k in (1, 8)]}
    pv.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
