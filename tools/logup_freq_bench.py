"""Times the fill of LogUp frequencies.

(1) starkhip_logup_frequencies (Prover.logup_frequencies_device) on a device-resident, column-major trace with a 16-bit range table:
2^16 and 2^20 rows, one lookup of m = 1 and of m = 16 limb columns, limbs uniform and all equal, and both forms of the count kernel
("logup_count_combine" = 1: equal positions of a wave added as one; 0: every cell alone).  Two warm-up calls per case, then eleven:
the library's split of each call (starkhip_logup_frequency_timings: upload, table sort, count, write from events on the stream;
read-back the host's time in the copies), the median of each phase, and the median wall time of the call from Python.  Beside it,
from the same run: the numpy count on the host (bincount over searchsorted in the table's distinct values), which is what a caller
did before.  The filled column is compared with that count at every case.

(2) The fill inside prove(): tools/logup_bench.py's degree-3 AIR (300 columns, eight 16-bit range checks) at 2^12 and 2^16 rows,
"fill_frequencies" = 1 on a trace whose frequencies column is zeroed against the pre-filled trace with the option off, the two
alternating, median of five, beside the numpy count of the same trace.

Prints one JSON document and, with an argument, writes it to that file."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (its HIP runtime has to be the process's first)

import logup_bench as B  # noqa: E402
import starky_bls12_381_amd as S  # noqa: E402
from starky_bls12_381_amd.air_builder import AirBuilder  # noqa: E402

WARMUP, REPS, PROVE_REPS = 2, 11, 5
PHASES = ("upload", "sort", "count", "write", "read_back")


def median(ts):
    return sorted(ts)[len(ts) // 2]


def range_air(m):
    """m + 2 columns: the limbs 0 .. m - 1, the table m, the frequencies m + 1"""
    b = AirBuilder(m + 2, 0, 3)
    b.constraint(b.L(0) - b.L(0))
    b.logup(list(range(m)), m, m + 1)
    return S.register_air(b.finish(), name="LogupFreqBench_m%d" % m)


def numpy_count(cols, m):
    """the host's count: f over the table's rows, all of a value's count on its lowest row"""
    uniq, first = np.unique(cols[m], return_index=True)
    pos = np.searchsorted(uniq, cols[:m].reshape(-1))
    assert (uniq[np.minimum(pos, len(uniq) - 1)] == cols[:m].reshape(-1)).all()
    f = np.zeros(cols.shape[1], dtype=np.uint64)
    f[first] = np.bincount(pos, minlength=len(uniq)).astype(np.uint64)
    return f


def measure(pv, n, m, kind, rng):
    cols = np.zeros((m + 2, n), dtype=np.uint64)  # column-major
    cols[:m] = rng.integers(0, 1 << 16, (m, n), dtype=np.uint64) if kind == "uniform" else 0
    cols[m] = np.arange(n, dtype=np.uint64) % np.uint64(1 << 16)
    air = range_air(m)
    t0 = time.perf_counter()
    want = numpy_count(cols, m)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    out = {"rows": n, "m": m, "limbs": kind, "numpy_count_on_the_host_ms": round(numpy_ms, 3)}
    for combine in (1, 0):
        pv.set_option("logup_count_combine", combine)
        dev = torch.from_numpy(cols.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        calls, splits = [], []
        for it in range(WARMUP + REPS):
            rep = pv.logup_frequencies_device(air, dev.data_ptr(), n, m + 2, layout=1)
            assert rep.failed == 0
            if it >= WARMUP:
                calls.append(pv.last_call_s * 1e3)
                splits.append(rep.timings)
        assert np.array_equal(dev.cpu().numpy().view(np.uint64)[m + 1], want)
        form = {"call_ms_median": round(median(calls), 4), "call_ms": [round(x, 4) for x in calls],
                "phase_ms_median": {p: round(median([s[p] for s in splits]), 4) for p in PHASES}}
        form["numpy_over_call"] = round(numpy_ms / form["call_ms_median"], 2)
        out["combine" if combine else "plain"] = form
    pv.set_option("logup_count_combine", 1)
    return out


def measure_prove(n, rng):
    air = B.make_air("logup", 3)
    cfg = S.StarkConfig.for_air(air)
    filled, freq_ms = B.make_trace(n, rng)
    zeroed = filled.copy()
    zeroed[:, B.FREQ] = 0
    provers = {"prefilled_option_off": (S.Prover(0), filled), "zeroed_fill_frequencies": (S.Prover(0), zeroed)}
    provers["zeroed_fill_frequencies"][0].set_option("fill_frequencies", 1)
    ms = {k: [] for k in provers}
    fill_ms = []
    proofs = {}
    for rep in range(PROVE_REPS + 1):  # the first round is the warm-up
        for name, (pv, trace) in provers.items():
            t0 = time.perf_counter()
            proofs[name] = pv.prove(air, cfg, trace, [])
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                ms[name].append(wall)
                if name == "zeroed_fill_frequencies":
                    fill_ms.append(pv.last_logup_frequency_timings())
    assert np.array_equal(proofs["prefilled_option_off"], proofs["zeroed_fill_frequencies"])
    for pv, _ in provers.values():
        pv.close()
    out = {"rows": n, "columns": B.WIDTH, "range_checks": len(B.INPUTS), "reps": PROVE_REPS, "same_proof_bytes": True,
           "numpy_frequencies_ms": round(freq_ms, 3), "ms_median": {k: round(median(v), 3) for k, v in ms.items()},
           "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "fill_phase_ms_median": {p: round(median([x[p] for x in fill_ms]), 4) for p in PHASES}}
    out["fill_minus_prefilled_ms"] = round(out["ms_median"]["zeroed_fill_frequencies"] - out["ms_median"]["prefilled_option_off"], 3)
    return out


def main():
    torch.cuda.set_device(0)
    rng = np.random.default_rng(31)
    pv = S.Prover(0)
    alone = [measure(pv, n, m, kind, rng) for n in (1 << 16, 1 << 20) for m in (1, 16) for kind in ("uniform", "equal")]
    pv.close()
    in_prove = [measure_prove(n, rng) for n in (1 << 12, 1 << 16)]
    doc = {"what": "milliseconds.  alone: Prover.logup_frequencies_device on a column-major trace in device memory, %d warm-up calls, then %d; "
                   "phase_ms: starkhip_logup_frequency_timings, call_ms: wall time from Python around the call; combine / plain: the two forms "
                   "of the count kernel.  in_prove: host rows in, proof out, wall time from Python, the two cases alternating, median of %d"
                   % (WARMUP, REPS, PROVE_REPS),
           "alone": alone, "in_prove": in_prove}
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
