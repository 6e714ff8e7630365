"""What a cross-table lookup costs and what it buys, end to end from host rows to the proof in host memory: a table of WIDTH columns
(2^16 or 2^20 rows) whose column 3 is range-checked, under the selector in column 4, against a 16-bit table of 2^16 rows, three ways:
  system      the two AIRs as one system with one CTL (SystemProver; the small table is committed once, at its own height);
  standalone  the same two AIRs proved one after the other without the CTL (two Provers): the difference is the feature's price;
  copied      the check as one LogUp lookup inside the big trace, the table and its multiplicities copied into two more columns at the
              big trace's height: the difference is what the feature buys.
One warm-up of each case per shape, then REPS rounds with the cases alternating inside a round; wall time from Python around the
proving call, the median, and the per-phase split of starkhip_last_timings (median per phase; for the system and the standalone pair,
per table).  Prints one JSON document and, with an argument, writes it to that file."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402

import starky_bls12_381_amd as S  # noqa: E402
from starky_bls12_381_amd.air_builder import AirBuilder, Column, Filter, SystemBuilder  # noqa: E402

REPS = 5
WIDTH, SMALL_WIDTH, SMALL_ROWS = 40, 5, 1 << 16
VALUE, SELECTOR, TABLE, FREQ = 3, 4, WIDTH, WIDTH + 1  # (TABLE and FREQ: the two columns the copied form adds)


def median(ts):
    return sorted(ts)[len(ts) // 2]


def make_air(n_cols, name, copied=False):
    b = AirBuilder(n_cols, 0, 3)
    b.constraint(b.L(1) - b.L(0) * b.L(0))
    b.transition(b.N(0) - b.L(0) - 1)
    if copied:
        b.logup_columns([(VALUE, Filter(sums=[Column.single(SELECTOR)]))], TABLE, FREQ)
    return S.register_air(b.finish(), name=name)


def own(t):
    t[:, 0] = np.arange(5, 5 + t.shape[0], dtype=np.uint64)
    t[:, 1] = t[:, 0] * t[:, 0]


def make_traces(n, rng):
    big = rng.integers(1, 1 << 31, (n, WIDTH + 2), dtype=np.uint64)
    own(big)
    big[:, VALUE] = rng.integers(0, SMALL_ROWS, n).astype(np.uint64)
    big[:, SELECTOR] = rng.integers(0, 2, n).astype(np.uint64)
    counts = np.bincount(big[:, VALUE][big[:, SELECTOR] == 1].astype(np.int64), minlength=SMALL_ROWS).astype(np.uint64)
    small = np.zeros((SMALL_ROWS, SMALL_WIDTH), dtype=np.uint64)
    own(small)
    small[:, VALUE] = np.arange(SMALL_ROWS, dtype=np.uint64)
    small[:, SELECTOR] = counts
    big[:, TABLE] = np.arange(n, dtype=np.uint64) % np.uint64(SMALL_ROWS)  # the table at the big trace's height: a value's multiplicity on its first row
    big[:, FREQ] = 0
    big[:SMALL_ROWS, FREQ] = counts
    return np.ascontiguousarray(big[:, :WIDTH]), small, big


def main():
    rng = np.random.default_rng(31)
    big_air, small_air, copied_air = make_air(WIDTH, "CtlBench_big"), make_air(SMALL_WIDTH, "CtlBench_small"), make_air(WIDTH + 2, "CtlBench_copied", copied=True)
    sb = SystemBuilder([big_air, small_air])
    sb.ctl(looked=(1, [VALUE], Filter(sums=[Column.single(SELECTOR)])), looking=[(0, [VALUE], Filter(sums=[Column.single(SELECTOR)]))])
    system = S.register_system(sb.finish())
    sp, pv_big, pv_small, pv_copied = S.SystemProver(system, 0), S.Prover(0), S.Prover(0), S.Prover(0)
    cfg = S.StarkConfig.for_air(big_air)
    runs = []
    for n in (1 << 16, 1 << 20):
        big, small, copied = make_traces(n, rng)
        ms = {k: [] for k in ("system", "standalone", "copied")}
        phases = {k: [] for k in ("system_big", "system_small", "standalone_big", "standalone_small", "copied")}
        for rep in range(REPS + 1):  # the first round is the warm-up
            t0 = time.perf_counter()
            proof = sp.prove([cfg, cfg], [big, small], [[], []])
            t1 = time.perf_counter()
            p_big = pv_big.prove(big_air, cfg, big, [])
            p_small = pv_small.prove(small_air, cfg, small, [])
            t2 = time.perf_counter()
            p_copied = pv_copied.prove(copied_air, cfg, copied, [])
            t3 = time.perf_counter()
            if rep == 0:
                S.verify_system_proof(system, [cfg, cfg], proof)
                S.verify_stark_proof(big_air, cfg, p_big)
                S.verify_stark_proof(small_air, cfg, p_small)
                S.verify_stark_proof(copied_air, cfg, p_copied)
                continue
            for k, v in (("system", t1 - t0), ("standalone", t2 - t1), ("copied", t3 - t2)):
                ms[k].append(v * 1e3)
            for k, v in (("system_big", sp.last_timings(0)), ("system_small", sp.last_timings(1)), ("standalone_big", pv_big.last_timings()),
                         ("standalone_small", pv_small.last_timings()), ("copied", pv_copied.last_timings())):
                phases[k].append(v)
        out = {"rows": n, "table_rows": SMALL_ROWS, "columns": WIDTH, "table_columns": SMALL_WIDTH, "reps": REPS, "proofs_verified": True,
               "ms_median": {k: round(median(v), 3) for k, v in ms.items()}, "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
               "phase_ms_median": {k: {p: round(median([x[p] for x in v]), 3) for p in v[0]} for k, v in phases.items()}}
        m = out["ms_median"]
        out["price_system_minus_standalone_ms"] = round(m["system"] - m["standalone"], 3)
        out["gain_copied_minus_system_ms"] = round(m["copied"] - m["system"], 3)
        runs.append(out)
    for p in (sp, pv_big, pv_small, pv_copied):
        p.close()
    doc = {"what": "milliseconds from host traces (row-major) to the proof in host memory, wall time from Python; one warm-up per case, then the cases "
                   "alternating; phases from starkhip_last_timings per context (in a system the CTL polynomials and the auxiliary commitment are timed "
                   "with the quotient phase; what a table's stream idles after its trace commitment while the other table's first half runs "
                   "is counted in its trace_merkle)", "runs": runs}
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
