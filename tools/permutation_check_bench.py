"""Times starkhip_check_trace_permutations (Prover.check_trace_permutations: host rows in, report out) on three inputs:
  * the benchmark AIR of DESIGN.md 13, tests/permutation_ref.make_air(3, 300), at 4096 rows (three pairs);
  * one one-entry pair at 2^20 rows (a 16-bit range check);
  * one three-entry pair at 2^20 rows.
Each on a satisfying trace and on the same trace with one rhs cell changed (so that the masks come back).  One warm-up call, then five:
the call times from Python, their median, and the library's split of the median call into upload, sort passes, classification and
read-back (starkhip_perm_check_timings).  Beside each, the only yardsticks there are on the same input: the C++ replay on the host
(median of three) and starkhip_permutation_zs, until now the tool for the same question (median of five after a warm-up call).
Prints one JSON document and, with an argument, writes it to that file."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import permutation_ref as R  # noqa: E402
import starky_bls12_381_amd as S  # noqa: E402
from starky_bls12_381_amd.air_builder import AirBuilder  # noqa: E402

P = R.P


def timed(f, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, out


def median(ts):
    return sorted(ts)[len(ts) // 2]


def one_pair_air(entries):
    b = AirBuilder(2 * entries, 0, 2)
    b.constraint(b.L(0) - b.L(0))
    b.permutation_pair([(c, entries + c) for c in range(entries)])
    return S.register_air(b.finish(), name="PermCheckBench_%d" % entries)


def one_pair_trace(entries, n_rows, rng):
    lhs = rng.integers(0, 1 << 16, (n_rows, entries), dtype=np.uint64) if entries == 1 else rng.integers(0, P, (n_rows, entries), dtype=np.uint64)
    return np.ascontiguousarray(np.concatenate([lhs, lhs[rng.permutation(n_rows)]], axis=1))


def measure(pv, air, trace, bad_cell):
    degree = S.air_constraint_degree(air)
    ch = [int(x) for x in np.random.default_rng(1).integers(0, P, 4 * max(1, degree - 1), dtype=np.uint64)]
    out = {"rows": int(trace.shape[0]), "columns": int(trace.shape[1]), "pairs": S.air_permutation_pairs(air)}
    for name in ("satisfying", "one_cell_changed"):
        t = trace
        if name == "one_cell_changed":
            t = trace.copy()
            t[bad_cell] = (int(t[bad_cell]) + 1) % P
        pv.check_trace_permutations(air, t)  # warm-up: the buffers are allocated here
        calls, splits = [], []
        for _ in range(5):
            rep = pv.check_trace_permutations(air, t)
            calls.append(pv.last_call_s * 1e3)
            splits.append(pv.last_perm_check_timings())
        mid = calls.index(median(calls))
        replay_ms, want = timed(lambda: S.check_trace_permutations_replay(air, t), 3)
        assert np.array_equal(rep.mask_words, want.mask_words) and np.array_equal(rep.list, want.list) and rep.unmatched == want.unmatched
        pv.permutation_zs(air, t, ch)
        zs_ms, (_, closing) = timed(lambda: pv.permutation_zs(air, t, ch), 5)
        out[name] = {"unmatched": rep.unmatched, "pairs_violated": rep.pairs_violated, "reseeds": rep.reseeds,
                     "call_ms": [round(x, 3) for x in calls], "median_ms": round(median(calls), 3),
                     "split_ms_of_the_median_call": {k: round(v, 4) for k, v in splits[mid].items()},
                     "replay_on_the_host_ms": [round(x, 3) for x in replay_ms], "replay_median_ms": round(median(replay_ms), 3),
                     "permutation_zs_ms": [round(x, 3) for x in zs_ms], "permutation_zs_median_ms": round(median(zs_ms), 3),
                     "closing_products_all_one": bool((closing == 1).all())}
    return out


def main():
    rng = np.random.default_rng(13)
    pv = S.Prover(0)
    doc = {"what": "wall milliseconds of Prover.check_trace_permutations (host rows in, report out, cap 1024): one warm-up call, then "
                   "five; the split is the library's (events on the stream; read_back: host time in the copies of the masks)"}
    air = S.register_air(R.make_air(3, 300), name="PermCheckBench_d3_c300")
    doc["make_air(3, 300) at 4096 rows"] = measure(pv, air, R.make_trace(3, 4096, 5, n_cols=300)[0], (1000, 4))
    n = 1 << 20
    doc["one one-entry pair at 2^20 rows"] = measure(pv, one_pair_air(1), one_pair_trace(1, n, rng), (77777, 1))
    doc["one three-entry pair at 2^20 rows"] = measure(pv, one_pair_air(3), one_pair_trace(3, n, rng), (77777, 4))
    pv.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
