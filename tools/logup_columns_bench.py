"""Measurements for LogUp lookups over Columns and Filters, with the method of tools/logup_bench.py: one warm-up, the cases alternating
inside a round, medians and all samples; wall time from Python around each call, phases from starkhip_last_timings.

  python tools/logup_columns_bench.py ab OTHER_LIBRARY [ROUNDS]
      1. no regression for plain lookups: logup_bench's logup_d3 at 2^12 and 2^16 rows (prove, starkhip_logup_polys) and the
         2^20 x 16-limb fill of logup_freq_bench (starkhip_logup_frequencies), in child processes that alternate between this build and
         OTHER_LIBRARY (the parent commit's, from `make variant`); the bar is the other library's own spread over its rounds.
         Raw lines -> profiles/logup_columns_bench_ab.jsonl.
  python tools/logup_columns_bench.py general
      2. the price of generality: the same plain program with STARKHIP_LOGUP_GENERAL=1 forcing the general kernels, alternating.
  python tools/logup_columns_bench.py buys
      3. what it buys: sixteen limbs range-checked only where a selector is on, at degree 3 -- with filters (19 columns) and with
         sixteen materialised columns sel * limb and their constraints (35 columns) -- at 2^16 and 2^20 rows.
  python tools/logup_columns_bench.py all OTHER_LIBRARY      all three -> profiles/logup_columns.json
  (child OUT: one process of `ab`, used by it.)"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

REPS = 5
P = 0xFFFFFFFF00000001


def median(ts):
    return sorted(ts)[len(ts) // 2]


def timed(call):
    t0 = time.perf_counter()
    r = call()
    return (time.perf_counter() - t0) * 1e3, r


def limb_trace(n, n_cols, limbs, table, freq, rng):
    """n rows of small random cells; `limbs` hold values of the table column (0 .. min(n, 2^16) - 1, every value on its first row
    counted in `freq` by numpy)"""
    t = rng.integers(1, 1 << 31, (n, n_cols), dtype=np.uint64)
    t[:, 0] = np.arange(5, 5 + n, dtype=np.uint64)
    t[:, 1] = t[:, 0] * t[:, 0]
    t[:, table] = np.arange(n, dtype=np.uint64) % np.uint64(1 << 16)
    t[:, limbs] = rng.integers(0, min(n, 1 << 16), (n, len(limbs))).astype(np.uint64)
    t[:, freq] = 0
    return t


def count_into(t, cells, freq):
    """the multiplicities of `cells` (values of the table 0 .. 2^16 - 1, whose first rows are rows 0 .. 2^16 - 1) into column freq"""
    t[:, freq] = np.bincount(cells.astype(np.int64).reshape(-1), minlength=t.shape[0]).astype(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. plain lookups, this build against another
def child(out_path):
    import logup_bench as LB
    import starky_bls12_381_amd as S
    rng = np.random.default_rng(29)
    air = LB.make_air("logup", 3)
    pv = S.Prover(0)
    lines = []
    for n in (1 << 12, 1 << 16):
        trace, _ = LB.make_trace(n, rng)
        cfg = S.StarkConfig.for_air(air)
        prove_ms, polys_ms, quotient_ms = [], [], []
        for rep in range(REPS + 1):
            a, _ = timed(lambda: pv.prove(air, cfg, trace, []))
            q = pv.last_timings()["quotient"]
            b, _ = timed(lambda: pv.logup_polys(air, trace, [3, 5]))
            if rep:
                prove_ms.append(a), polys_ms.append(b), quotient_ms.append(q)
        lines.append({"case": "logup_d3", "rows": n, "prove_ms": prove_ms, "quotient_phase_ms": quotient_ms, "logup_polys_ms": polys_ms})
    from starky_bls12_381_amd.air_builder import AirBuilder
    n, limbs = 1 << 20, list(range(2, 18))
    b = AirBuilder(20, 0, 3)
    b.constraint(b.L(1) - b.L(0) * b.L(0))
    b.logup(limbs, 18, 19)
    fair = S.register_air(b.finish(), name="LogupColumnsBench_fill")
    trace = np.ascontiguousarray(limb_trace(n, 20, limbs, 18, 19, rng).T)
    fill_ms = []
    for rep in range(REPS + 1):
        ms, rep_ = timed(lambda: pv.logup_frequencies(fair, trace, layout=1))
        assert rep_.failed == 0
        if rep:
            fill_ms.append(ms)
    lines.append({"case": "fill_16_limbs", "rows": n, "logup_frequencies_ms": fill_ms})
    pv.close()
    with open(out_path, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


def ab(other, rounds=3):
    raw, tmp = [], os.path.join(tempfile.mkdtemp(), "child.jsonl")
    for rnd in range(rounds):
        for build, lib in (("this", None), ("parent", other)):
            env = dict(os.environ)
            env.pop("STARKHIP_LIBRARY", None)
            if lib:
                env["STARKHIP_LIBRARY"] = os.path.abspath(lib)
            subprocess.run([sys.executable, os.path.abspath(__file__), "child", tmp], check=True, env=env, timeout=280)
            with open(tmp) as f:
                raw += [dict(json.loads(ln), build=build, round=rnd) for ln in f]
    with open(os.path.join(ROOT, "profiles", "logup_columns_bench_ab.jsonl"), "w") as f:
        for ln in raw:
            f.write(json.dumps(ln) + "\n")
    out = []
    for case, n in sorted({(ln["case"], ln["rows"]) for ln in raw}):
        for metric in ("prove_ms", "logup_polys_ms", "logup_frequencies_ms"):
            per = {bld: [round(median(ln[metric]), 3) for ln in raw if (ln["case"], ln["rows"], ln["build"]) == (case, n, bld) and metric in ln] for bld in ("this", "parent")}
            if per["this"]:
                lo, hi = min(per["parent"]), max(per["parent"])
                out.append({"case": case, "rows": n, "metric": metric, "round_medians": per, "this_median": median(per["this"]), "parent_spread": [lo, hi],
                            "inside_parent_spread": lo <= median(per["this"]) <= hi, "below_parent_worst": median(per["this"]) <= hi})
    return out


# ------------------------------------------------------------------------------------------------ 2. the general kernels on a plain program
def general():
    import logup_bench as LB
    import starky_bls12_381_amd as S
    rng = np.random.default_rng(29)
    air = LB.make_air("logup", 3)
    pv = S.Prover(0)
    out = []
    for n in (1 << 12, 1 << 16):
        trace, _ = LB.make_trace(n, rng)
        cfg = S.StarkConfig.for_air(air)
        ms = {k: {"prove_ms": [], "quotient_phase_ms": [], "logup_polys_ms": []} for k in ("plain", "general")}
        proofs = {}
        for rep in range(REPS + 1):
            for kind in ("plain", "general"):
                os.environ["STARKHIP_LOGUP_GENERAL"] = "1" if kind == "general" else "0"
                a, proofs[kind] = timed(lambda: pv.prove(air, cfg, trace, []))
                q = pv.last_timings()["quotient"]
                b, _ = timed(lambda: pv.logup_polys(air, trace, [3, 5]))
                if rep:
                    ms[kind]["prove_ms"].append(a), ms[kind]["quotient_phase_ms"].append(q), ms[kind]["logup_polys_ms"].append(b)
        del os.environ["STARKHIP_LOGUP_GENERAL"]
        assert proofs["plain"].tobytes() == proofs["general"].tobytes()
        out.append({"rows": n, "same_proof_bytes": True, "median": {k: {m: round(median(v), 3) for m, v in d.items()} for k, d in ms.items()},
                    "ms": {k: {m: [round(x, 3) for x in v] for m, v in d.items()} for k, d in ms.items()}})
    pv.close()
    return out


# ------------------------------------------------------------------------------------------------ 3. filters against materialised columns
def buys():
    import starky_bls12_381_amd as S
    from starky_bls12_381_amd.air_builder import AirBuilder, Filter
    LIMBS, SEL, TABLE, FREQ, MAT = list(range(2, 18)), 18, 19, 20, list(range(21, 37))  # columns 0, 1: the AIR's own

    def make(kind):
        b = AirBuilder(21 if kind == "filters" else 37, 0, 3)
        b.constraint(b.L(1) - b.L(0) * b.L(0))
        b.transition(b.N(0) - b.L(0) - 1)
        b.constraint(b.L(SEL) * (1 - b.L(SEL)))
        if kind == "filters":
            b.logup_columns([(c, Filter(sums=[SEL])) for c in LIMBS], TABLE, FREQ)
        else:
            for c, m in zip(LIMBS, MAT):
                b.constraint(b.L(m) - b.L(SEL) * b.L(c))
            b.logup(MAT, TABLE, FREQ)
        return S.register_air(b.finish(), name="LogupColumnsBench_" + kind)
    airs = {k: make(k) for k in ("filters", "materialised")}
    rng = np.random.default_rng(31)
    pv = S.Prover(0)
    out = []
    for n in (1 << 16, 1 << 20):
        wide = limb_trace(n, 37, LIMBS, TABLE, FREQ, rng)
        wide[:, SEL] = rng.integers(0, 2, n).astype(np.uint64)
        wide[:, MAT] = wide[:, LIMBS] * wide[:, SEL:SEL + 1]
        traces = {"materialised": wide, "filters": np.ascontiguousarray(wide[:, :21])}
        on = wide[:, SEL] == 1
        count_into(traces["filters"], wide[on][:, LIMBS], FREQ)
        count_into(traces["materialised"], wide[:, MAT], FREQ)
        ms, phases = {k: [] for k in airs}, {k: [] for k in airs}
        for rep in range(REPS + 1):
            for kind, air in airs.items():
                cfg = S.StarkConfig.for_air(air)
                wall, proof = timed(lambda: pv.prove(air, cfg, traces[kind], []))
                if rep == 0:
                    S.verify_stark_proof(air, cfg, proof)
                else:
                    ms[kind].append(wall), phases[kind].append(pv.last_timings())
        out.append({"rows": n, "limbs": 16, "committed_columns": {"filters": 19 + 2, "materialised": 35 + 2}, "proofs_verified": True,
                    "ms_median": {k: round(median(v), 3) for k, v in ms.items()}, "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                    "phase_ms_median": {k: {p: round(median([x[p] for x in v]), 3) for p in v[0]} for k, v in phases.items()}})
    pv.close()
    return out


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "child":
        return child(sys.argv[2])
    doc = {"what": "milliseconds, wall time from Python around each call (host trace in, result in host memory); one warm-up, then REPS = %d with the "
                   "cases alternating; phases from starkhip_last_timings (the LogUp work is timed with the quotient phase)" % REPS}
    if mode in ("ab", "all"):
        doc["plain_lookups_this_build_against_the_parent"] = ab(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    if mode in ("general", "all"):
        doc["general_kernels_forced_on_a_plain_program"] = general()
    if mode in ("buys", "all"):
        doc["filters_against_materialised_columns"] = buys()
    text = json.dumps(doc, indent=1)
    print(text)
    if mode == "all":
        with open(os.path.join(ROOT, "profiles", "logup_columns.json"), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
