"""Times starkhip_check_trace on a real FinalExp trace (8192 rows x 73 527 columns, 360 800 constraints) -- from host rows, and
from column-major device memory (no upload: the kernel plus a few small copies) -- against oracle_check_trace on the host's CPUs,
and the proof time of one mid-sized random AIR (300 columns, 4096 rows).  Prints one JSON line.

--report: times starkhip_check_trace_report instead, on the same trace in column-major device memory: the plain check (for the ratio),
the report on the clean trace (its first pass alone) and the report with cap = 1024 after every cell of row 4000 was raised by one
(both passes).  Best and median of five after a warm-up call; one JSON line.

--free-cells [OUT_DIR]: times starkhip_check_trace_free_cells (Prover.free_cells_device) on the same trace in column-major device
memory, with and without the read-back of the per-cell bitmap, beside the plain check for the ratio; one warm-up call, best and
median of five, call times from Python.  Then audits one real trace of each built-in AIR and records cells, free cells, wholly and
partly free columns and the indices of the wholly free columns.  Prints the two results as JSON lines and, with OUT_DIR, writes
them to OUT_DIR/free_cells_final_exp.json and OUT_DIR/free_cells_builtin_airs.json.

--free-classes [OUT_DIR]: times starkhip_check_trace_free_cell_classes (Prover.free_cell_classes_device) the same way, without and with
the read-back of the three planes, beside the plain check and the free-cell audit timed in the same session; one warm-up call, best
and median of five.  Then classifies one real trace of each built-in AIR and records the four class totals, the columns holding
silent cells, the wholly unread columns and the constraints that were never open, each list as runs of indices ("3,7-9").  Prints the two results as
JSON lines and, with OUT_DIR, writes them to OUT_DIR/free_cell_classes_final_exp.json and OUT_DIR/free_cell_classes_builtin_airs.json.

--in-prove [OUT_DIR]: the cost of the context option "check_trace" inside a proof.  One FinalExp proof alone, the trace in column-major
device memory, the option off and on alternated, five each after a warm-up proof of each: medians, minima and maxima of the call
time, of the proof's total device time and of its phase [0], which holds the check.  The same with the trace as host rows.  Then the
refusal of the trace with every cell of row 4000 raised by one.  One JSON line and, with OUT_DIR, OUT_DIR/check_in_prove.json.

--prove-off N: N FinalExp proofs from column-major device memory with every option at its default, after one warm-up proof; prints their
call times and total device times as one JSON line.  For alternating two builds on one box: --package-root DIR imports
starky_bls12_381_amd from DIR (another checkout, built) instead of this one."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE_ROOT = sys.argv[sys.argv.index("--package-root") + 1] if "--package-root" in sys.argv[1:-1] else ROOT
sys.path[:0] = [PACKAGE_ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime is loaded first, as in bench.py)

import oracle_lib as O  # noqa: E402
import starky_bls12_381_amd as S  # noqa: E402
from bls_util import fp_arr, native_vectors  # noqa: E402
from random_air import random_air  # noqa: E402


def best(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, sorted(ts)[len(ts) // 2] * 1e3, out


def report_mode():
    torch.cuda.set_device(0)
    out = {}
    pv = S.Prover(0)
    air = S.AIR_FINAL_EXP
    t, pis = S.trace_final_exp(fp_arr(*[int(s) for s in native_vectors()["final_exp_input_aa"]]))
    n = t.shape[0]
    cols = torch.from_numpy(np.ascontiguousarray(t.T).view(np.int64)).to("cuda:0")
    del t
    torch.cuda.synchronize()
    pv.check_trace_device(air, cols.data_ptr(), n, pis, layout=1)  # warm-up: op stream, buffers
    mn, md, r = best(lambda: pv.check_trace_device(air, cols.data_ptr(), n, pis, layout=1), 5)
    out["check_trace_clean_ms"] = {"min": mn, "median": md}
    assert r[0] == 0, r
    pv.check_trace_report_device(air, cols.data_ptr(), n, pis, layout=1)
    mn, md, rep = best(lambda: pv.check_trace_report_device(air, cols.data_ptr(), n, pis, layout=1), 5)
    out["report_clean_ms"] = {"min": mn, "median": md}
    assert rep.violations == 0 and len(rep.list) == 0, rep
    out["report_clean_over_check_trace"] = out["report_clean_ms"]["min"] / out["check_trace_clean_ms"]["min"]
    p_minus_1 = int(np.array([S.P - 1], dtype=np.uint64).view(np.int64)[0])
    row = cols[:, 4000]
    cols[:, 4000] = torch.where(row == p_minus_1, torch.zeros_like(row), row + 1)  # as test_check_trace_on_a_final_exp_trace corrupts it
    torch.cuda.synchronize()
    plain = pv.check_trace_device(air, cols.data_ptr(), n, pis, layout=1)
    pv.check_trace_report_device(air, cols.data_ptr(), n, pis, layout=1, cap=1024)
    mn, md, rep = best(lambda: pv.check_trace_report_device(air, cols.data_ptr(), n, pis, layout=1, cap=1024), 5)
    out["report_row_4000_corrupted_cap_1024_ms"] = {"min": mn, "median": md}
    assert rep.violations == plain[0] > 0 and tuple(int(x) for x in rep.list[0]) == plain[1], (rep, plain)
    out["row_4000_corrupted"] = {"violations": rep.violations, "constraints_violated": rep.constraints_violated, "rows_violated": rep.rows_violated,
                                 "rows": rep.rows.tolist()[:16], "listed": len(rep.list)}
    pv.close()
    print(json.dumps(out))


def builtin_traces():
    """(name, AIR, generator of (row-major trace, public inputs)) for one real trace of each built-in AIR, the ones the tests prove."""
    from bls_util import random_fp12
    from test_ecc_aggregate_cpu import pack, reference_vector
    b = {k: int(s) for k, s in native_vectors()["bls_signature"].items()}
    hm = (fp_arr(b["hm_x1"], b["hm_x2"]), fp_arr(b["hm_y1"], b["hm_y2"]), fp_arr(b["hm_z1"], b["hm_z2"]))
    sig = (fp_arr(b["gx"]), fp_arr(b["gy"]), fp_arr(b["s_x1"], b["s_x2"]), fp_arr(b["s_y1"], b["s_y2"]), fp_arr(b["s_z1"], b["s_z2"]))
    pts, bits, _ = reference_vector()
    return [("FP12Mul", S.AIR_FP12_MUL, lambda: S.trace_fp12_mul(random_fp12(0x5EED7200), random_fp12(0x5EED7201))),
            ("PairingPrecomp", S.AIR_PAIRING_PRECOMP, lambda: S.trace_pairing_precomp(*hm)),
            ("MillerLoop", S.AIR_MILLER_LOOP, lambda: S.trace_miller_loop(*sig)),
            ("ECCAgg", S.AIR_ECC_AGGREGATE, lambda: S.trace_ecc_aggregate(*pack(pts, bits))),
            ("FinalExp", S.AIR_FINAL_EXP, lambda: S.trace_final_exp(fp_arr(*[int(s) for s in native_vectors()["final_exp_input_aa"]])))]


def free_cells_mode(out_dir):
    torch.cuda.set_device(0)
    pv = S.Prover(0)
    timing, audit = {"delta": hex(S.DEFAULT_DELTA), "times": "call times from Python, ms"}, {"delta": hex(S.DEFAULT_DELTA), "airs": {}}
    for name, air, make in builtin_traces():
        t, pis = make()
        n = t.shape[0]
        cols = torch.from_numpy(np.ascontiguousarray(t.T).view(np.int64)).to("cuda:0")
        del t
        torch.cuda.synchronize()
        assert pv.check_trace_device(air, cols.data_ptr(), n, pis, layout=1)[0] == 0  # also the warm-up of the plain check
        fc = pv.free_cells_device(air, cols.data_ptr(), n, pis, layout=1, mask=False)  # warm-up: compiled form, buffers
        first_ms = pv.last_call_s * 1e3
        audit["airs"][name] = {"rows": n, "columns": int(fc.per_column.size), "cells": fc.cells, "free_cells": fc.free, "free_columns": fc.free_columns,
                               "partly_free_columns": fc.partly_free_columns, "first_call_ms": first_ms,
                               "wholly_free_column_indices": np.flatnonzero(fc.per_column == n).tolist()}
        if air == S.AIR_FINAL_EXP:
            mn, md, _ = best(lambda: pv.check_trace_device(air, cols.data_ptr(), n, pis, layout=1), 5)
            timing["check_trace_clean_ms"] = {"min": mn, "median": md}
            mn, md, again = best(lambda: pv.free_cells_device(air, cols.data_ptr(), n, pis, layout=1, mask=False), 5)
            timing["free_cells_no_mask_ms"] = {"min": mn, "median": md}
            assert np.array_equal(again.per_column, fc.per_column)
            pv.free_cells_device(air, cols.data_ptr(), n, pis, layout=1, mask=True)
            mn, md, full = best(lambda: pv.free_cells_device(air, cols.data_ptr(), n, pis, layout=1, mask=True), 5)
            timing["free_cells_with_mask_ms"] = {"min": mn, "median": md}
            ones = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)  # the bitmap's bits per column, without unpacking it
            assert np.array_equal(full.per_column, fc.per_column)
            assert np.array_equal(ones[full.mask_words.view(np.uint8)].reshape(fc.per_column.size, -1).sum(axis=1), fc.per_column)
            timing["mask_bytes"] = int(full.mask_words.nbytes)
            timing["no_mask_over_check_trace"] = timing["free_cells_no_mask_ms"]["min"] / timing["check_trace_clean_ms"]["min"]
            timing["with_mask_over_check_trace"] = timing["free_cells_with_mask_ms"]["min"] / timing["check_trace_clean_ms"]["min"]
            timing["op_evaluations_over_check_trace"] = 17459006 / 1932601  # counted from the program: re-walks against the plain walk
            timing["first_call_ms"] = first_ms
        del cols
    pv.close()
    for fname, obj in (("free_cells_final_exp.json", timing), ("free_cells_builtin_airs.json", audit)):
        print(json.dumps(obj))
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, fname), "w") as f:
                json.dump(obj, f, indent=1)
                f.write("\n")


def index_ranges(idx):
    """Ascending indices as one string of runs, "3,7-9,12": thousands of columns stay one line of the JSON file."""
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size == 0:
        return ""
    cut = np.flatnonzero(np.diff(idx) != 1)
    first, last = idx[np.r_[0, cut + 1]], idx[np.r_[cut, idx.size - 1]]
    return ",".join(str(a) if a == b else f"{a}-{b}" for a, b in zip(first.tolist(), last.tolist()))


def free_classes_mode(out_dir):
    torch.cuda.set_device(0)
    pv = S.Prover(0)
    timing, audit = {"delta": hex(S.DEFAULT_DELTA), "times": "call times from Python, ms"}, {"delta": hex(S.DEFAULT_DELTA), "airs": {}}
    for name, air, make in builtin_traces():
        t, pis = make()
        n = t.shape[0]
        cols = torch.from_numpy(np.ascontiguousarray(t.T).view(np.int64)).to("cuda:0")
        del t
        torch.cuda.synchronize()
        assert pv.check_trace_device(air, cols.data_ptr(), n, pis, layout=1)[0] == 0  # also the warm-up of the plain check
        fc = pv.free_cells_device(air, cols.data_ptr(), n, pis, layout=1, mask=False)  # warm-up of the audit: compiled form, buffers
        cl = pv.free_cell_classes_device(air, cols.data_ptr(), n, pis, layout=1, planes=False)  # warm-up: the planes' buffers
        first_ms = pv.last_call_s * 1e3
        assert cl.n_silent + cl.n_gated + cl.n_unread == fc.free and np.array_equal(cl.per_column.sum(axis=1, dtype=np.uint32), fc.per_column)
        silent_cols = np.flatnonzero(cl.per_column[:, 0])
        audit["airs"][name] = {"rows": n, "columns": int(cl.per_column.shape[0]), "constraints": int(cl.open_rows.size), "cells": cl.cells,
                               "caught": cl.n_caught, "silent": cl.n_silent, "gated": cl.n_gated, "unread": cl.n_unread,
                               "silent_columns": cl.silent_columns, "constraints_never_open": cl.constraints_never_open, "first_call_ms": first_ms,
                               "most_silent_rows_in_a_column": int(cl.per_column[:, 0].max()),
                               "silent_column_indices": index_ranges(silent_cols),
                               "wholly_unread_column_indices": index_ranges(np.flatnonzero(cl.per_column[:, 2] == n)),
                               "never_open_constraint_indices": index_ranges(np.flatnonzero(cl.open_rows == 0))}
        if air == S.AIR_FINAL_EXP:
            mn, md, _ = best(lambda: pv.check_trace_device(air, cols.data_ptr(), n, pis, layout=1), 5)
            timing["check_trace_clean_ms"] = {"min": mn, "median": md}
            mn, md, _ = best(lambda: pv.free_cells_device(air, cols.data_ptr(), n, pis, layout=1, mask=False), 5)
            timing["free_cells_no_mask_ms"] = {"min": mn, "median": md}
            mn, md, again = best(lambda: pv.free_cell_classes_device(air, cols.data_ptr(), n, pis, layout=1, planes=False), 5)
            timing["free_cell_classes_no_planes_ms"] = {"min": mn, "median": md}
            assert np.array_equal(again.per_column, cl.per_column) and np.array_equal(again.open_rows, cl.open_rows)
            pv.free_cell_classes_device(air, cols.data_ptr(), n, pis, layout=1, planes=True)
            mn, md, full = best(lambda: pv.free_cell_classes_device(air, cols.data_ptr(), n, pis, layout=1, planes=True), 5)
            timing["free_cell_classes_with_planes_ms"] = {"min": mn, "median": md}
            assert np.array_equal(full.per_column, cl.per_column)
            timing["plane_bytes"] = int(full.plane_words.nbytes)
            timing["no_planes_over_free_cells"] = timing["free_cell_classes_no_planes_ms"]["min"] / timing["free_cells_no_mask_ms"]["min"]
            timing["no_planes_over_check_trace"] = timing["free_cell_classes_no_planes_ms"]["min"] / timing["check_trace_clean_ms"]["min"]
            timing["first_call_ms"] = first_ms
            del full
        del cols
    pv.close()
    for fname, obj in (("free_cell_classes_final_exp.json", timing), ("free_cell_classes_builtin_airs.json", audit)):
        print(json.dumps(obj))
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, fname), "w") as f:
                json.dump(obj, f, indent=1)
                f.write("\n")


def spread(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def final_exp_on_device():
    t, pis = S.trace_final_exp(fp_arr(*[int(s) for s in native_vectors()["final_exp_input_aa"]]))
    cols = torch.from_numpy(np.ascontiguousarray(t.T).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return t, pis, cols


def in_prove_mode(out_dir):
    torch.cuda.set_device(0)
    pv = S.Prover(0)
    air = S.AIR_FINAL_EXP
    cfg = S.StarkConfig.for_air(air)
    t, pis, cols = final_exp_on_device()
    n = t.shape[0]
    out = {"times": "ms; call = wall time of the C call, total and phase0 = starkhip_last_timings [10] and [0]", "proofs_each": 5}

    def alternate(prove):
        runs = {0: {"call": [], "total": [], "phase0": []}, 1: {"call": [], "total": [], "phase0": []}}
        for on in (0, 1):  # warm-up: buffers, plan, the check program
            pv.set_option("check_trace", on)
            prove()
        for _ in range(5):
            for on in (0, 1):
                pv.set_option("check_trace", on)
                prove()
                runs[on]["call"].append(pv.last_call_s * 1e3)
                ms = pv.last_timings()
                runs[on]["total"].append(ms["total"])
                runs[on]["phase0"].append(ms["upload"])
        res = {("on" if on else "off"): {k: spread(v) for k, v in r.items()} for on, r in runs.items()}
        res["on_minus_off_median_ms"] = {k: res["on"][k]["median"] - res["off"][k]["median"] for k in ("call", "total", "phase0")}
        return res

    out["device_colmajor"] = alternate(lambda: pv.prove_device(air, cfg, cols.data_ptr(), n, pis, layout=1, keep=False))
    out["host_rows"] = alternate(lambda: pv.prove(air, cfg, t, pis))
    stats = pv.check_stats()
    assert stats == {"checked": 12, "rejected": 0}, stats
    p_minus_1 = int(np.array([S.P - 1], dtype=np.uint64).view(np.int64)[0])
    row = cols[:, 4000]
    cols[:, 4000] = torch.where(row == p_minus_1, torch.zeros_like(row), row + 1)
    torch.cuda.synchronize()
    pv.set_option("check_trace", 1)
    ts, rep = [], None
    for _ in range(3):
        t0 = time.perf_counter()
        try:
            pv.prove_device(air, cfg, cols.data_ptr(), n, pis, layout=1, keep=False)
            raise SystemExit("the corrupted trace was proven")
        except S.TraceViolation as e:
            rep = e.report
        ts.append((time.perf_counter() - t0) * 1e3)
    out["refusal_row_4000_corrupted_call_ms"] = spread(ts)
    out["refusal_row_4000_corrupted"] = {"violations": rep.violations, "constraints_violated": rep.constraints_violated,
                                         "rows_violated": rep.rows_violated, "listed": len(rep.list)}
    pv.close()
    print(json.dumps(out))
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "check_in_prove.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def prove_off_mode(reps):
    torch.cuda.set_device(0)
    pv = S.Prover(0)
    air = S.AIR_FINAL_EXP
    cfg = S.StarkConfig.for_air(air)
    t, pis, cols = final_exp_on_device()
    n = t.shape[0]
    del t
    pv.prove_device(air, cfg, cols.data_ptr(), n, pis, layout=1, keep=False)
    call, total = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        pv.prove_device(air, cfg, cols.data_ptr(), n, pis, layout=1, keep=False)
        call.append((time.perf_counter() - t0) * 1e3)  # (the wall time of the Python call: the parent's binding keeps no call time here)
        total.append(pv.last_timings()["total"])
    pv.close()
    print(json.dumps({"library": S.LIB_PATH, "call_ms": call, "total_ms": total}))


def main():
    if "--in-prove" in sys.argv[1:]:
        rest = sys.argv[sys.argv.index("--in-prove") + 1:]
        return in_prove_mode(rest[0] if rest else None)
    if "--prove-off" in sys.argv[1:]:
        return prove_off_mode(int(sys.argv[sys.argv.index("--prove-off") + 1]))
    if "--report" in sys.argv[1:]:
        return report_mode()
    if "--free-classes" in sys.argv[1:]:
        rest = sys.argv[sys.argv.index("--free-classes") + 1:]
        return free_classes_mode(rest[0] if rest else None)
    if "--free-cells" in sys.argv[1:]:
        rest = sys.argv[sys.argv.index("--free-cells") + 1:]
        return free_cells_mode(rest[0] if rest else None)
    torch.cuda.set_device(0)
    out = {}
    pv = S.Prover(0)
    air = S.AIR_FINAL_EXP
    t, pis = S.trace_final_exp(fp_arr(*[int(s) for s in native_vectors()["final_exp_input_aa"]]))
    pv.check_trace(air, t, pis)  # warm-up: op stream, buffers
    mn, md, r = best(lambda: pv.check_trace(air, t, pis), 5)
    out["final_exp_host_rows_ms"] = {"min": mn, "median": md}
    assert r[0] == 0, r
    cols = torch.from_numpy(np.ascontiguousarray(t.T).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    mn, md, r = best(lambda: pv.check_trace_device(air, cols.data_ptr(), t.shape[0], pis, layout=1), 5)
    out["final_exp_device_colmajor_ms"] = {"min": mn, "median": md}
    assert r[0] == 0, r
    del cols
    threads = int(os.environ.get("OMP_NUM_THREADS", "16") or 16)
    O.lib.oracle_set_threads.argtypes = [C.c_int]
    O.lib.oracle_set_threads(threads)
    t0 = time.perf_counter()
    bad, _ = O.check_trace(S.air_program(air), t, pis)
    out["final_exp_oracle_ms"] = (time.perf_counter() - t0) * 1e3
    out["oracle_threads"] = threads
    assert bad == 0
    del t
    blob, trace, rpis = random_air(8, 300, 5, 4096)
    rair = S.register_air(blob)
    cfg = S.StarkConfig.for_air(rair)
    pv.prove(rair, cfg, trace, rpis)
    mn, md, _ = best(lambda: pv.prove(rair, cfg, trace, rpis), 5)
    out["random_air_300x4096_deg5_prove_ms"] = {"min": mn, "median": md, "constraints": int(blob[4])}
    pv.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
