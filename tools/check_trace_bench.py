"""Times starkhip_check_trace on a real FinalExp trace (8192 rows x 73 527 columns, 360 800 constraints) -- from host rows, and
from column-major device memory (no upload: the kernel plus a few small copies) -- against oracle_check_trace on the host's CPUs,
and the proof time of one mid-sized random AIR (300 columns, 4096 rows).  Prints one JSON line.

--report: times starkhip_check_trace_report instead, on the same trace in column-major device memory: the plain check (for the ratio),
the report on the clean trace (its first pass alone) and the report with cap = 1024 after every cell of row 4000 was raised by one
(both passes).  Best and median of five after a warm-up call; one JSON line."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

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


def main():
    if "--report" in sys.argv[1:]:
        return report_mode()
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
