"""The scheduling rules of the proof pool that need no thread and no device: which queued recording a generator thread takes and which
queued job a context takes (csrc/pool_jobs.cpp, through tests/pool_pickers_main.cpp linked against the library), and the one
longest-first planner behind starkhip_plan_lpt and starkhip_plan_verify (csrc/multipool.cpp) against the rule written out here."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import starky_bls12_381_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AIRS = [S.AIR_FINAL_EXP, S.AIR_MILLER_LOOP, S.AIR_PAIRING_PRECOMP, S.AIR_FP12_MUL, S.AIR_ECC_AGGREGATE, S.AIR_TEST_FIBONACCI]


def test_pickers_keep_what_their_comments_promise(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    lib = os.path.abspath(S.api.LIB_PATH)
    exe = str(tmp_path / "pool_pickers")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "pool_pickers_main.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pickers: ok" in r.stdout


def _longest_first(airs, cost, n_pools):
    """The rule: by decreasing cost, ties in the caller's order; each to the pool with the least cost so far, ties to the lowest slot."""
    order = sorted(range(len(airs)), key=lambda i: -cost(airs[i]))  # sorted() is stable
    load, slots = [0.0] * n_pools, [0] * len(airs)
    for i in order:
        s = min(range(n_pools), key=lambda k: (load[k], k))
        slots[i] = s
        load[s] += cost(airs[i])
    return slots, order


def test_both_planners_are_the_one_longest_first_rule_ties_included():
    S.lib.starkhip_air_cost.restype = C.c_double
    S.lib.starkhip_air_verify_cost.restype = C.c_double
    cost, vcost = (lambda a: S.lib.starkhip_air_cost(a)), (lambda a: S.lib.starkhip_air_verify_cost(a))
    assert vcost(S.AIR_FINAL_EXP) == vcost(S.AIR_ECC_AGGREGATE)  # two AIRs of one cost: ties between different AIRs, not only repeats
    rng = random.Random(7)
    for case in range(300):
        n = rng.randrange(0, 40)
        n_pools = rng.randrange(1, 9)
        airs = [rng.choice(AIRS) for _ in range(n)]
        a = (C.c_int * max(n, 1))(*airs)
        slots = (C.c_int * max(n, 1))()
        order = (C.c_size_t * max(n, 1))()
        assert S.lib.starkhip_plan_lpt(n, a, n_pools, slots) == 0
        assert list(slots[:n]) == _longest_first(airs, cost, n_pools)[0]
        assert S.lib.starkhip_plan_verify(n, a, n_pools, slots, order) == 0
        want_slots, want_order = _longest_first(airs, vcost, n_pools)
        assert list(slots[:n]) == want_slots and list(order[:n]) == want_order
        assert S.lib.starkhip_plan_verify(n, a, n_pools, slots, None) == 0  # the order is optional
        assert list(slots[:n]) == want_slots
