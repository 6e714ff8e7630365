"""A proof pool's verifier (csrc/verify_service.cpp) on the CPU: tests/tsan_verify_pool_main.cpp under ThreadSanitizer against the
stand-in device of csrc/host_only_stubs.cc, whose verify launches run their routine on the host.  The proofs are the oracle's, of the
toy AIR, valid, tampered and malformed; every verdict must equal starkhip_verify's code.  And the split of a verify batch over the
pools of a multi-device handle (starkhip_plan_verify)."""
import ctypes as C
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AIR = S.AIR_TEST_FIBONACCI


def _proof(n, rate_bits):
    cfg = S.StarkConfig.standard_fast_config()
    cfg.rate_bits = rate_bits
    t, pis = S.trace_fibonacci(3, 5, n)
    return cfg, O.prove(S.air_program(AIR), cfg, S.trace_rows_to_poly_values(t), pis)


def _cases():
    out = [(AIR,) + _proof(n, rb) for n, rb in ((16, 1), (64, 2), (1024, 1))]
    cfg, proof = _proof(64, 1)
    L = S.proof_layout(proof)
    q0, qw = int(L.off_query_rounds), int(L.query_round_words)
    for pos in (int(L.off_trace_cap) + 1, q0 + 2, q0 + qw + 9, int(L.off_final_poly), int(L.off_pow_witness), proof.size - 1):
        bad = proof.copy()
        bad[pos] = (int(bad[pos]) + 1) % S.P
        out.append((AIR, cfg, bad))
    bad = proof.copy()
    bad[q0 + 5] = S.P + 1  # a word >= p in the query rounds
    out.append((AIR, cfg, bad))
    out.append((AIR, cfg, proof[:-1]))  # truncated
    out.append((AIR, cfg, proof[:10]))
    out.append((S.AIR_FP12_MUL, S.StarkConfig.for_air(S.AIR_FP12_MUL), proof))  # the wrong AIR
    out.append((AIR, cfg, proof))
    return out


def _write(path, cases):
    with open(path, "wb") as f:
        for air, cfg, proof in cases:
            p = np.ascontiguousarray(proof, dtype=np.uint64)
            cb = bytes(cfg)
            f.write(np.array([air, len(cb)], dtype=np.int32).tobytes())
            f.write(cb)
            f.write(np.array([p.size], dtype=np.uint64).tobytes())
            f.write(p.tobytes())


@pytest.mark.slow
def test_pool_verifier_is_race_free_and_exact_under_thread_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    cases = _cases()
    codes = []
    for air, cfg, proof in cases:
        try:
            S.verify_stark_proof(air, cfg, proof)
            codes.append(0)
        except S.StarkhipError as e:
            codes.append(e.code)
    assert 0 in codes and S.ERR_VERIFY in codes and S.ERR_BAD_SHAPE in codes
    data = str(tmp_path / "cases.bin")
    _write(data, cases)
    exe = str(tmp_path / "tsan_verify_pool")
    srcs = sorted(glob.glob(os.path.join(ROOT, "starky_bls12_381_amd", "csrc", "*.cpp"))) + [os.path.join(ROOT, "starky_bls12_381_amd", "csrc", "host_only_stubs.cc")]
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "tsan_verify_pool_main.cpp")] + srcs + ["-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if b.returncode != 0 and "tsan" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("libtsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1", STARKHIP_FAKE_DEVICE="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "ThreadSanitizer" not in r.stderr
    assert "pool: ok" in r.stdout and "multipool: ok" in r.stdout


def _plan(airs, n_pools):
    n = len(airs)
    a = (C.c_int * max(n, 1))(*airs)
    slots = (C.c_int * max(n, 1))()
    order = (C.c_size_t * max(n, 1))()
    assert S.lib.starkhip_plan_verify(n, a, n_pools, slots, order) == 0
    return list(slots[:n]), list(order[:n])


def test_verify_batch_split_places_every_proof_once_longest_first():
    S.lib.starkhip_air_verify_cost.restype = C.c_double
    cost = lambda air: S.lib.starkhip_air_verify_cost(air)
    # one signature's six proofs, eight times over, in the order a caller collects them
    sig = [S.AIR_PAIRING_PRECOMP, S.AIR_MILLER_LOOP, S.AIR_PAIRING_PRECOMP, S.AIR_MILLER_LOOP, S.AIR_FP12_MUL, S.AIR_FINAL_EXP]
    airs = sig * 8
    for n_pools in (1, 2, 3, 8):
        slots, order = _plan(airs, n_pools)
        assert sorted(order) == list(range(len(airs)))  # every proof placed exactly once
        assert all(0 <= s < n_pools for s in slots)
        costs = [cost(airs[i]) for i in order]
        assert costs == sorted(costs, reverse=True)  # longest first
        for a, b in zip(order, order[1:]):  # ties in the caller's order
            if cost(airs[a]) == cost(airs[b]):
                assert a < b
        loads = [sum(cost(airs[i]) for i in range(len(airs)) if slots[i] == s) for s in range(n_pools)]
        assert max(loads) - min(loads) <= max(cost(a) for a in airs)  # LPT: within one job of each other
        if n_pools > 1:
            assert len(set(slots)) == n_pools
    # the costs come from the measured split: MillerLoop > FinalExp > FP12Mul > PairingPrecomp
    assert cost(S.AIR_MILLER_LOOP) > cost(S.AIR_FINAL_EXP) > cost(S.AIR_FP12_MUL) > cost(S.AIR_PAIRING_PRECOMP) > 0
    assert _plan([], 2) == ([], [])
