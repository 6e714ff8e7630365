"""Trace cells at or above p on the device: every entry that reads a trace reads a 64-bit word w as the field element w mod p
(include/starkhip.h).  The trace checkers, the trace LDE in each of its kernels and whole proofs, given a trace with p added to some of
its small cells (alias_util: only cells <= 2^32 - 2 have a second representative, and random traces hold none), return what they
return for the canonical trace, which is what the host replays and the CPU oracle say of the canonical trace.  Bit for bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from alias_util import (ALL_SMALL_FLOOR, DIRECTED_VALUE, EDGES, HAND_FLOOR, P, SMALL_MAX, alias, assert_aliased, directed_blob, directed_traces,
                        hand_blob, hand_trace, hand_violating)
from bls_util import random_fp12
from check_report_util import Expected, assert_report
from config_cases import small_cell_air
from free_cells_util import assert_same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 1 << 20
NO_PIS = np.zeros(0, dtype=np.uint64)


def same_report(a, b):
    assert (a.violations, a.constraints_violated, a.rows_violated) == (b.violations, b.constraints_violated, b.rows_violated)
    for f in ("per_constraint", "row_mask", "rows", "list"):
        assert getattr(a, f).dtype == getattr(b, f).dtype and np.array_equal(getattr(a, f), getattr(b, f)), f


# ---------------------------------------------------------------- the trace checkers
def checkers_agree(prover, air, blob, clean, aliased, pis, want=None):
    """check_trace, check_trace_report (cap 0, 7, full) and free_cells on `aliased`: what they say of `clean`, what the host replays
    say of `clean`, and the oracle's expectation for it; both layouts; the caller's buffer left as it was."""
    want = want or Expected(blob, clean, pis)  # asserts the oracle's own count of the canonical trace
    first = tuple(int(x) for x in want.list[0]) if want.violations else (0, 0, 0)
    free = S.free_cells_replay(air, clean, pis)
    for layout, c, a in ((0, clean, aliased), (1, clean.T.copy(), aliased.T.copy())):
        kept = a.copy()
        assert prover.check_trace(air, a, pis, layout=layout) == (want.violations, first)
        assert prover.check_trace(air, c, pis, layout=layout) == (want.violations, first)
        for cap in (0, 7, FULL):
            got = prover.check_trace_report(air, a, pis, layout=layout, cap=cap)
            same_report(got, prover.check_trace_report(air, c, pis, layout=layout, cap=cap))
            if cap == FULL:  # (the shorter lists are cut from the same expectation below)
                same_report(got, S.check_trace_report_replay(air, c, pis, layout=layout, cap=cap))
            assert_report(got, want, cap)
        fc = prover.free_cells(air, a, pis, layout=layout)
        assert_same(fc, prover.free_cells(air, c, pis, layout=layout))
        assert_same(fc, free)
        assert np.array_equal(a, kept)
    return want


@functools.lru_cache(maxsize=None)
def hand_air():
    return S.register_air(hand_blob(), name="alias_hand")


# 8 rows: 56 idle lanes; 64: one wave; 256: several waves per constraint
@pytest.mark.parametrize("n", (8, 64, 256))
@pytest.mark.parametrize("violating", (False, True), ids=("satisfying", "violating"))
def test_checkers_on_the_hand_written_air(prover, n, violating):
    trace, pis = hand_violating(n) if violating else hand_trace(n)
    want = Expected(hand_blob(), trace, pis)
    assert (want.constraints_violated >= 12 and want.not_applicable > 0) if violating else want.violations == 0
    for share, seed in ((1.0, 1), (0.6, 2)):  # everything that can be, and a mix of the two representatives inside one constraint
        aliased, count = alias(trace, share, seed)
        assert_aliased(aliased, trace, HAND_FLOOR, share, count)
        checkers_agree(prover, hand_air(), hand_blob(), trace, aliased, pis, want)


@pytest.mark.parametrize("n", (8, 256))
def test_checkers_on_the_directed_rows(prover, n):
    """L1 - L0 + L2 on L0 = p + 5, L1 = 3, L2 = p - 2^32 + 3: subtracting the raw word p + 5 gives 2^64 - 2, and the sum with L2 is then
    exactly p -- a violated constraint read as satisfied, on every row, in either order of its terms"""
    air = S.register_air(directed_blob(), name="alias_directed")
    aliased, clean = directed_traces(n)
    assert_aliased(aliased, clean, HAND_FLOOR)
    want = checkers_agree(prover, air, directed_blob(), clean, aliased, NO_PIS)
    assert want.violations == 2 * n and all(int(v) == DIRECTED_VALUE for v in want.list[:, 2])


def test_checkers_on_a_real_fp12_mul_trace(prover):
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED7200), random_fp12(0x5EED7201))
    blob = S.air_program(S.AIR_FP12_MUL)
    for c in (0, 5, t.shape[1] // 7, t.shape[1] // 2):  # not every cell is constrained on every row: the first of these that is
        bad = t.copy()
        bad[9, c] += np.uint64(3)
        want = Expected(blob, bad, pis)
        if want.violations > 0:
            break
    assert want.violations > 0
    for trace, w in ((t, None), (bad, want)):
        aliased, count = alias(trace, 0.5, 50)
        assert_aliased(aliased, trace, ALL_SMALL_FLOOR, 0.5, count)
        got = checkers_agree(prover, S.AIR_FP12_MUL, blob, trace, aliased, pis, w)
        assert (got.violations == 0) == (w is None)


# ---------------------------------------------------------------- the trace LDE, one case per kernel
def lde_columns(log_n, n_cols, seed):
    """(aliased, canonical) column-major [n_cols][2^log_n]: the columns the closed-form classes of kernels_lde.hip could take for what
    they are not, in either representative, edge values, small random cells half of them aliased, and one column of large cells."""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    edges = np.array(EDGES, dtype=np.uint64)[i % len(EDGES)]

    def unit(zero, one):
        col = np.full(n, zero, dtype=np.uint64)
        col[n // 2 + 1 if n > 2 else 1] = one
        return col

    mixed = np.full(n, 1, dtype=np.uint64)
    mixed[1::2] = P + 1
    cols = [np.full(n, P, dtype=np.uint64),                                    # all p: the constant 0
            np.full(n, 7 + P, dtype=np.uint64),                                # the constant 7 as 7 + p
            edges + np.uint64(P) * ((i + i // len(EDGES)) % 2).astype(np.uint64),  # every edge value in both representatives
            unit(P, 1),                                                        # a unit vector whose zeros are p
            mixed,                                                             # the constant 1 as 1 and p + 1
            edges + np.uint64(P),                                              # every edge value aliased
            np.full(n, 7, dtype=np.uint64),                                    # the constant 7
            unit(0, P + 1)]                                                    # a unit vector whose one is p + 1
    cols = cols[:n_cols]
    while len(cols) < n_cols - (1 if n_cols >= 10 else 0):
        cols.append(alias(rng.integers(0, SMALL_MAX + 1, size=n, dtype=np.uint64), 0.5, int(rng.integers(1 << 30)))[0])
    if len(cols) < n_cols:
        cols.append(rng.integers(0, P, size=n, dtype=np.uint64))
    aliased = np.stack(cols)
    return aliased, aliased % np.uint64(P)


# log_n 1, 4, 7: lde_columns_kernel; 8, 12: lde_columns_v2_kernel, 12 with its closed forms; 13: the wave kernel and, with
# lde_impl = 1 and for the coefficients, v2; 14: the long kernels
@pytest.mark.parametrize("log_n,rate_bits,n_cols", [(1, 1, 5), (4, 2, 7), (7, 1, 17), (8, 2, 9), (12, 1, 13), (12, 2, 9), (13, 1, 9), (13, 2, 11),
                                                    (14, 1, 5), (14, 2, 9)])
def test_lde_of_aliased_columns_is_the_oracles_of_the_canonical_ones(prover, log_n, rate_bits, n_cols):
    aliased, clean = lde_columns(log_n, n_cols, 100 * log_n + rate_bits)
    assert_aliased(aliased, clean, ALL_SMALL_FLOOR)
    assert n_cols < 8 or sum(len(set(col.tolist())) <= 2 for col in aliased[:8]) == 6  # the six columns a closed form is near to
    kept = aliased.copy()
    ocoeffs, olde_rows = O.lde_rows(clean, rate_bits)
    for impl in ((0, 1) if log_n == 13 else (0,)):
        for closed in (1, 0):
            prover.set_option("lde_impl", impl)
            prover.set_option("lde_closed_forms", closed)
            try:
                coeffs, lde = prover.lde_batch(aliased, rate_bits)
            finally:
                prover.set_option("lde_impl", 0)
                prover.set_option("lde_closed_forms", 1)
            assert np.array_equal(lde, olde_rows.T), (impl, closed, np.flatnonzero((lde != olde_rows.T).any(axis=1)))
            assert np.array_equal(coeffs, ocoeffs), (impl, closed, np.flatnonzero((coeffs != ocoeffs).any(axis=1)))
    assert np.array_equal(aliased, kept)


# ---------------------------------------------------------------- whole proofs
def _pow(proof):
    return int(proof[int(S.proof_layout(proof).off_pow_witness)])


# name: (log_n, columns) of config_cases.small_cell_air, whose cells are all 0 or 1; the share of them that gets p added
SMALL_CELL = {"64x6": (6, 6, 1.0), "1024x300": (10, 300, 0.5), "8192x5": (13, 5, 0.5), "16384x4": (14, 4, 0.5)}


@functools.lru_cache(maxsize=None)
def proof_case(name):
    """(air, config, blob, canonical row-major trace, aliased trace, public inputs); shared, read-only"""
    if name == "fibonacci":
        air, share = S.AIR_TEST_FIBONACCI, 1.0
        t, pis = S.trace_fibonacci(3, 5, 16)
        blob = S.air_program(air)
    elif name == "fp12_mul":
        air, share = S.AIR_FP12_MUL, 0.5
        t, pis = S.trace_fp12_mul(random_fp12(0x5EED7200), random_fp12(0x5EED7201))
        blob = S.air_program(air)
    else:
        log_n, cols, share = SMALL_CELL[name]
        blob, t, pis = small_cell_air(cols, 3, log_n, seed=cols + log_n)
        air = S.register_air(blob, name="alias_cells" + name, default_rows=1 << log_n)
    aliased, count = alias(t, share, 11)
    if share == 1.0:
        assert count == t.size  # every cell of these traces has an alias
    assert_aliased(aliased, t, ALL_SMALL_FLOOR, share, count)
    assert not (np.asarray(pis) >= np.uint64(P)).any()
    for a in (t, aliased, pis):
        a.setflags(write=False)
    return air, S.StarkConfig.for_air(air), blob, t, aliased, pis


@pytest.mark.parametrize("name", ["fibonacci"] + list(SMALL_CELL) + ["fp12_mul"])
def test_proof_of_an_aliased_trace_is_the_oracles_of_the_canonical_one(prover, name):
    air, cfg, blob, clean, aliased, pis = proof_case(name)
    proof = prover.prove(air, cfg, aliased, pis)
    w = _pow(proof)
    ref = O.prove(blob, cfg, clean.T.copy(), pis, w)
    assert proof.size == ref.size and np.array_equal(proof, ref)
    S.verify_stark_proof(air, cfg, proof)
    assert np.array_equal(prover.prove(air, cfg, clean, pis, pow_witness=w), proof)
    assert np.array_equal(prover.prove(air, cfg, aliased.T.copy(), pis, pow_witness=w, layout=1), proof)
    columns = [c.copy() for c in aliased.T]
    assert np.array_equal(prover.prove_columns(air, cfg, columns, pis, pow_witness=w), proof)
    assert all(np.array_equal(c, k) for c, k in zip(columns, aliased.T))  # the caller's buffers are left as they were


def test_proof_under_either_quotient_evaluator_and_through_a_pool(prover):
    air, cfg, blob, clean, aliased, pis = proof_case("64x6")
    proof = prover.prove(air, cfg, aliased, pis)
    w = _pow(proof)
    assert np.array_equal(proof, O.prove(blob, cfg, clean.T.copy(), pis, w))
    prover.set_option("quotient_impl", 1)
    try:
        other = prover.prove(air, cfg, aliased, pis, pow_witness=w)
    finally:
        prover.set_option("quotient_impl", 0)
    assert np.array_equal(other, proof)
    pool = S.ProofPool(0, big_contexts=1, small_contexts=1)
    try:
        got = pool.wait(pool.submit(air, cfg, aliased, pis, pow_witness=w))[0]
    finally:
        pool.close()
    assert np.array_equal(got, proof)


# ---------------------------------------------------------------- traces in device memory
DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first, as in tools/check_trace_bench.py
import oracle_lib as O
import starky_bls12_381_amd as S
from alias_util import ALL_SMALL_FLOOR, HAND_FLOOR, alias, assert_aliased, hand_blob, hand_violating
from check_report_util import Expected, assert_report
from config_cases import small_cell_air
from free_cells_util import assert_same
torch.cuda.set_device(0)
pv = S.Prover(0)

def on_device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return t

def unchanged(t, a):
    torch.cuda.synchronize()
    return np.array_equal(t.cpu().numpy().view(np.uint64), a)

# the checkers: the hand-written AIR, 256 rows, violated
n = 256
trace, pis = hand_violating(n)
aliased, count = alias(trace, 0.6, 2)
assert_aliased(aliased, trace, HAND_FLOOR, 0.6, count)
air = S.register_air(hand_blob())
want = Expected(hand_blob(), trace, pis)
assert want.constraints_violated >= 12
free = S.free_cells_replay(air, trace, pis)
for layout, host in ((1, aliased.T.copy()), (0, aliased)):
    dev = on_device(host)
    assert pv.check_trace_device(air, dev.data_ptr(), n, pis, layout=layout) == (want.violations, tuple(int(x) for x in want.list[0]))
    for cap in (7, 1 << 20):
        assert_report(pv.check_trace_report_device(air, dev.data_ptr(), n, pis, layout=layout, cap=cap), want, cap)
    assert_same(pv.free_cells_device(air, dev.data_ptr(), n, pis, layout=layout), free)
    assert unchanged(dev, host)  # read in place, left as it was
print("device checkers ok")

# a proof: 64 rows x 6 boolean columns, every cell aliased
blob, t, pis = small_cell_air(6, 3, 6, seed=12)
aliased, count = alias(t, 1.0, 11)
assert count == t.size
assert_aliased(aliased, t, ALL_SMALL_FLOOR)
air = S.register_air(blob)
cfg = S.StarkConfig.for_air(air)
proof = pv.prove(air, cfg, t, pis)
w = int(proof[int(S.proof_layout(proof).off_pow_witness)])
assert np.array_equal(proof, O.prove(blob, cfg, t.T.copy(), pis, w))
for layout, host in ((1, aliased.T.copy()), (0, aliased)):
    dev = on_device(host)
    assert np.array_equal(pv.prove_device(air, cfg, dev.data_ptr(), 64, pis, pow_witness=w, layout=layout), proof), layout
    assert unchanged(dev, host)
pv.close()
print("device proofs ok")
"""


def test_aliased_traces_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device checkers ok" in r.stdout and "device proofs ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
