"""starkhip_check_trace_permutations on the GPU (csrc/permutation_check.hip over csrc/kernels_multiset.hip: keys, the stable radix sort,
the classification; the tile, the workgroup scan and the run-end search are csrc/block_scan.h's): the device result equals the replay and the Python reference of permutation_check_util.py byte for byte -- counts, per_pair, masks and
list.  The shapes are the smallest at which the sort can go wrong: 2 rows (four items, less than a wave), 32 (2 n is one wave), 512
and 1024 (2 n is one and two workgroups' tiles: MULTISET_TILE = 1024 items), 2^13 and 2^14 (16 and 32 tiles: a digit table of one scan
chunk, scanned without chunk sums, and the first of two), and one run at 2^20 rows (a table of 128 chunks) against the C++ replay alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

import permutation_check_util as U
import permutation_ref as R
import starky_bls12_381_amd as S
from permutation_util import golden_case, load_golden, perm_air

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
SEED = S.DEFAULT_SEED
SMALL = [2, 32, 512, 1024]  # csrc/kernels_multiset.h: MULTISET_TILE = TILE_ITEMS (csrc/block_scan.h) = 1024 items per workgroup


def _check(prover, air, pairs, trace, reference=True, **kw):
    """the device's report from both host layouts; equal to the replay's and, unless told otherwise, to the reference"""
    want = S.check_trace_permutations_replay(air, trace, **kw)
    for layout, t in ((0, trace), (1, np.ascontiguousarray(trace.T))):
        rep = prover.check_trace_permutations(air, t, layout=layout, **kw)
        U.assert_same_report(rep, want)
    if reference:
        U.assert_equals_reference(want, pairs, trace, cap=kw.get("cap", 1024))
    return want


@pytest.mark.parametrize("n_rows", SMALL + [1 << 13, 1 << 14])  # 2^13: the largest digit table of one scan chunk; 2^14: two chunks
def test_three_pairs_clean_and_broken(prover, n_rows):
    air, blob = perm_air(3, 8)
    pairs = R.split_program(blob)[1]
    trace = R.make_trace(3, n_rows, seed=n_rows + 1, n_cols=8, noncanonical=True)[0]
    assert (trace >= np.uint64(P)).any()
    assert _check(prover, air, pairs, trace).unmatched == 0
    rng = np.random.default_rng(n_rows)
    for r in sorted({0} | {int(x) for x in rng.integers(0, n_rows, 5)}):  # row 0: column 3, which pairs 0 and 1 name
        c = 3 + r % 3
        trace[r, c] = (int(trace[r, c]) + 1) % P
    rep = _check(prover, air, pairs, trace, cap=7)
    assert rep.pairs_violated >= 2 and len(rep.list) == min(7, rep.unmatched)


def _family(name, n, rng):
    """the lhs cells of one key family: for the one-entry pair the sort key is the cell"""
    r = np.arange(n, dtype=np.uint64)
    if name == "top_byte":
        return (r % np.uint64(251)) << np.uint64(56)  # 250 << 56 < p
    if name == "bottom_byte":
        return (r * np.uint64(7)) % np.uint64(256)
    if name == "all_equal":
        return np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    if name == "equal_within_a_wave":
        return (r // np.uint64(64)) * np.uint64(0x0101010101010101)
    if name == "noncanonical":
        v = rng.integers(0, 1 << 31, n, dtype=np.uint64)
        v[::2] += np.uint64(P)  # fits: v < 2^32 - 1
        return v
    assert name == "multiplicities"
    return rng.integers(0, max(2, n // 8), n, dtype=np.uint64)


@pytest.mark.parametrize("n_rows", SMALL)
@pytest.mark.parametrize("family", ["top_byte", "bottom_byte", "all_equal", "equal_within_a_wave", "noncanonical", "multiplicities"])
def test_key_families(prover, family, n_rows):
    air, pairs = U.range_air()
    rng = np.random.default_rng(n_rows)
    lhs = _family(family, n_rows, rng)
    # the rhs in the lhs' own order (equal_within_a_wave: every wave of rhs items holds one key too), or shuffled
    rhs = lhs.copy() if family == "equal_within_a_wave" else lhs[rng.permutation(n_rows)]
    trace = np.ascontiguousarray(np.stack([lhs, rhs], axis=1))
    assert _check(prover, air, pairs, trace).unmatched == 0
    # unequal multiplicities: a few rhs cells take the value of another row, or one no lhs row holds
    for r in sorted({0} | {int(x) for x in rng.integers(0, n_rows, 4)}):
        trace[r, 1] = trace[(r * 5 + 1) % n_rows, 0] if r % 2 else np.uint64(0x7777777777777777)
    rep = _check(prover, air, pairs, trace)
    assert rep.pairs_violated == 1


def test_wide_and_many_pairs(prover):
    air, pairs = U.wide_air()
    trace = U.wide_trace(32, seed=4)
    trace[3, 64 + 63] = (int(trace[3, 64 + 63]) + 1) % P
    trace[9, 64 + 10] = (int(trace[9, 64 + 10]) + 1) % P
    rep = _check(prover, air, pairs, trace, cap=4096)
    assert rep.per_pair.tolist()[0] == 2 and rep.per_pair.tolist()[11] == 1


def test_forced_collision_and_forced_undecided(prover):
    air, blob = perm_air(3)
    trace, (t0, t1) = U.collision_trace(32, SEED)
    assert U.key(t0, SEED) == U.key(t1, SEED)
    rep = _check(prover, air, R.split_program(blob)[1], trace, seed=SEED)
    assert rep.reseeds >= 1 and rep.pairs_undecided == 0
    wide, wpairs = U.wide_air()
    trace = U.undecided_trace(32, SEED)
    trace[9, 64 + 10] = (int(trace[9, 64 + 10]) + 1) % P
    rep = _check(prover, wide, wpairs, trace, reference=False, seed=SEED)
    assert rep.pairs_undecided == 1 and rep.reseeds == 3
    U.assert_equals_reference(rep, wpairs, trace, undecided=(0,))


def test_a_million_rows_of_a_range_check(prover):
    air, pairs = U.range_air()
    n = 1 << 20
    rng = np.random.default_rng(20)
    lhs = rng.integers(0, 1 << 16, n, dtype=np.uint64)  # a 16-bit range check: long runs of equal keys
    rhs = np.sort(lhs)
    trace = np.ascontiguousarray(np.stack([lhs, rhs], axis=1))
    for r in (0, 77777, n - 1):
        trace[r, 1] = np.uint64(1 << 16) + np.uint64(r)
    want = S.check_trace_permutations_replay(air, trace, cap=16)
    assert want.unmatched == 6
    U.assert_same_report(prover.check_trace_permutations(air, trace, cap=16), want)


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import permutation_ref as R
import permutation_check_util as U
import starky_bls12_381_amd as S
from permutation_util import perm_air
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")
pv = S.Prover(0)
air, blob = perm_air(3, 8)
for n in (32, 1024):
    trace = R.make_trace(3, n, seed=n, n_cols=8, noncanonical=True)[0]
    trace[n // 2, 4] = (int(trace[n // 2, 4]) + 1) %% R.P   # column 4: the three-entry pair and the pair (1, 4)
    want = S.check_trace_permutations_replay(air, trace)
    assert want.unmatched == 4
    for layout, t in ((0, dev(trace)), (1, dev(trace.T))):
        torch.cuda.synchronize()
        U.assert_same_report(pv.check_trace_permutations_device(air, t.data_ptr(), n, layout=layout), want)
        assert np.array_equal(t.cpu().numpy().view(np.uint64), trace if layout == 0 else trace.T)  # read in place, left as it was
pv.close()
print("device forms ok")
"""


def test_traces_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_context_still_gives_the_golden_proof():
    air, blob, cfg, trace, pis = golden_case()
    bad = trace.copy()
    bad[7, 4] = (int(bad[7, 4]) + 1) % P
    p = S.Prover(0)
    try:
        rep = p.check_trace_permutations(air, bad)
        assert rep.per_pair.tolist() == [1, 0, 1]
        assert p.check_trace_permutations(air, trace).unmatched == 0
        assert np.array_equal(p.prove(air, cfg, trace, pis), load_golden()[S.HASHER_POSEIDON])
        assert p.check_trace_permutations(air, bad).list.tolist() == rep.list.tolist()
    finally:
        p.close()
