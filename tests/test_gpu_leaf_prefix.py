"""The leaf hash's saved state past an identity prefix ("leaf_hash_prefix"; kernels.h: LeafPrefix).  Where the first n columns of an
n-row trace are the unit vectors e_0 .. e_{n-1}, the lane and pair forms start every leaf at block n / 8 from a table of the shape; the
proof's own LDE says whether they are (a counter the LDE kernels fill), and every other trace is hashed in full.

Kernel level, at the smallest shape with closed forms (4 096 rows, rate_bits 1: 8 192 leaves), through starkhip_lde_batch -- which
counts as prove() does -- and starkhip_leaf_hash_lane_group, whose prefix_mask hands chosen segments the context's counter and table:
digests with the prefix equal the digests without it word for word and their Merkle cap is the CPU oracle's, for 4 096 + 7 columns
(must not skip), + 8 and + 19, in the lane form alone, in a group of two of which one member has the prefix, and in the pair form.  That
the skip happens at all is shown by what it does not read: a cell of a prefix column changed AFTER the LDE changes no digest with the
prefix and one digest without it.  Near misses of the identity keep the equality (the counter misses n: the full hash runs), also right
after a trace that had the prefix.  The table equals the host sponge over the rotated LDE of e_0.  End to end: FinalExp proofs with the
option at 0 and at 1 are the same bytes with the committed oracle digest, and so is what a trace with one selector cell cleared gives."""
import hashlib
import os

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S

pytestmark = pytest.mark.gpu
P = S.P
LOG_N, RATE = 12, 1
n, R = 1 << LOG_N, 1 << RATE
N = n * R
CAP_H = 4
EXTRA = (7, 8, 19)


def coset_major(lde_natural):
    """[C][N] in natural point order i = k R + s -> [C][N] at q = s n + k, the device layout the leaf kernels read"""
    c = lde_natural.shape[0]
    return np.ascontiguousarray(lde_natural.reshape(c, n, R).transpose(0, 2, 1)).reshape(c, N)


def bump(mat, col, q):
    mat[col, q] = (int(mat[col, q]) + 1) % P


def cap_of(digests):
    """the cap of height CAP_H over leaf digests [N][4] in tree order, with the host permutation (two_to_one: a | b | 0000)"""
    level = digests
    while level.shape[0] > (1 << CAP_H):
        nxt = np.zeros((level.shape[0] // 2, 4), dtype=np.uint64)
        for j in range(nxt.shape[0]):
            state = np.zeros(12, dtype=np.uint64)
            state[:4] = level[2 * j]
            state[4:8] = level[2 * j + 1]
            nxt[j] = S.api.poseidon_permute_host(state)[:4]
        level = nxt
    return level


@pytest.fixture(scope="module")
def values():
    """[4 096 + 19][4 096]: the identity, then random columns"""
    rng = np.random.default_rng(0x1EAF)
    v = np.zeros((n + max(EXTRA), n), dtype=np.uint64)
    v[np.arange(n), np.arange(n)] = 1
    v[n:] = rng.integers(0, P, size=(max(EXTRA), n), dtype=np.uint64)
    return v


@pytest.fixture(scope="module")
def other():
    """another matrix of the largest shape, already coset-major: the group's member without a prefix"""
    return np.random.default_rng(0x07E2).integers(0, P, size=(n + max(EXTRA), N), dtype=np.uint64)


@pytest.fixture(scope="module")
def fresh():
    """a context of this module's own: its option and its counter are what the tests are about"""
    pv = S.Prover(0)
    yield pv
    pv.close()


def hash_both_ways(pv, mat, form, mask=1, mats=None, grouped=False):
    m = mat[None] if mats is None else mats
    on = pv.leaf_hash_lane_group(m, LOG_N, RATE, grouped=grouped, form=form, prefix_mask=mask)
    off = pv.leaf_hash_lane_group(m, LOG_N, RATE, grouped=grouped, form=form, prefix_mask=0)
    return on, off


@pytest.mark.parametrize("extra", EXTRA)
def test_digests_with_the_prefix_equal_those_without_and_the_oracle_cap(fresh, values, other, extra):
    c = n + extra
    _, lde = fresh.lde_batch(values[:c], RATE)
    want_cap = O.merkle_cap(np.ascontiguousarray(lde.T), CAP_H)
    mat = coset_major(lde)
    del lde
    lane_on, lane_off = hash_both_ways(fresh, mat, 3)
    assert np.array_equal(lane_on, lane_off), "lane form, %d columns" % c
    assert np.array_equal(cap_of(lane_on[0]), want_cap)
    pair_on, pair_off = hash_both_ways(fresh, mat, 4)
    assert np.array_equal(pair_on, pair_off), "pair form, %d columns" % c
    assert np.array_equal(pair_on, lane_on)
    # a group of two, ONE grid: member 0 has the prefix, member 1 (another matrix) has none; then the other way round
    for mats, mask in ((np.stack([mat, other[:c]]), 1), (np.stack([other[:c], mat]), 2)):
        on, off = hash_both_ways(fresh, None, 3, mask=mask, mats=mats, grouped=True)
        assert np.array_equal(on, off), "group of two, mask %d, %d columns" % (mask, c)
        assert np.array_equal(on[mask - 1], lane_on[0])
    # the skip is real where it may happen and only there: a cell of prefix column 5 changed after the LDE is not read with the prefix
    q = 1234
    bump(mat, 5, q)
    for form in (3, 4):
        on, off = hash_both_ways(fresh, mat, form)
        changed_on = np.argwhere((on != lane_on).any(axis=2)).tolist()
        changed_off = np.argwhere((off != lane_on).any(axis=2)).tolist()
        assert len(changed_off) == 1
        assert changed_on == ([] if extra >= 8 else changed_off), "form %d, %d columns" % (form, c)


def near_misses(v):
    """(name, the change) -- each leaves a trace whose first n columns are NOT e_0 .. e_{n-1}"""
    def moved(m):
        m[7, 7], m[7, 9] = 0, 1
    def doubled(m):
        m[100, 100] = 2
    def two_ones(m):
        m[n - 1, 3] = 1
    def all_zero(m):
        m[0, 0] = 0
    def shifted(m):
        m[1:n + 1] = v[:n]
        m[0] = v[n]
    return [("one selector's 1 in another row", moved), ("one selector doubled", doubled), ("one selector with two ones", two_ones),
            ("one selector all zero", all_zero), ("the identity in columns 1 .. n", shifted)]


@pytest.mark.parametrize("case", range(6))
def test_near_misses_of_the_identity_are_hashed_in_full(fresh, values, case):
    c = n + 8
    cases = [(name, change, 1) for name, change in near_misses(values)] + [("lde_closed_forms = 0", lambda m: None, 0)]
    for name, change, closed in cases[case:case + 1]:
        # the stale state: right before every near miss, a trace that HAS the prefix leaves its count in the context
        _, lde = fresh.lde_batch(values[:c], RATE)
        good = coset_major(lde)
        on, off = hash_both_ways(fresh, good, 3)
        assert np.array_equal(on, off)
        bump(good, 5, 77)
        assert np.array_equal(fresh.leaf_hash_lane_group(good[None], LOG_N, RATE, grouped=False, prefix_mask=1), on), "the good trace did not skip"
        v = values[:c].copy()
        change(v)
        fresh.set_option("lde_closed_forms", closed)
        try:
            _, lde = fresh.lde_batch(v, RATE)
        finally:
            fresh.set_option("lde_closed_forms", 1)
        mat = coset_major(lde)
        del lde
        for form in (3, 4):
            on, off = hash_both_ways(fresh, mat, form)
            assert np.array_equal(on, off), "%s, form %d" % (name, form)
        bump(mat, 5, 77)   # ... and it was the full hash: the changed prefix cell is read
        assert not np.array_equal(fresh.leaf_hash_lane_group(mat[None], LOG_N, RATE, grouped=False, prefix_mask=1), on), name


def test_option_off_gives_null_pointers(values):
    pv = S.Prover(0)
    try:
        c = n + 8
        _, lde = pv.lde_batch(values[:c], RATE)
        mat = coset_major(lde)
        want = pv.leaf_hash_lane_group(mat[None], LOG_N, RATE, grouped=False, prefix_mask=1)
        pv.set_option("leaf_hash_prefix", 0)
        pv.lde_batch(values[:c], RATE)
        bump(mat, 5, 77)
        got = pv.leaf_hash_lane_group(mat[None], LOG_N, RATE, grouped=False, prefix_mask=1)
        assert len(np.argwhere((got != want).any(axis=2))) == 1   # nothing skipped
        with pytest.raises(S.StarkhipError):
            pv.leaf_prefix_table(LOG_N, RATE)
        with pytest.raises(S.StarkhipError):
            pv.set_option("leaf_hash_prefix", 2)
    finally:
        pv.close()


def test_the_table_is_the_host_sponge_over_the_rotated_lde_of_e0(fresh):
    e0 = np.zeros((1, n), dtype=np.uint64)
    e0[0, 0] = 1
    _, lde = fresh.lde_batch(e0, RATE)
    e0_lde = coset_major(lde)[0].reshape(R, n)
    cap = fresh.leaf_prefix_table(LOG_N, RATE)
    assert cap.shape == (4, N) and (cap < P).all()
    for q in (0, n - 1, n, N - 1, 1, 2 * n - 1, 4321):
        s, k = divmod(q, n)
        state = np.zeros(12, dtype=np.uint64)
        for b in range(n // 8):
            state[:8] = e0_lde[s, (k - 8 * b - np.arange(8)) % n]
            state = S.api.poseidon_permute_host(state)
        assert np.array_equal(cap[:, q], state[8:]), "leaf %d" % q


def test_final_exp_proofs_are_the_same_bytes_either_way():
    """One FinalExp proof with "leaf_hash_prefix" 0 and with 1, in the lane and in the pair form: identical bytes with the committed
    oracle digest."""
    from bls_util import GOLDEN, random_fp12
    air = S.AIR_FINAL_EXP
    cfg = S.StarkConfig.for_air(air)
    want = open(os.path.join(GOLDEN, "final_exp_seed_5eed0001_proof.sha256")).read().split()[0]
    trace, pis = S.trace_final_exp(random_fp12(0x5EED0001), compact=True)
    pv = S.Prover(0)
    try:
        for form in (3, 4):
            pv.set_option("leaf_hash_form", form)
            for on in (1, 0, 1):
                pv.set_option("leaf_hash_prefix", on)
                proof = pv.prove(air, cfg, trace, pis)
                assert hashlib.sha256(proof.tobytes()).hexdigest() == want, (form, on)
    finally:
        pv.close()


BROKEN_SELECTOR_CHILD = r"""
import os, sys, hashlib, faulthandler
faulthandler.dump_traceback_later(150, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import starky_bls12_381_amd as S
from bls_util import random_fp12
torch.cuda.set_device(0)
air = S.AIR_FINAL_EXP
cfg = S.StarkConfig.for_air(air)
want = open(%(golden)r).read().split()[0]
dense, pis = S.trace_final_exp(random_fp12(0x5EED0001))
rows = dense.shape[0]
cols = torch.from_numpy(dense.view(np.int64)).to("cuda:0").t().contiguous()   # column-major [C][rows] on the device
del dense
torch.cuda.synchronize()
provers = {}
for on in (1, 0):
    provers[on] = S.Prover(0)
    provers[on].set_option("leaf_hash_prefix", on)
    provers[on].set_option("leaf_hash_form", 3)
def outcome(pv):
    try:
        return ("proof", hashlib.sha256(pv.prove_device(air, cfg, cols.data_ptr(), rows, pis, layout=1).tobytes()).hexdigest())
    except S.StarkhipError as e:
        return ("error", e.code)
# the context with the option proves the good trace first (its counter reaches the row count), then the broken one, then the good one again
assert outcome(provers[1]) == ("proof", want)
assert int(cols[300, 300]) == 1
cols[300, 300] = 0   # selector column 300 is all zero now
torch.cuda.synchronize()
got = {on: outcome(provers[on]) for on in (1, 0)}
assert got[1] == got[0], got
assert got[1] != ("proof", want)
cols[300, 300] = 1
torch.cuda.synchronize()
assert outcome(provers[1]) == ("proof", want)
for pv in provers.values():
    pv.close()
print("broken selector ok", got[1][0])
"""


def test_a_final_exp_trace_with_a_cleared_selector_cell_gives_the_same_either_way():
    """Device-resident columns of a FinalExp trace with one selector cell cleared: what comes out -- proof bytes, or the error of a
    quotient that does not divide -- is the same with "leaf_hash_prefix" 1 and 0, on a context that has just proven a trace WITH the
    prefix; the good trace proves to the oracle digest before and after."""
    import subprocess
    import sys
    from bls_util import GOLDEN
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    child = BROKEN_SELECTOR_CHILD % {"root": root, "golden": os.path.join(GOLDEN, "final_exp_seed_5eed0001_proof.sha256")}
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "broken selector ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
