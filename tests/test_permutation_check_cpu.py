"""starkhip_check_trace_permutations without a device: the host driver -- argument checks, the seed sequence, undecided pairs, the list
from the masks, the summary -- over the replay's host loops (starkhip_check_trace_permutations_replay), against the Python reference
of permutation_check_util.py: collections.Counter over tuples mod p, then the "highest rows" rule."""
import ctypes as C

import numpy as np
import pytest

import permutation_check_util as U
import permutation_ref as R
import starky_bls12_381_amd as S
from permutation_util import perm_air

P = R.P
SEED = S.DEFAULT_SEED


def _air3():
    air, blob = perm_air(3)
    return air, R.split_program(blob)[1]


def _replay(air, trace, **kw):
    return S.check_trace_permutations_replay(air, trace, **kw)


@pytest.mark.parametrize("noncanonical", [False, True])
@pytest.mark.parametrize("n_rows", [2, 32, 256])
def test_a_satisfying_trace_gives_an_all_zero_report(n_rows, noncanonical):
    air, pairs = _air3()
    trace = R.make_trace(3, n_rows, seed=n_rows, noncanonical=noncanonical)[0]
    assert noncanonical == bool((trace >= np.uint64(P)).any())
    for layout, t in ((0, trace), (1, np.ascontiguousarray(trace.T))):
        rep = _replay(air, t, layout=layout)
        assert (rep.pairs, rep.pairs_violated, rep.pairs_undecided, rep.unmatched, rep.reseeds) == (3, 0, 0, 0, 0)
        assert not rep.per_pair.any() and not rep.mask_words.any() and len(rep.list) == 0
        assert rep.masks.shape == (3, 2, n_rows)


def test_one_changed_cell_shows_in_exactly_the_pairs_that_name_its_column():
    air, pairs = _air3()
    trace = R.make_trace(3, 256, seed=11)[0]
    trace[100, 4] = (int(trace[100, 4]) + 1) % P  # the case of test_gpu_permutation.py: an rhs cell no constraint of the AIR reads
    rep = _replay(air, trace)
    names = [any(4 in e for e in pair) for pair in pairs]
    assert names == [True, False, True]
    assert rep.per_pair.tolist() == [1, 0, 1] and rep.pairs_violated == 2 and rep.unmatched == 4
    assert (rep.list[:, 2][rep.list[:, 1] == 1] == 100).all()  # on the rhs the changed row itself
    U.assert_equals_reference(rep, pairs, trace)
    # the closing products say only that something in each batch is off
    ch = [int(x) for x in np.random.default_rng(1).integers(0, P, 8, dtype=np.uint64)]
    assert (S.permutation_zs_replay(air, trace, ch)[1] != 1).all()


def test_unequal_multiplicities_flag_the_highest_rows():
    air, pairs = U.range_air()
    n = 32
    trace = np.zeros((n, 2), dtype=np.uint64)
    trace[:, 0] = np.arange(100, 100 + n)
    trace[:, 1] = trace[::-1, 0]
    for r in (3, 9, 20):
        trace[r, 0] = 77  # 77 three times on the lhs ...
    trace[31 - 9, 1] = 77  # ... and once on the rhs, where 103 and 120 stay without a partner
    rep = _replay(air, trace)
    assert rep.per_pair.tolist() == [2]
    assert rep.list.tolist() == [[0, 0, 9], [0, 0, 20], [0, 1, 31 - 20], [0, 1, 31 - 3]]
    U.assert_equals_reference(rep, pairs, trace)


def test_a_constant_column_is_one_run_and_clean():
    air, pairs = U.range_air()
    trace = np.full((64, 2), 5, dtype=np.uint64)
    rep = _replay(air, trace)
    assert rep.unmatched == 0 and rep.pairs_violated == 0
    trace[7, 1] = 6
    assert _replay(air, trace).list.tolist() == [[0, 0, 63], [0, 1, 7]]  # of 64 equal lhs rows the highest is the one without a partner


def test_cells_v_and_v_plus_p_count_as_equal():
    air, pairs = U.range_air()
    trace = np.array([[3, 4 + P], [4, 3 + P], [P - 1, 0], [P, P - 1]], dtype=np.uint64)
    rep = _replay(air, trace)
    assert rep.unmatched == 0
    U.assert_equals_reference(rep, pairs, trace)
    air3, pairs3 = _air3()
    t3 = R.make_trace(3, 32, seed=2, noncanonical=True)[0]
    t3[5, 3] = (int(t3[5, 3]) + 1) % P
    assert np.array_equal(_replay(air3, t3).mask_words, _replay(air3, t3 % np.uint64(P)).mask_words)
    U.assert_equals_reference(_replay(air3, t3), pairs3, t3)


def test_wide_and_many_pairs():
    # 64 pairs cannot be registered (permutation_check_util.wide_air says why): one pair of 64 entries and 48 one-entry pairs
    air, pairs = U.wide_air()
    assert len(pairs) == 49 and len(pairs[0]) == 64 and S.air_permutation_pairs(air) == 49
    trace = U.wide_trace(32, seed=4)
    assert _replay(air, trace).unmatched == 0
    trace[3, 64 + 63] = (int(trace[3, 64 + 63]) + 1) % P  # the wide pair's last entry alone
    trace[9, 64 + 10] = (int(trace[9, 64 + 10]) + 1) % P  # the wide pair and pair 11
    trace[20, 64 + 47], trace[21, 64 + 47] = trace[21, 64 + 47], trace[20, 64 + 47]  # rows 20 and 21 of the wide pair; pair 48 still holds
    rep = _replay(air, trace, cap=4096)
    per_pair = U.assert_equals_reference(rep, pairs, trace, cap=4096)
    assert per_pair[0] == 4 and per_pair[11] == 1 and per_pair[48] == 0 and sum(per_pair) == 5


def test_a_forced_collision_is_rerun_under_the_next_seed():
    air, pairs = _air3()
    trace, (t0, t1) = U.collision_trace(32, SEED)
    seeds = S.perm_check_seeds(SEED)
    assert len(seeds) == S.PERM_CHECK_ATTEMPTS == 4 and seeds[0] == SEED
    assert U.key(t0, seeds[0]) == U.key(t1, seeds[0]) and t0 != t1
    assert all(U.key(t0, s) != U.key(t1, s) for s in seeds[1:])
    rep = _replay(air, trace, seed=SEED)
    assert rep.reseeds >= 1 and rep.pairs_undecided == 0
    U.assert_equals_reference(rep, pairs, trace)
    other = _replay(air, trace, seed=12345)  # whatever the seed: the same bytes
    assert other.reseeds == 0
    assert np.array_equal(other.mask_words, rep.mask_words) and np.array_equal(other.list, rep.list) and np.array_equal(other.per_pair, rep.per_pair)


def test_the_seed_sequence():
    s = 2
    want = [s]
    for _ in range(3):
        s = (7 * s + 1) % P
        while s < 2:
            s = (7 * s + 1) % P
        want.append(s)
    assert S.perm_check_seeds(2) == want
    # 7 s + 1 = 0 mod p: the rule is applied again, 0 -> 1 -> 8
    s0 = (P - 1) * pow(7, P - 2, P) % P
    assert (7 * s0 + 1) % P == 0 and S.perm_check_seeds(s0)[:2] == [s0, 8]
    for bad in (0, 1, P, (1 << 64) - 1):
        with pytest.raises(S.StarkhipError) as e:
            S.perm_check_seeds(bad)
        assert e.value.code == S.ERR_BAD_SHAPE


def test_a_pair_that_collides_under_every_seed_is_undecided():
    air, pairs = U.wide_air()
    trace = U.undecided_trace(32, SEED)
    d = U.undecided_difference(SEED)
    assert len(d) == 5 and [(int(trace[1, t]) - int(trace[0, t])) % P for t in range(64)] == d + [0] * 59
    trace[9, 64 + 10] = (int(trace[9, 64 + 10]) + 1) % P  # pair 11 is violated and still decided
    rep = _replay(air, trace, seed=SEED)
    assert rep.pairs_undecided == 1 and int(rep.per_pair[0]) == S.PERM_UNDECIDED == 0xFFFFFFFF
    assert rep.reseeds == S.PERM_CHECK_ATTEMPTS - 1 and not rep.mask_words[0].any()
    per_pair = U.assert_equals_reference(rep, pairs, trace, undecided=(0,))
    assert per_pair[11] == 1 and rep.unmatched == 2
    # under a seed outside the four the pair is decided: row 9 of the wide pair too
    U.assert_equals_reference(_replay(air, trace, seed=424242), pairs, trace)


def test_the_list_is_cut_at_cap_in_the_fixed_order():
    air, pairs = _air3()
    trace = R.make_trace(3, 64, seed=3)[0]
    for r in (5, 17, 40):
        trace[r, 3] = (int(trace[r, 3]) + 1) % P
    full = _replay(air, trace)
    assert full.unmatched == 12 and len(full.list) == 12
    U.assert_equals_reference(full, pairs, trace)
    for cap in (0, 1, 5, 11, 12):
        rep = _replay(air, trace, cap=cap)
        assert rep.unmatched == 12 and np.array_equal(rep.list, full.list[:cap]) and np.array_equal(rep.mask_words, full.mask_words)
    # cap = 0 with list = NULL, and no per_pair or masks either: the summary alone
    out = S.api._PermCheckStruct()
    rc = S.lib.starkhip_check_trace_permutations_replay(air, trace.ctypes.data_as(C.c_void_p), 64, 6, 0, SEED, None, None, None, 0, C.byref(out))
    assert rc == 0 and (out.pairs, out.pairs_violated, out.unmatched, out.listed) == (3, 2, 12, 0)


def _raw(air, trace, n_rows, n_cols, layout=0, seed=SEED, cap=4, with_list=True, with_out=True, device=False):
    lst = np.zeros((max(1, min(cap, 16)), 3), dtype=np.uint64)
    out = S.api._PermCheckStruct()
    tail = (seed, None, None, lst.ctypes.data_as(C.POINTER(C.c_uint64)) if with_list else None, cap, C.byref(out) if with_out else None)
    ptr = trace.ctypes.data_as(C.c_void_p) if trace is not None else None
    if device:
        return S.lib.starkhip_check_trace_permutations(C.c_void_p(), air, ptr, n_rows, n_cols, layout, 0, *tail)
    return S.lib.starkhip_check_trace_permutations_replay(air, ptr, n_rows, n_cols, layout, *tail)


def test_what_the_entries_refuse():
    air, pairs = _air3()
    trace = R.make_trace(3, 32, seed=1)[0]
    assert _raw(air, trace, 32, 6) == 0
    assert _raw(air, trace, 32, 6, cap=0, with_list=False) == 0
    # BAD_AIR: an unknown AIR, a built-in AIR and a registered AIR without pairs
    b = U.AirBuilder(6, 0, 2)
    b.constraint(b.L(0) - b.L(0))
    no_pairs = S.register_air(b.finish(), name="PermCheck_no_pairs")
    fib = S.trace_fibonacci(3, 5, 32)[0]
    assert _raw(123456, trace, 32, 6) == S.ERR_BAD_AIR
    assert _raw(S.AIR_TEST_FIBONACCI, fib, 32, fib.shape[1]) == S.ERR_BAD_AIR
    assert _raw(no_pairs, trace, 32, 6) == S.ERR_BAD_AIR
    with pytest.raises(S.StarkhipError) as e:
        S.check_trace_permutations_replay(no_pairs, trace)
    assert e.value.code == S.ERR_BAD_AIR
    # BAD_SHAPE: starkhip_check_trace's cases ...
    big = np.zeros((3, 6), dtype=np.uint64)
    for kw in (dict(trace=None), dict(n_cols=5), dict(n_cols=7), dict(layout=2), dict(layout=-1), dict(n_rows=0), dict(n_rows=1), dict(n_rows=3, trace=big),
               dict(n_rows=24), dict(n_rows=1 << 21, trace=big)):
        args = dict(trace=trace, n_rows=32, n_cols=6)
        args.update(kw)
        assert _raw(air, **args) == S.ERR_BAD_SHAPE, kw
    # ... and this entry's own: the seed, the cap, a missing list, a missing result
    for kw in (dict(seed=0), dict(seed=1), dict(seed=P), dict(seed=(1 << 64) - 1), dict(cap=S.CHECK_LIST_MAX + 1), dict(cap=1, with_list=False),
               dict(with_out=False)):
        assert _raw(air, trace, 32, 6, **kw) == S.ERR_BAD_SHAPE, kw
    assert _raw(air, trace, 32, 6, seed=2) == 0 and _raw(air, trace, 32, 6, seed=P - 1) == 0
    with pytest.raises(S.StarkhipError) as e:
        S.check_trace_permutations_replay(air, trace, cap=S.CHECK_LIST_MAX + 1)
    assert e.value.code == S.ERR_BAD_SHAPE
    # the device entry without a context refuses before it looks at anything else
    assert _raw(air, trace, 32, 6, device=True) == S.ERR_NO_DEVICE


def test_a_trace_can_close_every_z_and_still_fail_the_check():
    # COMPAT.md 2a: one (beta, gamma) per batch, so the argument sees the union of a batch's pairs; the check looks at each pair
    b = U.AirBuilder(4, 0, 3)  # B = 2: both pairs in one batch
    b.constraint(b.L(0) - b.L(0))
    b.permutation_pair([(0, 1)])
    b.permutation_pair([(2, 3)])
    blob = b.finish()
    air = S.register_air(blob, name="PermCheck_crossed")
    rng = np.random.default_rng(6)
    n = 32
    a, c = rng.integers(0, P, n, dtype=np.uint64), rng.integers(0, P, n, dtype=np.uint64)
    trace = np.ascontiguousarray(np.stack([a, c[rng.permutation(n)], c, a[rng.permutation(n)]], axis=1))  # column 1 holds c's values, column 3 a's
    ch = [int(x) for x in rng.integers(0, P, 8, dtype=np.uint64)]
    assert (S.permutation_zs_replay(air, trace, ch)[1] == 1).all()
    rep = _replay(air, trace, cap=4096)
    assert rep.pairs_violated == 2 and rep.per_pair.tolist() == [n, n]
    U.assert_equals_reference(rep, R.split_program(blob)[1], trace, cap=4096)


def test_rust_mirror_has_the_new_names():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rs = open(os.path.join(root, "bindings", "rust", "starkhip-sys", "src", "lib.rs")).read()
    hdr = open(os.path.join(root, "include", "starkhip.h")).read()
    for name in ("starkhip_check_trace_permutations", "starkhip_check_trace_permutations_replay", "starkhip_perm_check_seeds",
                 "starkhip_perm_check_timings"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
    fields = re.search(r"typedef struct \{([^}]*)\} starkhip_perm_check_t;", hdr).group(1)
    names = re.findall(r"\b(pairs|pairs_violated|pairs_undecided|unmatched|listed|reseeds)\b(?=[,;])", re.sub(r"/\*.*?\*/", "", fields))
    assert names == ["pairs", "pairs_violated", "pairs_undecided", "unmatched", "listed", "reseeds"]
    mirror = re.search(r"pub struct starkhip_perm_check_t \{(.*?)\n\}", rs, re.S).group(1)
    assert re.findall(r"pub (\w+): u64", mirror) == names
    assert [f for f, _ in S.api._PermCheckStruct._fields_] == names
    assert "#define STARKHIP_PERM_CHECK_ATTEMPTS 4" in hdr and "STARKHIP_PERM_CHECK_ATTEMPTS: usize = 4" in rs
