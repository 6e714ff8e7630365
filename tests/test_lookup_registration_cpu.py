"""An AIR registered with its lookups (starkhip_air_register_lookups, _air_lookups, _air_check_lookups) and the lookup blob a prove
with "fill_lookups" hands back (starkhip_lookup_blob_replay, _lookup_blob_layout), without a device.  The ground truth for what a
blob must hold is tests/lookup_ref.py."""
import os

import numpy as np
import pytest

import lookup_ref as R
import starky_bls12_381_amd as S
from starky_bls12_381_amd.air_builder import AirBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COLS = 11
LOOKUPS = [(0, 3, 5, 6), (1, 3, 7, 8), (2, 4, 9, 10)]  # three value columns, two tables (one shared), the permuted columns


def _builder(lookups=LOOKUPS, n_cols=N_COLS, degree=4):  # (degree 4: B = 3 pairs a batch, so the six pairs of three lookups fit)
    b = AirBuilder(n_cols, 0, degree)
    for lk in lookups:
        b.lookup(*lk)
    return b


def _blob(lookups=LOOKUPS, **kw):
    return _builder(lookups, **kw).finish()


# ------------------------------------------------------------------------------------------------ the validation
def test_a_builders_list_is_accepted():
    b = _builder()
    blob = b.finish()
    assert b.lookups == LOOKUPS
    assert S.air_check_lookups(blob, b.lookups) is None
    assert S.air_check_lookups(blob, b.lookups[1:]) is None  # a part of what the program declares is covered too


@pytest.mark.parametrize("field", range(4))
def test_column_out_of_range(field):
    bad = list(LOOKUPS[0])
    bad[field] = N_COLS
    why = S.air_check_lookups(_blob(), [tuple(bad)] + LOOKUPS[1:])
    assert why and "out of range" in why and "lookup 0" in why
    with pytest.raises(S.StarkhipError) as e:
        S.register_air(_blob(), lookups=[tuple(bad)] + LOOKUPS[1:])
    assert e.value.code == S.ERR_BAD_AIR


@pytest.mark.parametrize("lookups, word", [
    ([(0, 3, 5, 6), (5, 3, 7, 8)], "input"),     # lookup 0's output is lookup 1's input
    ([(0, 6, 5, 7), (1, 3, 6, 8)], "table"),     # lookup 1's output is lookup 0's table
    ([(0, 3, 5, 6), (1, 3, 5, 8)], "output"),    # both write column 5
    ([(0, 3, 5, 6), (1, 3, 7, 6)], "output"),    # both write column 6
    ([(0, 3, 5, 5)], "both"),                    # one lookup, one column for its two outputs
])
def test_output_column_rules(lookups, word):
    why = S.air_check_lookups(_blob(), lookups)
    assert why and word in why, why


def test_lookup_counts():
    blob = _blob()
    why = S.air_check_lookups(blob, [])
    assert why and "no lookups" in why
    many = [(0, 3, 5, 6)] * 65
    why = S.air_check_lookups(blob, many)
    assert why and "65" in why and "64" in why
    for lookups in ([], many):
        with pytest.raises(S.StarkhipError) as e:
            S.register_air(blob, lookups=lookups)
        assert e.value.code == S.ERR_BAD_AIR


@pytest.mark.parametrize("drop", (0, 1))
def test_program_must_declare_both_pairs(drop):
    """the constraints and one pair of lookup (2, 4, 9, 10), written by hand: the list names a pair the program does not bind"""
    b = AirBuilder(N_COLS, 0, 3)
    b.lookup(0, 3, 5, 6)
    b.constraint((b.N(9) - b.L(9)) * (b.N(9) - b.N(10)))
    b.last_row(b.N(9) - b.N(10))
    b.permutation_pair([(4, 10)] if drop == 0 else [(2, 9)])
    blob = b.finish()
    assert S.air_check_program(blob) is None
    why = S.air_check_lookups(blob, [(0, 3, 5, 6), (2, 4, 9, 10)])
    assert why and "lookup 1" in why and "declares no permutation pair" in why
    assert ("(2, 9)" in why) == (drop == 0) and ("(4, 10)" in why) == (drop == 1)
    assert S.air_check_lookups(blob, [(0, 3, 5, 6)]) is None
    # a pair of two entries that holds the lookup's columns among others is not the lookup's pair
    b2 = AirBuilder(N_COLS, 0, 3)
    b2.constraint((b2.N(5) - b2.L(5)) * (b2.N(5) - b2.N(6)))
    b2.last_row(b2.N(5) - b2.N(6))
    b2.permutation_pair([(0, 5), (1, 7)])
    b2.permutation_pair([(3, 6)])
    why = S.air_check_lookups(b2.finish(), [(0, 3, 5, 6)])
    assert why and "(0, 5)" in why


def test_a_bad_program_is_refused_with_its_own_reason():
    blob = _blob().copy()
    blob[0] ^= np.uint64(1)
    why = S.air_check_lookups(blob, LOOKUPS)
    assert why and "magic" in why


# ------------------------------------------------------------------------------------------------ ids
def test_ids():
    blob = _blob()
    a = S.register_air(blob, name="LookupReg_full", default_rows=64, lookups=LOOKUPS)
    assert S.register_air(blob, name="LookupReg_again", lookups=LOOKUPS) == a
    assert S.air_lookups(a) == LOOKUPS
    plain = S.register_air(blob, name="LookupReg_plain")
    assert plain != a and S.air_lookups(plain) == []
    assert S.register_air(blob) == plain  # the plain id is stable too
    part = S.register_air(blob, lookups=LOOKUPS[:2])
    assert part not in (a, plain) and S.air_lookups(part) == LOOKUPS[:2]
    swapped = S.register_air(blob, lookups=LOOKUPS[::-1])
    assert swapped not in (a, plain, part) and S.air_lookups(swapped) == LOOKUPS[::-1]
    for air in (a, plain, part, swapped):  # one program: what every verifier reads is the same
        assert np.array_equal(S.air_program(air), blob)
        assert S.air_columns(air) == N_COLS and S.air_permutation_pairs(air) == 6
    assert S.air_default_rows(a) == 64


def test_builtin_airs_have_no_lookups():
    for air in (S.AIR_FP12_MUL, S.AIR_FINAL_EXP, S.AIR_TEST_FIBONACCI, S.AIR_MILLER_LOOP, S.AIR_PAIRING_PRECOMP, S.AIR_ECC_AGGREGATE):
        assert S.air_lookups(air) == []
    assert S.air_lookups(12345) == []


def test_python_and_cpp_builders_agree():
    """the C++ AirBuilder's program registered with AirBuilder::lookups() is the Python builder's (blob, list): one id"""
    b = _builder()
    blob = b.finish()
    assert np.array_equal(S.lookup_air_blob(N_COLS, 4, LOOKUPS), blob)
    cpp = S.lookup_air_register(N_COLS, 4, LOOKUPS, name="LookupReg_cpp")
    assert S.air_lookups(cpp) == b.lookups
    assert S.register_air(blob, lookups=b.lookups) == cpp
    five = [(q, 5, 6 + 2 * q, 7 + 2 * q) for q in range(5)]
    b5 = _builder(five, n_cols=16, degree=5)
    cpp5 = S.lookup_air_register(16, 5, five)
    assert S.air_lookups(cpp5) == b5.lookups == five and S.register_air(b5.finish(), lookups=five) == cpp5


# ------------------------------------------------------------------------------------------------ lookup blobs
def _air():
    return S.register_air(_blob(), name="LookupReg_blob", lookups=LOOKUPS)


def _trace(n, seed, bad=()):
    """[n][11]: inputs in 0 .. 2, tables 0 .. n - 1 in 3 and 4, other bytes in the permuted columns; bad: (column, row, value) cells"""
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 1 << 63, (n, N_COLS), dtype=np.uint64)
    t[:, :3] = rng.integers(0, n, (n, 3), dtype=np.uint64)
    t[:, 3] = rng.permutation(n)
    t[:, 4] = np.arange(n)
    for c, r, v in bad:
        t[r, c] = v
    return t


def _expect(air, trace, blob, cap, layout=0):
    """the blob against lookup_ref.fill of the same trace"""
    _, per, _, entries = R.fill(trace, LOOKUPS, layout)
    rep = S.parse_lookup_blob(blob)
    n = trace.shape[0] if layout == 0 else trace.shape[1]
    assert (rep.air, rep.n_rows, rep.lookups) == (air, n, len(LOOKUPS))
    assert rep.failed == sum(1 for c in per if c) and rep.missing_rows == sum(per)
    assert rep.list.tolist() == [list(e) for e in entries[:cap]]
    assert int(blob[0]) == S.LOOKUP_MAGIC and int(blob[7]) == 0 and blob.size == 8 + 2 * min(cap, len(entries))
    return rep


@pytest.mark.parametrize("layout", (0, 1))
def test_blob_replay_against_the_reference(layout):
    air, n = _air(), 64
    good = _trace(n, 1)
    arg = (lambda t: np.ascontiguousarray(t.T)) if layout else (lambda t: t)
    assert S.lookup_blob_replay(air, arg(good), layout=layout) is None
    one = _trace(n, 2, bad=[(1, 17, n + 5)])
    before = arg(one).copy()
    blob = S.lookup_blob_replay(air, before, layout=layout)
    assert np.array_equal(before, arg(one))  # the trace is only read
    rep = _expect(air, arg(one), blob, 16, layout)
    assert rep.failed == 1 and rep.list.tolist() == [[1, 17]]
    every = _trace(n, 3)
    every[:, 0] = np.arange(n) + n  # every row of lookup 0 is missing
    rep = _expect(air, arg(every), S.lookup_blob_replay(air, arg(every), layout=layout, cap=1024), 1024, layout)
    assert rep.missing_rows == n and rep.list.tolist() == [[0, r] for r in range(n)]
    two = _trace(n, 4, bad=[(0, 3, R.P - 1), (0, 60, n), (2, 0, 1 << 40)])  # lookups 0 and 2 fail beside lookup 1, which holds
    rep = _expect(air, arg(two), S.lookup_blob_replay(air, arg(two), layout=layout), 16, layout)
    assert rep.failed == 2 and rep.list.tolist() == [[0, 3], [0, 60], [2, 0]]


@pytest.mark.parametrize("cap", (0, 1, 5, 64, 65))
def test_blob_list_is_cut_at_cap(cap):
    air, n = _air(), 64
    t = _trace(n, 5, bad=[(2, 9, n)])
    t[:, 0] = np.arange(n) + n
    rep = _expect(air, t, S.lookup_blob_replay(air, t, cap=cap), cap)
    assert rep.missing_rows == n + 1 and len(rep.list) == min(cap, n + 1)


def test_blob_replay_without_a_list_and_bad_arguments():
    plain = S.register_air(_blob())
    assert S.lookup_blob_replay(plain, _trace(64, 6, bad=[(0, 0, 999)])) is None
    air = _air()
    for bad in (np.zeros((64, N_COLS + 1), dtype=np.uint64), np.zeros((48, N_COLS), dtype=np.uint64)):
        with pytest.raises(S.StarkhipError) as e:
            S.lookup_blob_replay(air, bad)
        assert e.value.code == S.ERR_BAD_SHAPE
    with pytest.raises(S.StarkhipError) as e:
        S.lookup_blob_replay(777, _trace(64, 6))
    assert e.value.code == S.ERR_BAD_AIR


def test_blob_layout_refuses_what_is_no_lookup_blob():
    air, n = _air(), 64
    t = _trace(n, 7, bad=[(0, 1, n), (0, 2, n + 1), (1, 5, n)])
    blob = S.lookup_blob_replay(air, t)
    assert S.parse_lookup_blob(blob).missing_rows == 3

    def refused(b):
        with pytest.raises(S.StarkhipError) as e:
            S.parse_lookup_blob(b)
        return e.value.code == S.ERR_BAD_SHAPE

    proof = blob.copy()
    proof[0] = 0x3130304652505353  # STARKHIP_PROOF_MAGIC
    assert refused(proof)
    # a check blob of the same AIR: its own parser takes it, this one does not
    check = S.check_blob_replay(air, t, [])
    assert check is not None and S.parse_check_blob(check).violations > 0 and refused(check)
    with pytest.raises(S.StarkhipError):
        S.parse_check_blob(blob)
    assert refused(blob[:-1]) and refused(blob[:7]) and refused(np.zeros(0, dtype=np.uint64))
    assert refused(np.concatenate([blob, blob[-2:]]))
    more = blob.copy()
    more[6] += np.uint64(1)  # listed disagrees with the length
    assert refused(more)
    fewer = blob.copy()
    fewer[6] -= np.uint64(1)
    assert refused(fewer)
    over = blob.copy()
    over[5] = 2  # more listed than missing
    assert refused(over)
    nonzero = blob.copy()
    nonzero[7] = 1
    assert refused(nonzero)
    v = S.TraceViolation(blob)
    assert v.report is None and v.lookup_report.list.tolist() == [[0, 1], [0, 2], [1, 5]]
    v = S.TraceViolation(check)
    assert v.lookup_report is None and v.report.violations > 0


# ------------------------------------------------------------------------------------------------ bindings
def test_rust_declarations_are_present():
    with open(os.path.join(ROOT, "bindings", "rust", "starkhip-sys", "src", "lib.rs")) as f:
        text = f.read()
    for name in ("starkhip_air_register_lookups", "starkhip_air_lookups", "starkhip_air_check_lookups", "starkhip_lookup_blob_layout",
                 "starkhip_lookup_blob_replay", "STARKHIP_LOOKUP_MAGIC"):
        assert name in text, name
    with open(os.path.join(ROOT, "include", "starkhip.h")) as f:
        header = f.read()
    assert "0x313030504B4C5353" in header and "0x3130_3050_4B4C_5353" in text  # one magic in both
