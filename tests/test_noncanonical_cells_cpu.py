"""Trace cells at or above p on the host: a 64-bit word w of a trace is the field element w mod p (include/starkhip.h), so the replays
of the trace checkers and air_eval_frame give, for a trace with p added to some of its small cells, what they give for the
canonical trace -- field by field, values and mask words included, in both layouts -- and that is what the CPU oracle says of the
canonical trace.  The inputs are alias_util's: only cells <= 2^32 - 2 have a second representative, and random traces hold none.
No GPU."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from alias_util import (ALL_SMALL_FLOOR, DIRECTED_VALUE, EDGES, GATE_CELLS, HAND_FLOOR, P, alias, assert_aliased, directed_blob, directed_traces,
                        gate_blob, gate_trace, hand_blob, hand_trace, hand_violating)
from bls_util import random_fp12
from check_report_util import Expected, assert_report
from free_cells_util import Expected as FreeExpected
from free_cells_util import assert_free_cells, assert_same

FULL = 1 << 20


def same_report(a, b):
    assert (a.violations, a.constraints_violated, a.rows_violated) == (b.violations, b.constraints_violated, b.rows_violated)
    for f in ("per_constraint", "row_mask", "rows", "list"):
        assert getattr(a, f).dtype == getattr(b, f).dtype and np.array_equal(getattr(a, f), getattr(b, f)), f


def replays_agree(air, blob, clean, aliased, pis, want=None, layouts=(0, 1), caps=(FULL, 3), canonical=None):
    """Both replays on `aliased` against themselves on `clean` and against the oracle's expectation for `clean`, in `layouts`.
    `canonical`: a dict that keeps the replays of `clean` for the next call with the same `clean`."""
    kept = aliased.copy()
    want = want or Expected(blob, clean, pis)  # asserts the oracle's own count of the canonical trace
    canonical = {} if canonical is None else canonical

    def of_clean(key, call):
        if key not in canonical:
            canonical[key] = call()
        return canonical[key]

    free = None
    for layout in layouts:
        c, a = (clean, aliased) if layout == 0 else (clean.T.copy(), aliased.T.copy())
        for cap in caps:
            got = S.check_trace_report_replay(air, a, pis, layout=layout, cap=cap)
            same_report(got, of_clean((layout, cap), lambda: S.check_trace_report_replay(air, c, pis, layout=layout, cap=cap)))
            assert_report(got, want, cap)
        fc = S.free_cells_replay(air, a, pis, layout=layout)
        assert_same(fc, of_clean((layout, "free"), lambda: S.free_cells_replay(air, c, pis, layout=layout)))
        if free is not None:
            assert_same(fc, free)
        free = fc
    assert np.array_equal(aliased, kept)  # the caller's buffer is left as it was
    return want, free


@functools.lru_cache(maxsize=None)
def hand_air():
    return S.register_air(hand_blob(), name="alias_hand")


@pytest.mark.parametrize("n", (8, 64))
@pytest.mark.parametrize("violating", (False, True), ids=("satisfying", "violating"))
def test_replays_on_the_hand_written_air(n, violating):
    trace, pis = hand_violating(n) if violating else hand_trace(n)
    for share, seed in ((1.0, 1), (0.6, 2)):  # everything that can be, and a mix of the two representatives inside one constraint
        aliased, count = alias(trace, share, seed)
        assert_aliased(aliased, trace, HAND_FLOOR, share, count)
        want, free = replays_agree(hand_air(), hand_blob(), trace, aliased, pis)
        if violating:
            assert want.constraints_violated >= 12 and want.not_applicable > 0
        else:
            assert want.violations == 0
        if n == 8:  # the rule itself, in plain Python, on the canonical trace
            assert_free_cells(free, FreeExpected(hand_blob(), trace, pis))


def test_the_hand_written_trace_holds_every_edge_in_every_free_column():
    trace, _ = hand_trace(8)
    for c in (0, 1, 3, 4, 5, 6, 7):
        assert sorted(int(x) for x in trace[:, c]) == sorted(EDGES)
    aliased, count = alias(trace, 1.0, 0)
    assert int(aliased.max()) == (1 << 64) - 1 and count >= 8 * 9  # the free columns, and the two a gate leaves free


@pytest.mark.parametrize("cell", GATE_CELLS)
def test_replays_on_a_complemented_gate(cell):
    """(1 - L0) (L1^2 - L1) with L1 = 5: (1 - cell) 20 on every row, whichever word holds the cell"""
    air = S.register_air(gate_blob(), name="alias_gate")
    clean = gate_trace(cell)
    gate_only = clean.copy()
    gate_only[:, 0] += np.uint64(P)
    everything, count = alias(clean, 1.0, 0)
    assert count == clean.size
    for aliased, floor in ((gate_only, ALL_SMALL_FLOOR), (everything, 1.0)):
        assert_aliased(aliased, clean, floor)
        want, _ = replays_agree(air, gate_blob(), clean, aliased, pis=np.zeros(0, dtype=np.uint64))
        assert want.violations == 8
        assert [int(v) for v in want.list[:, 2]] == [(1 - cell) * 20 % P] * 8


def test_replays_on_the_directed_rows():
    air = S.register_air(directed_blob(), name="alias_directed")
    aliased, clean = directed_traces()
    assert_aliased(aliased, clean, HAND_FLOOR)
    want, _ = replays_agree(air, directed_blob(), clean, aliased, pis=np.zeros(0, dtype=np.uint64))
    assert want.violations == 16 and all(int(v) == DIRECTED_VALUE for v in want.list[:, 2])


@functools.lru_cache(maxsize=None)
def fp12_mul():
    """(trace, the trace with one cell raised, public inputs, Expected of either) of a real FP12Mul trace, all of whose cells are small"""
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED7200), random_fp12(0x5EED7201))
    blob = S.air_program(S.AIR_FP12_MUL)
    for c in (0, 5, t.shape[1] // 7, t.shape[1] // 2):  # not every cell is constrained on every row: the first of these that is
        bad = t.copy()
        bad[9, c] += np.uint64(3)
        wants = (Expected(blob, t, pis), Expected(blob, bad, pis))
        if wants[1].violations > 0:
            break
    assert wants[0].violations == 0 and wants[1].violations > 0
    for a in (t, bad, pis):
        a.setflags(write=False)
    return t, bad, pis, wants, ({}, {})


@pytest.mark.parametrize("share", (1.0, 0.5, 0.05))
def test_replays_on_a_real_fp12_mul_trace(share):
    """16 rows x 60 285 columns, 82 560 constraints: the satisfying trace column-major, the violating one row-major, at every share
    (both layouts of both would take ten seconds a case; the replays of the canonical traces are shared between the cases)"""
    t, bad, pis, wants, canonical = fp12_mul()
    for trace, want, kept, layout in ((t, wants[0], canonical[0], 1), (bad, wants[1], canonical[1], 0)):
        aliased, count = alias(trace, share, int(share * 100))
        if share == 1.0:
            assert count == trace.size  # every cell of the trace has an alias
        assert_aliased(aliased, trace, ALL_SMALL_FLOOR, share, count)
        replays_agree(S.AIR_FP12_MUL, None, trace, aliased, pis, want, layouts=(layout,), caps=(FULL,), canonical=kept)


def _ext_rows(rng, base_rows, n_cols):
    """[n_cols, 2] extension elements: a trace row in the first component, edge values in the second"""
    out = np.zeros((n_cols, 2), dtype=np.uint64)
    out[:, 0] = base_rows
    out[:, 1] = [EDGES[int(i)] for i in rng.integers(0, len(EDGES), size=n_cols)]
    return out


@pytest.mark.parametrize("which", ("hand", "gate", "directed"))
def test_air_eval_frame_reads_cells_mod_p(which):
    """The verifier's evaluator over the quadratic extension (the only one starkhip_air_eval_frame reaches; the base-field
    instantiation of the same template is fed by the library alone): aliased local / next rows, in either component, fold to what the
    canonical rows fold to, and on base-field rows to the oracle's constraint values folded by hand."""
    rng = np.random.default_rng(17)
    if which == "hand":
        blob, (trace, pis) = hand_blob(), hand_violating(8)
    elif which == "gate":
        blob, trace, pis = gate_blob(), np.array([[c, 5] for c in GATE_CELLS], dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    else:
        blob, trace, pis = directed_blob(), directed_traces()[1], np.zeros(0, dtype=np.uint64)
    air = S.register_air(blob, name="alias_" + which)
    n, n_cols = trace.shape
    masks = rng.integers(1, P, size=(4, 2), dtype=np.uint64)
    alphas = rng.integers(1, P, size=(2, 2), dtype=np.uint64)
    for r in range(min(n, 4)):
        local, nxt = _ext_rows(rng, trace[r], n_cols), _ext_rows(rng, trace[(r + 1) % n], n_cols)
        want = S.air_eval_frame(air, local, nxt, pis, masks, alphas)
        for share, seed in ((1.0, r), (0.5, 100 + r)):
            (la, ca), (na, cb) = alias(local, share, seed), alias(nxt, share, seed + 50)
            assert_aliased(np.concatenate([la, na]), np.concatenate([local, nxt]), HAND_FLOOR, share, ca + cb)
            assert np.array_equal(S.air_eval_frame(air, la, na, pis, masks, alphas), want), (r, share)
    # base-field rows under base-field masks and alphas: the plain fold of the oracle's values
    one = np.array([[1, 0]] * 4, dtype=np.uint64)
    alpha = int(rng.integers(1, P, dtype=np.uint64))
    local, nxt = np.zeros((n_cols, 2), dtype=np.uint64), np.zeros((n_cols, 2), dtype=np.uint64)
    local[:, 0], nxt[:, 0] = trace[0], trace[1 % n]
    acc = 0
    for v in O.eval_frame(blob, trace[0], trace[1 % n], pis, [1, 1, 1, 1]):
        acc = (acc * alpha + int(v)) % P
    la, na = alias(local, 1.0, 0)[0], alias(nxt, 1.0, 0)[0]
    assert_aliased(np.concatenate([la, na]), np.concatenate([local, nxt]), ALL_SMALL_FLOOR)  # the second components are zero
    got = S.air_eval_frame(air, la, na, pis, one, np.array([[alpha, 0]], dtype=np.uint64))
    assert [int(x) for x in got[0]] == [acc, 0]
