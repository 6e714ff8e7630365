"""What starkhip_check_trace_report must say about a trace, built from the CPU oracle alone: oracle_eval_frame with masks
[1, 1, 1, 1] gives the mask-free value of every constraint on a frame, the kinds come from the program blob.  Test code."""
import functools

import numpy as np

import air_blob
import oracle_lib as O
import starky_bls12_381_amd as S
from random_air import CASES, random_air

P = 0xFFFFFFFF00000001
PLAIN, TRANSITION, FIRST, LAST = range(4)


class Expected:
    def __init__(self, blob, trace, pis):
        n = trace.shape[0]
        kinds = np.array([k for k, _, _ in air_blob.constraints(air_blob.parse_blob(blob))])
        values = np.array([O.eval_frame(blob, trace[r], trace[(r + 1) % n], pis, [1, 1, 1, 1]) for r in range(n)], dtype=np.uint64)  # [n][K]
        assert values.shape == (n, kinds.size)
        row = np.arange(n)[:, None]
        applies = ((kinds == PLAIN) | ((kinds == TRANSITION) & (row < n - 1)) | ((kinds == FIRST) & (row == 0)) | ((kinds == LAST) & (row == n - 1)))
        bad = applies & (values != 0)
        self.not_applicable = int(((values != 0) & ~applies).sum())  # nonzero, but off the rows of their kind
        self.per_constraint = bad.sum(axis=0).astype(np.uint32)
        self.rows = np.flatnonzero(bad.any(axis=1))
        self.violations = int(bad.sum())
        self.constraints_violated = int((self.per_constraint != 0).sum())
        ks, rs = np.nonzero(bad.T)  # constraint ascending, then row ascending
        self.list = np.stack([ks.astype(np.uint64), rs.astype(np.uint64), values[rs, ks]], axis=1) if ks.size else np.zeros((0, 3), dtype=np.uint64)
        self.row_mask = np.zeros((n + 63) // 64, dtype=np.uint64)
        for r in self.rows:
            self.row_mask[r >> 6] |= np.uint64(1 << (int(r) & 63))
        # the expectation is itself checked: the oracle's own checker counts the same pairs
        assert O.check_trace(blob, trace, pis)[0] == self.violations

    def cuts_inside_a_constraint(self, cap):
        """A list of `cap` entries ends between two rows of one constraint."""
        return 0 < cap < self.violations and self.list[cap - 1][0] == self.list[cap][0]


def assert_report(rep, want, cap):
    assert (rep.violations, rep.constraints_violated, rep.rows_violated) == (want.violations, want.constraints_violated, len(want.rows))
    assert rep.per_constraint.dtype == np.uint32 and np.array_equal(rep.per_constraint, want.per_constraint)
    assert rep.row_mask.dtype == np.uint64 and np.array_equal(rep.row_mask, want.row_mask)
    assert np.array_equal(rep.rows, want.rows)
    assert rep.list.dtype == np.uint64 and rep.list.shape == (min(cap, want.violations), 3)
    assert np.array_equal(rep.list, want.list[:cap])


def corrupt(trace):
    """Row rows // 2 and column cols // 2, every cell plus one."""
    bad = trace.copy()
    n, c = bad.shape
    bump = lambda x: np.where(x == np.uint64(P - 1), np.uint64(0), x + np.uint64(1))
    bad[n // 2] = bump(bad[n // 2])
    bad[:, c // 2] = bump(bad[:, c // 2])
    return bad


@functools.lru_cache(maxsize=None)
def case(i):
    """(blob, trace, corrupted trace, public inputs, Expected of the corrupted trace) of random_air.CASES[i]; shared, read-only."""
    seed, cols, degree, rows = CASES[i]
    blob, trace, pis = random_air(seed, cols, degree, rows)
    bad = corrupt(trace)
    want = Expected(blob, bad, pis)
    for a in (blob, trace, bad, pis):
        a.setflags(write=False)
    if i >= 1:  # the corruption is one a checker can get wrong: several constraints, and for seeds 5-7 one spread over several waves
        assert want.constraints_violated > 1 and want.not_applicable > 0
    if i >= 4:
        assert want.per_constraint.max() >= 128
    return blob, trace, bad, pis, want


# ---- the replay's checks per case, shared by test_check_report_cpu.py and test_trace_check_report_one_column_cpu.py
FULL = 1 << 20


def check_clean(air, i):
    _, trace, _, pis, _ = case(i)
    for layout, t in ((0, trace), (1, trace.T.copy())):
        rep = S.check_trace_report_replay(air, t, pis, layout=layout, cap=FULL)
        assert (rep.violations, rep.constraints_violated, rep.rows_violated) == (0, 0, 0)
        assert not rep.per_constraint.any() and rep.per_constraint.size == S.air_num_constraints(air)
        assert not rep.row_mask.any() and rep.row_mask.size == (trace.shape[0] + 63) // 64
        assert rep.rows.size == 0 and rep.list.shape == (0, 3)


def check_corrupted(air, i):
    _, _, bad, pis, want = case(i)
    assert want.violations > 0
    assert_report(S.check_trace_report_replay(air, bad, pis, cap=FULL), want, FULL)
    assert_report(S.check_trace_report_replay(air, bad.T.copy(), pis, layout=1, cap=FULL), want, FULL)
    if bad.shape[0] < 64:  # one mask word, and only its low bits can be set
        assert int(S.check_trace_report_replay(air, bad, pis).row_mask[0]) >> bad.shape[0] == 0


def check_caps(air, i):
    _, _, bad, pis, want = case(i)
    total = want.violations
    for cap in (0, 1, 7, total - 1, total, total + 5):
        assert_report(S.check_trace_report_replay(air, bad, pis, cap=cap), want, cap)
