"""Constraint classes of the quotient (csrc/quotient_plan.h): a constraint with d cell factors is evaluated on max(1, d - 1) cosets of
n points (d for first-row and last-row constraints) instead of all 2^qdb, and the classes' values are recombined into the quotient's
coefficient chunks.  Host only: the class rule against degrees multiplied out in Python, the per-class plans through the host replay
of the kernel's record streams, and the recombination in Python integers with the library's constants."""
import numpy as np
import pytest

import air_blob as AB
import starky_bls12_381_amd as S
from quotient_classes_util import P, class_air, class_by_degrees, quotient_chunks
from random_air import random_air
from starky_bls12_381_amd.air_builder import AirBuilder


def _every_kind_and_degree_air():
    """One constraint of every (kind, d) an AIR of degree 5 may hold, d split into every (gates, longest monomial) the program allows."""
    b = AirBuilder(16, 1, 5)
    want = []
    for kind, emit in enumerate((b.constraint, b.transition, b.first_row, b.last_row)):
        for d in range(1, 6 if kind < 2 else 5):
            for gates in range(0, min(4, d - 1) + 1):
                mono = d - gates
                if mono > 3:
                    continue
                body = b.L(9)
                for f in range(1, mono):
                    body = body * b.L(9 + f)
                e = b.N(8) - body if mono > 1 else (b.N(8) - b.L(9) - b.PI(0))
                for gi in range(gates):
                    e = (b.L(gi) if gi % 2 == 0 else (1 - b.L(gi))) * e
                emit(e)
                want.append((kind, d))
    return b.finish(), want


def test_class_rule_is_the_degree_bound_for_every_kind_and_degree():
    blob, made = _every_kind_and_degree_air()
    air = S.register_air(blob)
    got = S.quotient_classes(air)
    cons = list(AB.constraints(AB.parse_blob(blob)))
    assert len(cons) == len(made) == got.size
    seen = set()
    for (kind, gates, terms), (mkind, d), cls in zip(cons, made, got):
        assert kind == mkind
        assert len(gates) + max(len(cells) for _, _, cells in terms) == d
        assert int(cls) == class_by_degrees(kind, gates, terms) == (max(1, d - 1) if kind < 2 else d)
        seen.add((kind, d))
    assert seen == {(k, d) for k in range(4) for d in range(1, 6 if k < 2 else 5)}
    assert set(int(c) for c in got) == {1, 2, 3, 4}


def _random_degree_5():
    blob, _, _ = random_air(6, 130, 5, 256)
    return S.register_air(blob)


@pytest.mark.parametrize("which", ["fp12_mul", "ecc_aggregate", "random_degree_5"])
@pytest.mark.parametrize("chunks", [1, 6, 64])
def test_per_class_plans_replay_to_the_fold_restricted_to_the_class(which, chunks):
    air = {"fp12_mul": lambda: S.AIR_FP12_MUL, "ecc_aggregate": lambda: S.AIR_ECC_AGGREGATE, "random_degree_5": _random_degree_5}[which]()
    # the entry itself replays the plan of every coset: its sums per class are the plain fold restricted to that class for the classes
    # above the coset and zero for the others, and the classes add up to the whole fold
    st = S.quotient_class_plan_check(air, chunks, seed=0xC1A55 + chunks)
    degree = S.air_constraint_degree(air)
    assert st["classes"] == max(1, degree - 1) and st["cosets"] == 1 << (st["classes"] - 1).bit_length()
    cls = S.quotient_classes(air)
    assert st["class_constraints"] == [int((cls == k).sum()) for k in range(1, st["classes"] + 1)]
    assert sum(st["class_constraints"]) == S.air_num_constraints(air)
    assert sum(st["coset_chunks"]) == st["chunks"] == st["work_rows"]
    for t in range(st["cosets"]):  # a coset has work exactly when a class above it has a constraint; a spare coset runs them all
        above = sum(st["class_constraints"][t:]) if t < st["classes"] else sum(st["class_constraints"])
        assert (st["coset_chunks"][t] > 0) == (above > 0)
        assert st["coset_chunks"][t] <= max(1, chunks)
    assert st["coset_chunks"][:st["classes"]] == sorted(st["coset_chunks"][:st["classes"]], reverse=True)  # lighter cosets: fewer chunks
    assert st["contributions"] >= S.quotient_plan_check(air, 1)["contributions"]


@pytest.mark.parametrize("n", [16, 64])
def test_recombined_chunks_equal_the_inverse_transform_of_all_values(n):
    blob, trace, pis = class_air(n)
    air = S.register_air(blob)
    cls = S.quotient_classes(air)
    kinds = [kind for kind, _, _ in AB.constraints(AB.parse_blob(blob))]
    assert {(k, int(c)) for k, c in zip(kinds, cls)} == {(k, c) for k in range(4) for c in range(1, 5)}  # every kind in every class
    want, got = quotient_chunks(blob, trace, pis, cls, 2, 0x1234567890ABCDEF % P, S.quotient_solve_table(n.bit_length() - 1, 2))
    assert want == got
    assert any(want[3])  # the top chunk is in use: nothing above the degree bound was dropped


def test_empty_top_classes_leave_their_cosets_without_work():
    n = 16
    blob, trace, pis = class_air(n, top=2, degree=5)
    air = S.register_air(blob)
    cls = S.quotient_classes(air)
    assert set(int(c) for c in cls) == {1, 2}
    st = S.quotient_class_plan_check(air, 8, seed=3)
    assert st["classes"] == st["cosets"] == 4
    assert st["coset_chunks"][2:] == [0, 0] and st["coset_chunks"][0] >= st["coset_chunks"][1] > 0
    want, got = quotient_chunks(blob, trace, pis, cls, 2, 0xFEDCBA9876543 % P, S.quotient_solve_table(4, 2))
    assert want == got
    assert not any(want[2]) and not any(want[3]) and any(want[1])
