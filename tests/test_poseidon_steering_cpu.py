"""Boundary states at every round of the Poseidon permutation, without a GPU (tests/poseidon_steer.py makes them by inverting the
rounds): first the helper is shown right, then the host permutations -- the challenger's AVX-512 one and the portable loop -- run
the whole steering set, and the generated asm blocks of the row, lane and pair forms run, in the generators' interpreter, the
steered states of exactly the rounds they implement.  Every comparison is equality of integers.
tests/test_gpu_poseidon_forms.py runs the same set through the device's forms."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as O
import poseidon_steer as PS
import starky_bls12_381_amd as S

import gen_lane_round_asm as L   # (tools/ is on the path: poseidon_steer put it there)
import gen_pair_round_asm as Q
import gen_row_round_asm as G

P = PS.P


def as_array(states):
    return np.array(states, dtype=np.uint64).reshape(-1, 12)


# ---------------------------------------------------------------- the helper is right before it judges anything
def test_python_permutation_equals_the_oracle():
    rng = np.random.default_rng(21)
    states = [[0] * 12, list(range(12)), [P - 1] * 12] + [[v] * 12 for v in PS.VALUES] + [[int(x) for x in rng.integers(0, P, size=12, dtype=np.uint64)] for _ in range(300)]
    for s in states:
        assert PS.forward(s) == [int(x) for x in O.poseidon_permute(as_array(s)[0])], s


def test_inverse_undoes_forward():
    rng = np.random.default_rng(22)
    for s in [[0] * 12, [P - 1] * 12] + [[int(x) for x in rng.integers(0, P, size=12, dtype=np.uint64)] for _ in range(100)]:
        assert PS.inverse(PS.forward(s)) == s and PS.forward(PS.inverse(s)) == s
    for r in range(PS.ROUNDS):
        assert PS.inverse_round(PS.forward_round(s, r), r) == s
    assert PS.matvec(PS.MDS, PS.matvec(PS.MDS_INV, list(range(1, 13)))) == list(range(1, 13))


def test_the_steering_set_has_every_pattern_at_every_round():
    cases = PS.steering_set()
    per_site = len(PS.VALUES) + 12 * len(PS.POSITION_VALUES) + PS.MIXED_PER_SITE
    steered = [c for c in cases if c.rnd is not None]
    assert len(steered) == PS.ROUNDS * 2 * per_site == 4560 and len(cases) == 4560 + 3 + PS.RANDOM_STATES
    for rnd in range(PS.ROUNDS):
        for site in PS.SITES:
            here = [c for c in steered if c.rnd == rnd and c.site == site]
            assert [c.target for c in here[:len(PS.VALUES)]] == [[v] * 12 for v in PS.VALUES]
            for pos in range(12):
                for v in PS.POSITION_VALUES:
                    assert any(c.target[pos] == v and c.pattern.startswith("word %d " % pos) for c in here)
    assert all(len(c.state) == 12 and all(0 <= x < P for x in c.state) for c in cases)
    assert PS.steering_set() is cases and [c.state for c in cases[:50]] == [c.state for c in PS.steering_set.__wrapped__()[:50]]   # fixed and seeded


def test_every_steered_input_shows_its_target_at_its_round_and_site():
    """the condition that keeps the set honest: all of it, no skips"""
    checked = 0
    for c in PS.steering_set():
        if c.rnd is not None:
            assert PS.site_of(c.state, c.rnd, c.site) == c.target, c
            checked += 1
    assert checked == 4560


# ---------------------------------------------------------------- the host permutations on the whole set
def test_host_permutations_on_the_whole_steering_set():
    cases, want = PS.steering_set(), PS.expected_outputs()
    many = S.lib.starkhip_poseidon_permute_host_many
    many.argtypes, many.restype = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_int], None
    for c, w in zip(cases, want):
        assert [int(x) for x in S.poseidon_permute_host(as_array(c.state)[0])] == list(w), ("host permutation (AVX-512, partial4)", c)
        s = as_array(c.state)[0].copy()
        many(s.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1, 1)
        assert [int(x) for x in s] == list(w), ("portable loop", c)


# ---------------------------------------------------------------- the generated blocks on the steered states of their rounds
@functools.lru_cache(maxsize=None)
def sbox_in_traces():
    """per steered case: the words entering the S-boxes of rounds 0 .. its round (a block's entry state: its round's constants added)"""
    out = []
    for c in PS.steering_set():
        if c.rnd is None:
            continue
        s, trace = list(c.state), []
        for r in range(c.rnd + 1):
            sbox_in, _, s = PS.round_sites(s, r)
            trace.append(sbox_in)
        out.append((c, trace))
    return out


def constants_after(r):
    return PS.RC[r + 1] if r + 1 < PS.ROUNDS else [0] * 12   # the forms seed the last layer with zeros


def block_cases(first, count):
    """(entry state, following constants) of every steered case whose round lies in first .. first + count - 1, for a block that takes
    the state at round `first` (constants added) through `count` rounds with the shipped constants"""
    out = []
    for c, trace in sbox_in_traces():
        if first <= c.rnd < first + count:
            cs = [constants_after(r) for r in range(first, first + count)]
            out.append((trace[first], cs[0] if count == 1 else cs))
    return out


def cases_of_rounds(rounds, count=1):
    out = [x for r in rounds for x in block_cases(r, count)]
    assert len(out) == 152 * count * len(rounds)    # every steered state of those rounds, both sites
    return out


FULL_ROUNDS, PLAIN_PARTIAL = [0, 1, 2, 3, 26, 27, 28, 29], [24, 25]
FOURS, TRIPLES = [4, 8, 12, 16, 20], [4, 7, 10, 13, 16, 19, 22]


def test_row_form_blocks_on_steered_round_entries():
    """poseidon_permute_row_merged_asm: full rounds 0 .. 3 and 26 .. 29, seven merged triples from round 4, the plain partial round 25"""
    full, partial, triple = (G.AB.schedule(b(), G.HAZARDS) for b in (G.block_full, G.block_partial, G.block_triple))
    G.test(full, False, cases_of_rounds(FULL_ROUNDS))
    G.test(partial, True, cases_of_rounds([25]))
    G.test_triple(triple, cases_of_rounds(TRIPLES, 3))


def test_lane_form_blocks_on_steered_round_entries():
    """poseidon_permute_lane_asm: matrix-pipe full rounds 0 .. 3 and 26 .. 28, five merged fours from round 4, matrix-pipe partial rounds
    24 and 25, and round 29 as the multiply-add block, whole and capacity-only"""
    L.test_round_mfma(L.schedule(L.block_full_mfma()), False, cases=cases_of_rounds(FULL_ROUNDS[:-1]))
    L.test_four(L.schedule(L.block_four()), cases_of_rounds(FOURS, 4))
    L.test_round_mfma(L.schedule(L.block_partial_mfma()), True, cases=cases_of_rounds(PLAIN_PARTIAL))
    L.test_round(L.schedule(L.block_full()), False, cases=cases_of_rounds([29]))
    L.test_round(L.schedule(L.block_full(8)), False, 8, cases=cases_of_rounds([29]))


def test_pair_form_blocks_on_steered_round_entries():
    """poseidon_permute_pair_asm: full rounds 0 .. 3 and 26 .. 29 (the last one also capacity-only), five merged fours, partial rounds 24, 25"""
    Q.test_round_pair(Q.schedule_pair(Q.block_full_pair(), Q.ROUND_LOAD_LATENCY), False, cases=cases_of_rounds(FULL_ROUNDS))
    Q.test_round_pair(Q.schedule_pair(Q.block_full_pair(2), Q.ROUND_LOAD_LATENCY), False, 2, cases=cases_of_rounds([29]))
    Q.test_round_pair(Q.schedule_pair(Q.block_partial_pair(), Q.ROUND_LOAD_LATENCY), True, cases=cases_of_rounds(PLAIN_PARTIAL))
    Q.test_four_pair(Q.schedule_pair(Q.block_four_pair(), Q.FOUR_LOAD_LATENCY), cases_of_rounds(FOURS, 4))


def test_block_testers_reject_a_wrong_result_on_steered_cases():
    """the cases really reach the testers' assertions: the right block against constants that are not the ones it was given fails"""
    cases = cases_of_rounds([29])[:3]
    order = L.schedule(L.block_full())
    L.test_round(order, False, cases=cases)
    with pytest.raises(AssertionError):
        L.test_round(order, True, cases=cases)    # judged as a partial round
