"""Every device form of the Poseidon permutation -- the generic loop and the quad, row, lane and pair forms of the leaf hash, with the
capacity-only last rounds the leaf kernels use -- on boundary states at every round (tests/poseidon_steer.py steers them there by
inverting the rounds; tests/test_poseidon_steering_cpu.py shows the helper right), at every position of a wave and with partly
filled last waves.  Prover.poseidon_permute_batch(states, form, variant) runs the very functions the leaf kernels call on whole
12-word states.  Every comparison is equality of integers against the permutation in Python integers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import poseidon_steer as PS
import starky_bls12_381_amd as S

pytestmark = pytest.mark.gpu
P = S.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORM_NAMES = {0: "generic", 1: "quad", 2: "row", 3: "lane", 4: "pair"}
FORM_VARIANTS = [(0, 0), (1, 0), (1, 1), (2, 0), (3, 0), (3, 1), (4, 0), (4, 1)]
# the words a variant is specified to produce (include/starkhip.h); the others come back as they went in
CAP = [8, 9, 10, 11]
SPECIFIED = {(1, 1): CAP, (3, 1): CAP, (4, 1): [2, 3, 4, 5] + CAP}
ROTATIONS = [0, 1, 2, 3, 5, 9, 17, 33]      # every residue mod 4 (states per wave of the row form), then other places mod 16, 32 and 64
BATCH_SIZES = [1, 31, 32, 33, 63, 64, 65, 1000]
WINDOWS = [0, 1487, 4013]                   # where in the steered part a short batch starts


def lanes_of(form, i):
    """where state i of a batch sits"""
    if form == 1:
        return "block %d wave %d lanes %d..%d" % (i // 64, i % 64 // 16, 4 * (i % 16), 4 * (i % 16) + 3)
    if form == 2:
        return "block %d wave %d lanes %d..%d" % (i // 16, i % 16 // 4, 16 * (i % 4), 16 * (i % 4) + 15)
    if form == 4:
        return "block %d wave %d lanes %d and %d" % (i // 128, i % 128 // 32, i % 32, i % 32 + 32)
    return "block %d lane %d" % ((i // 256, i % 256) if form == 3 else (i // 64, i % 64))


@pytest.fixture(scope="module")
def steering():
    cases = PS.steering_set()
    return cases, np.array([c.state for c in cases], dtype=np.uint64), np.array(PS.expected_outputs(), dtype=np.uint64)


def check_batch(prover, form, variant, cases, states, want, what):
    got = prover.poseidon_permute_batch(states, form, variant)
    words = SPECIFIED.get((form, variant), list(range(12)))
    rest = [w for w in range(12) if w not in words]
    bad = np.flatnonzero((got[:, words] != want[:, words]).any(axis=1) | (got[:, rest] != states[:, rest]).any(axis=1))
    if bad.size:
        i = int(bad[0])
        wrong = [w for w in range(12) if got[i, w] != (want[i, w] if w in words else states[i, w])]
        raise AssertionError("%s form, variant %d, %s: %d of %d states differ; the first is state %d (%s): %r, target %s; words %s: got %s, want %s" % (
            FORM_NAMES[form], variant, what, bad.size, len(cases), i, lanes_of(form, i), cases[i],
            None if cases[i].target is None else [hex(x) for x in cases[i].target], wrong, [hex(int(got[i, w])) for w in wrong],
            [hex(int(want[i, w] if w in words else states[i, w])) for w in wrong]))


@pytest.mark.parametrize("form,variant", FORM_VARIANTS)
def test_form_on_the_whole_steering_set_at_every_lane_position(prover, steering, form, variant):
    cases, states, want = steering
    n = len(cases)
    assert n % 256 != 0
    for rot in ROTATIONS:
        idx = (np.arange(n) + rot) % n
        check_batch(prover, form, variant, [cases[i] for i in idx], states[idx], want[idx], "set rotated by %d" % rot)


@pytest.mark.parametrize("form,variant", FORM_VARIANTS)
def test_form_with_partly_shadowed_last_waves(prover, steering, form, variant):
    cases, states, want = steering
    for n in BATCH_SIZES:
        for start in WINDOWS:
            sl = slice(start, start + n)
            check_batch(prover, form, variant, cases[sl], states[sl], want[sl], "batch of %d from state %d" % (n, start))


def test_a_wrong_word_is_reported_with_its_round_site_pattern_and_lanes(prover, steering):
    """the comparison bites and says where: one word of one expected state changed, in the form whose states span lanes l and l + 32"""
    cases, states, want = steering
    i = next(k for k, c in enumerate(cases) if c.rnd == 17 and c.site == "sbox_in" and c.pattern == "12 x 0xffffffff")
    sl = slice(i - 37, i + 30)
    wrong = want[sl].copy()
    wrong[37, 9] ^= np.uint64(1)
    with pytest.raises(AssertionError, match=r"pair form, variant 1, .*1 of 67 states differ; the first is state 37 \(block 0 wave 1 lanes 5 and 37\): "
                                             r"round 17 sbox_in, 12 x 0xffffffff, .*words \[9\]"):
        check_batch(prover, 4, 1, cases[sl], states[sl], wrong, "one expected word changed")
    wrong[37, 0] ^= np.uint64(1)     # a word the capacity-only variant does not specify is compared with the input instead
    wrong[37, 9] ^= np.uint64(1)
    check_batch(prover, 4, 1, cases[sl], states[sl], wrong, "an unspecified word of the expectation changed")
    with pytest.raises(AssertionError, match=r"pair form, variant 0, .*words \[0\]"):
        check_batch(prover, 4, 0, cases[sl], states[sl], wrong, "the same for the full permutation")


def test_bad_form_or_variant_is_refused_and_the_prover_stays_usable(prover, steering):
    cases, states, want = steering
    for form, variant in ((5, 0), (-1, 0), (0, 1), (2, 1), (1, 2), (3, 2), (4, 2), (3, -1), (7, 7)):
        with pytest.raises(S.StarkhipError):
            prover.poseidon_permute_batch(states[:4], form, variant)
    for form, variant in FORM_VARIANTS:
        check_batch(prover, form, variant, cases[:70], states[:70], want[:70], "after the refusals")
    assert prover.poseidon_permute_batch(states[:0], 3, 0).shape == (0, 12)


@pytest.mark.parametrize("ncols", [8, 9, 13, 24])
@pytest.mark.parametrize("form", [2, 1, 3, 4])
def test_merkle_cap_with_round_0_steered_leaves(prover, form, ncols):
    """The sponge paths: a leaf form's first permutation has capacity 0, so its round 0 can still be steered through a commitment.  Leaf j
    starts with the eight rate words  v - rc[0][e]  for v = the steering values in turn: after the first round's constants every rate
    S-box sees v.  Against the oracle's cap, as test_merkle_cap_in_both_leaf_hash_forms compares."""
    log_N = 7
    rng = np.random.default_rng(300 + ncols)
    mat = rng.integers(0, P, size=(ncols, 1 << log_N), dtype=np.uint64)
    for j in range(1 << log_N):
        v = PS.VALUES[j % len(PS.VALUES)]
        for e in range(8):
            mat[e, j] = (v - PS.RC[0][e]) % P
    prover.set_option("leaf_hash_form", form)
    try:
        cap = prover.merkle_cap(mat, 2)
    finally:
        prover.set_option("leaf_hash_form", 0)
    assert np.array_equal(cap, O.merkle_cap(np.ascontiguousarray(mat.T), 2))


# One fresh process: for the quad form and then the row form, the permutation entry and a commitment in that form, in the order
# given.  The quad form's two entries read two constant-memory symbols of one type (kernels_hash.hip, kernels_hash_quad_form.hip); the row
# form's read one.  64 leaves x 9 columns: one full block and a remainder of one, in a part-filled last wave.
UPLOAD_ORDER_CHILD = """
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np
import oracle_lib as O
import starky_bls12_381_amd as S
rng = np.random.default_rng(0x0DE2)
states = rng.integers(0, S.P, size=(5, 12), dtype=np.uint64)
want = np.array([S.poseidon_permute_host(s) for s in states])
mat = rng.integers(0, S.P, size=(9, 64), dtype=np.uint64)
want_cap = O.merkle_cap(np.ascontiguousarray(mat.T), 2)
pv = S.Prover(0)
def permute(form):
    assert np.array_equal(pv.poseidon_permute_batch(states, form, 0), want), ("permutation", form)
def commit(form):
    pv.set_option("leaf_hash_form", form)
    try:
        cap = pv.merkle_cap(mat, 2)
    finally:
        pv.set_option("leaf_hash_form", 0)
    assert np.array_equal(cap, want_cap), ("cap", form)
for form in (1, 2):
    for step in %(order)s:
        step(form)
pv.close()
print("upload order ok")
"""


def test_each_table_is_uploaded_before_its_first_use_whichever_entry_comes_first():
    """Each constant-memory table is uploaded by the first launch that reads it, and by every entry that can be that launch: in a fresh
    process (the suite's own order would have uploaded everything long before), the permutation entry before the commitment and the
    other way round.  Against the host permutation and the oracle's cap."""
    for order in ("(permute, commit)", "(commit, permute)"):
        r = subprocess.run([sys.executable, "-c", UPLOAD_ORDER_CHILD % {"root": ROOT, "order": order}], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "upload order ok" in r.stdout, order + "\n" + r.stdout[-2000:] + r.stderr[-4000:]
