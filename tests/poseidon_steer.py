"""Preimage steering for the Poseidon permutation, in plain Python integers.

Poseidon is a permutation, so any state can be placed at any round of it exactly: choose the twelve words that shall enter the
S-boxes (or the linear layer) of round r, invert rounds r - 1 .. 0, and the result is the canonical input that reaches them.  The
tests use this to put boundary values (0, p - 1, 2^32 - 1, 2^32, ...) in front of every round of every implementation, which a sponge
cannot do: its capacity words are fixed, so its inputs shape round 0 and nothing after it.

Only CANONICAL values can be steered.  An implementation that keeps lazily reduced words holds SOME 64-bit representative of the
steered value in its registers; which one is the implementation's business.

Reads only this repository: the round constants from csrc/poseidon_consts.h, the circulant and the diagonal as tools/asm_blocks.py
has them (CIRC, mds_coef).
"""
import functools
import os
import random
import re
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_blocks as AB  # noqa: E402

P = AB.P
ROUNDS, HALF_FULL = 30, 4
RC_FLAT = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{16})ULL", open(os.path.join(ROOT, "starky_bls12_381_amd", "csrc", "poseidon_consts.h")).read())]
assert len(RC_FLAT) == 12 * ROUNDS and all(c < P for c in RC_FLAT)
RC = [RC_FLAT[12 * r:12 * r + 12] for r in range(ROUNDS)]
MDS = [[AB.mds_coef(i, j) for j in range(12)] for i in range(12)]
SBOX_INV_EXP = pow(7, -1, P - 1)
SITES = ("sbox_in", "layer_in")


def is_partial(r):
    return HALF_FULL <= r < ROUNDS - HALF_FULL


def _inverse_matrix(m):
    n = len(m)
    a = [[x % P for x in row] + [1 if i == j else 0 for j in range(n)] for i, row in enumerate(m)]
    for c in range(n):
        piv = next(r for r in range(c, n) if a[r][c])
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], -1, P)
        a[c] = [x * inv % P for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(x - f * y) % P for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


MDS_INV = _inverse_matrix(MDS)


def matvec(m, s):
    return [sum(c * x for c, x in zip(row, s)) % P for row in m]


def sbox_layer(s, r):
    return [pow(s[0], 7, P)] + list(s[1:]) if is_partial(r) else [pow(x, 7, P) for x in s]


def sbox_layer_inverse(s, r):
    return [pow(s[0], SBOX_INV_EXP, P)] + list(s[1:]) if is_partial(r) else [pow(x, SBOX_INV_EXP, P) for x in s]


def round_sites(state, r):
    """(the words entering the S-boxes of round r, the words entering its linear layer, the state after it) for the state before it"""
    sbox_in = [(x + c) % P for x, c in zip(state, RC[r])]
    layer_in = sbox_layer(sbox_in, r)
    return sbox_in, layer_in, matvec(MDS, layer_in)


def forward_round(state, r):
    return round_sites(state, r)[2]


def inverse_round(state, r):
    return [(x - c) % P for x, c in zip(sbox_layer_inverse(matvec(MDS_INV, state), r), RC[r])]


def forward(state, first=0, end=ROUNDS):
    s = [int(x) for x in state]
    for r in range(first, end):
        s = forward_round(s, r)
    return s


def inverse(state):
    s = [int(x) for x in state]
    for r in reversed(range(ROUNDS)):
        s = inverse_round(s, r)
    return s


def steer(rnd, site, target):
    """the canonical input state whose forward run shows `target` (twelve canonical words) at `site` of round `rnd`:
    sbox_in   the words entering the S-boxes of that round, after its constants (in a partial round only word 0 passes an S-box; the
              other eleven are steered all the same);
    layer_in  the words entering the linear layer of that round."""
    assert site in SITES and 0 <= rnd < ROUNDS and len(target) == 12 and all(0 <= x < P for x in target)
    s = list(target) if site == "sbox_in" else sbox_layer_inverse(target, rnd)
    s = [(x - c) % P for x, c in zip(s, RC[rnd])]
    for r in reversed(range(rnd)):
        s = inverse_round(s, r)
    return s


def site_of(state, rnd, site):
    """what the forward run of `state` shows at `site` of round `rnd`"""
    return round_sites(forward(state, 0, rnd), rnd)[SITES.index(site)]


# ---------------------------------------------------------------- the steering set
VALUES = [0, 1, 2, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, P - 2, P - 1, 0xFFFFFFFE00000001, 0x00000001FFFFFFFF]
POSITION_VALUES = [0, P - 1, (1 << 32) - 1, 1 << 32]
MIXED_PER_SITE = 16
RANDOM_STATES = 3000
SEED = 0x57EE12


class Case:
    """one state of the set: `state` (the input), where it was steered to (rnd, site; None for the plain inputs), the target there
    and a name of the pattern for assertion messages"""

    def __init__(self, state, rnd, site, target, pattern):
        self.state, self.rnd, self.site, self.target, self.pattern = state, rnd, site, target, pattern

    def __repr__(self):
        return "round %s %s, %s" % (self.rnd, self.site, self.pattern)


def targets(rng):
    """the (pattern, target) list of ONE round and site: twelve of a kind for every value, every position set to each position value
    among random words, and states with every word drawn from the values"""
    out = [("12 x %#x" % v, [v] * 12) for v in VALUES]
    for pos in range(12):
        for v in POSITION_VALUES:
            t = [rng.randrange(P) for _ in range(12)]
            t[pos] = v
            out.append(("word %d = %#x among random words" % (pos, v), t))
    for k in range(MIXED_PER_SITE):
        out.append(("boundary mix %d" % k, [rng.choice(VALUES) for _ in range(12)]))
    return out


@functools.lru_cache(maxsize=None)
def steering_set():
    """the fixed, seeded set: for every round and both sites the targets above, steered; then the all-zero, 0 .. 11 and all-(p - 1)
    inputs and RANDOM_STATES plain random ones"""
    rng = random.Random(SEED)
    cases = []
    for rnd in range(ROUNDS):
        for site in SITES:
            for pattern, t in targets(rng):
                cases.append(Case(steer(rnd, site, t), rnd, site, t, pattern))
    cases.append(Case([0] * 12, None, None, None, "input 12 x 0"))
    cases.append(Case(list(range(12)), None, None, None, "input 0 .. 11"))
    cases.append(Case([P - 1] * 12, None, None, None, "input 12 x (p - 1)"))
    for k in range(RANDOM_STATES):
        cases.append(Case([rng.randrange(P) for _ in range(12)], None, None, None, "random input %d" % k))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def expected_outputs():
    """forward() of every state of the set, in its order"""
    return tuple(tuple(forward(c.state)) for c in steering_set())
