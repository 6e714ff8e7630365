"""The Keccak hasher (KeccakGoldilocksConfig) on the GPU: its kernels against the pure-Python reference of tests/keccak_ref.py, and whole
proofs with "hasher" = 1 through the product's CPU verifier, its device verifier and the Python mini-verifier."""
import numpy as np
import pytest

import keccak_ref as K
import oracle_lib as O
import starky_bls12_381_amd as S
from keccak_util import cpu_code, flips, mini_ok
from random_air import random_air

pytestmark = pytest.mark.gpu


@pytest.fixture
def kprover(prover):
    """the shared context with "hasher" = 1 for the length of one test"""
    prover.set_option("hasher", S.HASHER_KECCAK)
    yield prover
    prover.set_option("hasher", S.HASHER_POSEIDON)


def _bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_permutation_batch_is_the_references(prover, n):
    rng = np.random.default_rng(n)
    states = rng.integers(0, S.P, size=(n, 12), dtype=np.uint64)
    states[0] = 0
    if n > 1:
        states[1] = S.P - 1
    got = prover.keccak_permute_batch(states)
    for i in range(0, n, max(1, n // 70)):  # every state of the short batches, 70-odd of the long one (pure Python: 3 hashes each)
        assert [int(x) for x in got[i]] == K.permute([int(x) for x in states[i]]), i
    assert np.array_equal(got[-1], S.keccak_permute_host(states[-1]))
    assert np.array_equal(got, np.array([S.keccak_permute_host(s) for s in states]))  # ... and all of them against the host's


WIDTHS = [1, 2, 3, 4, 5, 16, 17, 18, 33, 34, 35, 51]  # the noop boundary; one word either side of the first three block edges
_REF_TREES = {}


def _ref_tree(width, log_N):
    """(matrix [width][N], leaf digests in tree order, {cap height: cap}) by the reference, computed once"""
    key = (width, log_N)
    if key not in _REF_TREES:
        N = 1 << log_N
        rng = np.random.default_rng(1000 * width + log_N)
        mat = rng.integers(0, S.P, size=(width, N), dtype=np.uint64)
        mat[0, 0] = S.P - 1
        leaves = [K.hash_or_noop([int(mat[c, _bitrev(j, log_N)]) for c in range(width)]) for j in range(N)]
        caps, level, h = {log_N: leaves}, leaves, log_N
        while h > 0:
            level = [K.two_to_one(level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
            h -= 1
            caps[h] = level
        _REF_TREES[key] = (mat, leaves, caps)
    return _REF_TREES[key]


@pytest.mark.parametrize("log_N", [1, 3, 6, 7])
@pytest.mark.parametrize("width", WIDTHS)
def test_merkle_tree_is_the_references(prover, width, log_N):
    mat, leaves, caps = _ref_tree(width, log_N)
    for cap_h in (0, 1, log_N):
        digests, cap = prover.merkle_tree(mat, cap_h, hasher=S.HASHER_KECCAK)
        assert [[int(x) for x in d] for d in digests] == leaves, (width, log_N)
        assert [[int(x) for x in d] for d in cap] == caps[cap_h], (width, log_N, cap_h)
        assert (digests[:, :3] < (1 << 56)).all() and (digests[:, 3] < (1 << 32)).all()


@pytest.mark.parametrize("width,log_N", [(1, 3), (4, 6), (5, 6), (35, 7)])
def test_merkle_tree_under_hasher_0_is_merkle_cap(prover, width, log_N):
    mat = _ref_tree(width, log_N)[0]
    for cap_h in (0, 1, log_N):
        digests, cap = prover.merkle_tree(mat, cap_h, hasher=S.HASHER_POSEIDON)
        assert np.array_equal(cap, prover.merkle_cap(mat, cap_h))
        assert np.array_equal(cap, O.merkle_cap(mat.T.copy(), cap_h))
        if cap_h == log_N:
            assert np.array_equal(cap, digests)


@pytest.mark.parametrize("n_leaves", [1, 64, 65])
@pytest.mark.parametrize("width", [2, 3, 4, 32, 512])
def test_row_hashing_is_the_references(prover, width, n_leaves):
    rng = np.random.default_rng(width * 100 + n_leaves)
    rows = rng.integers(0, S.P, size=(n_leaves, width), dtype=np.uint64)
    got = prover.hash_rows(rows, hasher=S.HASHER_KECCAK)
    step = 1 if width < 512 else 13  # pure Python at 512 words a leaf: 5 of the 65
    for j in list(range(0, n_leaves, step)) + [n_leaves - 1]:
        assert [int(x) for x in got[j]] == K.hash_or_noop([int(x) for x in rows[j]]), j
    ref0 = np.array([K.PoseidonHasher.hash_or_noop(r) for r in rows], dtype=np.uint64)
    assert np.array_equal(prover.hash_rows(rows, hasher=S.HASHER_POSEIDON), ref0)


def test_entries_refuse_an_unknown_hasher(prover):
    mat = np.ones((2, 4), dtype=np.uint64)
    for call in (lambda: prover.merkle_tree(mat, 0, hasher=2), lambda: prover.hash_rows(mat, hasher=-1), lambda: prover.set_option("hasher", 2)):
        with pytest.raises(S.StarkhipError) as e:
            call()
        assert e.value.code == S.ERR_BAD_SHAPE


# ------------------------------------------------------------------------------------------------ whole proofs
def _cfg(**kw):
    cfg = S.StarkConfig.standard_fast_config()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


_AIRS = {}


def _air(name):
    """(air id, program blob, row-major trace, public inputs)"""
    if name not in _AIRS:
        if name.startswith("fib"):
            t, pis = S.trace_fibonacci(3, 5, 1 << int(name[3:]))
            _AIRS[name] = (S.AIR_TEST_FIBONACCI, S.air_program(S.AIR_TEST_FIBONACCI), t, pis)
        elif name == "noop6":  # one column, two quotient polynomials: trace and quotient leaves are copied, not hashed
            blob, t, pis = random_air(11, 1, 2, 1 << 6)
            _AIRS[name] = (S.register_air(blob, name="keccak_noop6"), blob, t, pis)
        elif name == "rand8":
            blob, t, pis = random_air(22, 12, 3, 1 << 8)
            _AIRS[name] = (S.register_air(blob, name="keccak_rand8"), blob, t, pis)
        else:  # a registered AIR on the long-trace path
            blob, t, pis = random_air(23, 4, 2, 1 << 14)
            _AIRS[name] = (S.register_air(blob, name="keccak_long14"), blob, t, pis)
    return _AIRS[name]


# Leaves of at most 3 words take the noop rule under Keccak, a 4-word leaf is hashed: both happen among these (narrow trace and quotient
# leaves, 2-word FRI leaves at arity 1 -- 2 x 2^1 = 4 words, hashed --, wide random and long traces).  Configs: standard_fast,
# cap_height 0, arity_bits 1 and 8, no query rounds.
PROOF_CASES = [
    ("fib4", {}), ("fib6", {}), ("fib10", {}),
    ("fib6", {"cap_height": 0}), ("fib10", {"arity_bits": 1, "num_query_rounds": 20}), ("fib6", {"num_query_rounds": 0}),
    ("noop6", {"num_query_rounds": 28}), ("rand8", {}), ("rand8", {"cap_height": 0, "num_query_rounds": 28}), ("rand8", {"arity_bits": 1, "num_query_rounds": 20}),
    ("long14", {"num_query_rounds": 28}), ("long14", {"arity_bits": 8, "num_query_rounds": 6}),
]


@pytest.mark.parametrize("name,cfg_kw", PROOF_CASES, ids=[n + "".join("-%s%d" % (k[:3], v) for k, v in kw.items()) for n, kw in PROOF_CASES])
def test_keccak_proof_verifies_everywhere_and_its_flips_nowhere(kprover, name, cfg_kw):
    air, blob, t, pis = _air(name)
    cfg = _cfg(**cfg_kw)
    proof = kprover.prove(air, cfg, t, pis)
    assert S.proof_hasher(proof) == S.HASHER_KECCAK and int(proof[12]) == 1
    assert (proof[16:] < S.P).all()
    assert cpu_code(air, cfg, proof) == 0
    assert mini_ok(blob, cfg, proof, K.KECCAK)
    assert np.array_equal(kprover.prove(air, cfg, t, pis), proof)
    bad = flips(proof)
    assert len(bad) == (5 if cfg.num_query_rounds else 4)
    items = [(air, cfg, proof)] + [(air, cfg, b) for b in bad.values()]
    codes = kprover.verify_batch(items)
    assert codes[0] == 0
    for (what, b), code in zip(bad.items(), codes[1:]):
        assert code != 0, what
        assert cpu_code(air, cfg, b) == code, what
        assert not mini_ok(blob, cfg, b, K.KECCAK), what
    assert S.verify_batch_replay(items) == codes


def test_hasher_0_proofs_are_what_they_were(prover):
    air, blob, t, pis = _air("fib6")
    cfg = _cfg()
    first = prover.prove(air, cfg, t, pis)
    prover.set_option("hasher", S.HASHER_KECCAK)
    try:
        second = prover.prove(air, cfg, t, pis)
    finally:
        prover.set_option("hasher", S.HASHER_POSEIDON)
    third = prover.prove(air, cfg, t, pis)
    assert S.proof_hasher(first) == 0 and S.proof_hasher(second) == 1
    assert np.array_equal(first, third) and not np.array_equal(first, second)
    w = int(first[int(S.proof_layout(first).off_pow_witness)])
    assert np.array_equal(first, O.prove(blob, cfg, t.T.copy(), pis, w))
    assert mini_ok(blob, cfg, first, K.POSEIDON) and not mini_ok(blob, cfg, first, K.KECCAK)


def _builtin(which):
    from bls_util import fp_arr, native_vectors, random_fp12
    if which == "fp12":
        return S.AIR_FP12_MUL, S.trace_fp12_mul(random_fp12(0x6B01), random_fp12(0x6B02))
    b = {k: int(s) for k, s in native_vectors()["bls_signature"].items()}
    return S.AIR_PAIRING_PRECOMP, S.trace_pairing_precomp(fp_arr(b["hm_x1"], b["hm_x2"]), fp_arr(b["hm_y1"], b["hm_y2"]),
                                                          fp_arr(b["hm_z1"], b["hm_z2"]))


@pytest.mark.parametrize("which", ["fp12", "precomp"])
def test_builtin_air_under_keccak(kprover, which):
    """FP12Mul: 60 285 columns = 17 x 3546 + 3, a last block of 3 words; PairingPrecomp: 29 376 = 17 x 1728, the padding-only block."""
    air, (t, pis) = _builtin(which)
    C_ = S.air_columns(air)
    assert C_ % 17 == (3 if which == "fp12" else 0)
    cfg = S.StarkConfig.for_air(air)
    proof = kprover.prove(air, cfg, t, pis)
    assert S.proof_hasher(proof) == 1
    L = S.proof_layout(proof)
    q0 = int(L.off_query_rounds)
    bad = proof.copy()
    bad[q0 + 5] = (int(bad[q0 + 5]) + 1) % S.P  # a word of the first opened trace leaf
    assert kprover.verify_batch([(air, cfg, proof), (air, cfg, bad)]) == [0, S.ERR_VERIFY]
    assert cpu_code(air, cfg, proof) == 0 and cpu_code(air, cfg, bad) == S.ERR_VERIFY
    # three opened trace leaves by the reference: leaf -> siblings -> the cap entry the index selects
    depth, cap_h = int(L.initial_sibling_count), int(L.cap_height)
    cap = [int(x) for x in proof[int(L.off_trace_cap):int(L.off_trace_cap) + 4 * (1 << cap_h)]]
    for q in range(3):
        base = q0 + q * int(L.query_round_words)
        cur = K.hash_or_noop([int(x) for x in proof[base:base + C_]])
        sibs = [int(x) for x in proof[base + int(L.q_trace_siblings):base + int(L.q_trace_siblings) + 4 * depth]]
        level = [cur]  # the index is the transcript's: every left / right order of the path, one of which ends in the cap
        for d in range(depth):
            sb = sibs[4 * d:4 * d + 4]
            level = [K.two_to_one(sb, c) for c in level] + [K.two_to_one(c, sb) for c in level]
        assert any(c == cap[4 * e:4 * e + 4] for c in level for e in range(1 << cap_h)), q


def test_mixed_batch_verdicts_are_the_cpu_verifiers(prover):
    air, blob, t, pis = _air("fib6")
    air2, blob2, t2, pis2 = _air("rand8")
    cfg = _cfg(num_query_rounds=12)
    items = []
    for hasher in (0, 1):
        prover.set_option("hasher", hasher)
        try:
            for a, tt, pp in ((air, t, pis), (air2, t2, pis2)):
                proof = prover.prove(a, cfg, tt, pp)
                items.append((a, cfg, proof))
                items += [(a, cfg, b) for b in flips(proof).values()]
                swapped = proof.copy()
                swapped[12] = 1 - hasher  # the other hasher's id on the same words
                items.append((a, cfg, swapped))
                unknown = proof.copy()
                unknown[12] = 2
                items.append((a, cfg, unknown))
        finally:
            prover.set_option("hasher", S.HASHER_POSEIDON)
    order = [k for pair in zip(range(len(items) // 2), range(len(items) // 2, len(items))) for k in pair]  # Poseidon and Keccak alternate
    items = [items[k] for k in order]
    codes = prover.verify_batch(items)
    assert codes == [cpu_code(a, c, p) for a, c, p in items]
    assert codes.count(0) == 4 and S.ERR_BAD_SHAPE in codes and S.ERR_VERIFY in codes
    assert S.verify_batch_replay(items) == codes
