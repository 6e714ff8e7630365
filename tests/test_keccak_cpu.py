"""The Keccak hasher without a GPU: the test-side reference (tests/keccak_ref.py) against hashlib and known digests, the product's host
keccak256, word filter and challenger permutation against the reference, the Python mini-verifier against the oracle's Poseidon proofs
(so that it cannot pass vacuously), and a golden Keccak proof through the product's CPU verifier, its device verifier's CPU replay and
the mini-verifier."""
import hashlib
import random

import numpy as np
import pytest

import keccak_ref as K
import oracle_lib as O
import starky_bls12_381_amd as S
from keccak_util import cpu_code, flips, load_golden, mini_ok, replay_code
from random_air import random_air
from starky_bls12_381_amd import handoff

LENGTHS = [0, 1, 135, 136, 137, 272]
P = S.P


def _msg(n, seed=0):
    return bytes(random.Random(1000 * seed + n).randrange(256) for _ in range(n))


# ------------------------------------------------------------------------------------------------ the reference validates itself
@pytest.mark.parametrize("n", LENGTHS)
def test_reference_sponge_with_the_sha3_pad_is_hashlibs_sha3_256(n):
    m = _msg(n)
    assert K.sponge256(m, 0x06) == hashlib.sha3_256(m).digest()
    assert K.keccak256(m) != K.sponge256(m, 0x06)


def test_reference_keccak256_known_digests():
    assert K.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert K.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"


def test_reference_digest_encoding_round_trips_and_rejects_out_of_range_words():
    d = bytes(range(1, 26))
    w = K.digest_words(d)
    assert w == [int.from_bytes(d[0:7], "little"), int.from_bytes(d[7:14], "little"), int.from_bytes(d[14:21], "little"),
                 int.from_bytes(d[21:25], "little")]
    assert K.words_digest(w) == d and all(x < P for x in w)
    for i, bound in enumerate((1 << 56, 1 << 56, 1 << 56, 1 << 32)):
        bad = list(w)
        bad[i] = bound
        assert K.words_digest(bad) is None
    # K4: three elements are copied, four are hashed
    assert K.hash_or_noop([1, 2, 3]) == K.digest_words((1).to_bytes(8, "little") + (2).to_bytes(8, "little") + (3).to_bytes(8, "little") + b"\0")
    assert K.hash_or_noop([1, 2, 3, 4]) == K.hash_no_pad([1, 2, 3, 4]) != [1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ the product's host code
def test_host_keccak256_is_the_references():
    for n in LENGTHS:
        assert S.keccak256(_msg(n, 1)) == K.keccak256(_msg(n, 1)), n
    rng = random.Random(2)
    for _ in range(200):
        n = rng.randrange(1001)
        m = bytes(rng.randrange(256) for _ in range(n))
        assert S.keccak256(m) == K.keccak256(m), n


@pytest.mark.parametrize("where", [0, 5, 11], ids=["first", "middle", "twelfth"])
def test_word_filter_skips_words_at_or_above_p(where):
    rng = random.Random(where)
    good = [rng.randrange(P) for _ in range(12)]
    for big in (P, P + 1, (1 << 64) - 1):
        stream = good[:where] + [big] + good[where:] + [7, 8]
        state, used = S.keccak_state_from_words(stream)
        assert [int(x) for x in state] == good and used == 13
        assert K.state_from_words(stream) == (good, 13)
    # several in a row, and the largest word that passes
    stream = good[:where] + [P, (1 << 64) - 1, P - 1] + good[where:]
    state, used = S.keccak_state_from_words(stream)
    want = (good[:where] + [P - 1] + good[where:])[:12]
    assert [int(x) for x in state] == want and used == 14 and K.state_from_words(stream) == (want, 14)


def test_word_filter_on_a_stream_that_is_too_short():
    assert S.keccak_state_from_words([1] * 11)[1] == -1
    assert S.keccak_state_from_words([1] * 11 + [P] * 5)[1] == -1
    assert K.state_from_words([1] * 11 + [P] * 5) is None
    state, used = S.keccak_state_from_words([3] * 12)
    assert used == 12 and [int(x) for x in state] == [3] * 12


def test_host_permutation_is_the_references():
    rng = random.Random(3)
    states = [[0] * 12, [P - 1] * 12] + [[rng.randrange(P) for _ in range(12)] for _ in range(30)]
    for s in states:
        got = [int(x) for x in S.keccak_permute_host(s)]
        assert got == K.permute(s) and all(x < P for x in got)


# ------------------------------------------------------------------------------------------------ the mini-verifier is not vacuous
def _oracle_cases():
    cfg = S.StarkConfig.standard_fast_config()
    out = []
    for log_n in (4, 6):
        t, pis = S.trace_fibonacci(3, 5, 1 << log_n)
        blob = S.air_program(S.AIR_TEST_FIBONACCI)
        out.append(("fib%d" % log_n, S.AIR_TEST_FIBONACCI, blob, cfg, O.prove(blob, cfg, t.T.copy(), pis)))
    blob, t, pis = random_air(22, 12, 3, 1 << 6)
    out.append(("rand6", S.register_air(blob, name="keccak_cpu_rand6"), blob, cfg, O.prove(blob, cfg, t.T.copy(), pis)))
    return out


@pytest.fixture(scope="module")
def oracle_cases():
    return _oracle_cases()


def test_mini_verifier_accepts_the_oracles_poseidon_proofs_and_rejects_their_flips(oracle_cases):
    for name, air, blob, cfg, proof in oracle_cases:
        assert S.proof_hasher(proof) == S.HASHER_POSEIDON
        assert mini_ok(blob, cfg, proof, K.POSEIDON), name
        assert cpu_code(air, cfg, proof) == 0
        bad = flips(proof)
        assert sorted(bad) == ["cap", "final_poly", "opening", "sibling", "witness"]
        for what, b in bad.items():
            assert not mini_ok(blob, cfg, b, K.POSEIDON), (name, what)
            assert cpu_code(air, cfg, b) != 0, (name, what)
        assert not mini_ok(blob, cfg, proof, K.KECCAK), name  # the header names Poseidon


def test_poseidon_proof_with_the_keccak_id_is_rejected(oracle_cases):
    name, air, blob, cfg, proof = oracle_cases[1]
    bad = proof.copy()
    bad[12] = S.HASHER_KECCAK
    assert S.proof_hasher(bad) == S.HASHER_KECCAK
    assert cpu_code(air, cfg, bad) != 0 and replay_code(air, cfg, bad) == cpu_code(air, cfg, bad)
    assert not mini_ok(blob, cfg, bad, K.KECCAK) and not mini_ok(blob, cfg, bad, K.POSEIDON)
    bad[12] = 2
    with pytest.raises(S.StarkhipError) as e:
        S.proof_hasher(bad)
    assert e.value.code == S.ERR_BAD_SHAPE
    assert cpu_code(air, cfg, bad) == S.ERR_BAD_SHAPE == replay_code(air, cfg, bad)


# ------------------------------------------------------------------------------------------------ the golden Keccak proof
@pytest.fixture(scope="module")
def golden():
    cfg, proof = load_golden()
    return S.AIR_TEST_FIBONACCI, S.air_program(S.AIR_TEST_FIBONACCI), cfg, proof


def test_golden_keccak_proof_is_accepted_by_all_three_verifiers(golden):
    air, blob, cfg, proof = golden
    assert cfg.num_query_rounds == 4 and int(proof[3]) == 6
    assert S.proof_hasher(proof) == S.HASHER_KECCAK == 1
    assert cpu_code(air, cfg, proof) == 0
    assert replay_code(air, cfg, proof) == 0
    assert mini_ok(blob, cfg, proof, K.KECCAK)
    # every digest of the blob is in the ranges of its encoding
    L = S.proof_layout(proof)
    caps = proof[int(L.off_trace_cap):int(L.off_local_values)].reshape(-1, 4)
    assert (caps[:, :3] < (1 << 56)).all() and (caps[:, 3] < (1 << 32)).all()


def test_golden_keccak_proof_flips_are_rejected_by_all_three_verifiers(golden):
    air, blob, cfg, proof = golden
    bad = flips(proof)
    assert sorted(bad) == ["cap", "final_poly", "opening", "sibling", "witness"]
    for what, b in bad.items():
        assert cpu_code(air, cfg, b) != 0, what
        assert replay_code(air, cfg, b) == cpu_code(air, cfg, b), what
        assert not mini_ok(blob, cfg, b, K.KECCAK), what


def test_golden_keccak_proof_with_the_poseidon_id_is_rejected(golden):
    air, blob, cfg, proof = golden
    bad = proof.copy()
    bad[12] = S.HASHER_POSEIDON
    assert cpu_code(air, cfg, bad) != 0 and replay_code(air, cfg, bad) != 0
    assert not mini_ok(blob, cfg, bad, K.POSEIDON) and not mini_ok(blob, cfg, bad, K.KECCAK)


def test_golden_keccak_proof_with_a_digest_word_out_of_range_is_rejected(golden):
    air, blob, cfg, proof = golden
    L = S.proof_layout(proof)
    sib = int(L.off_query_rounds) + int(L.q_trace_siblings)
    positions = [int(L.off_trace_cap), int(L.off_quotient_cap) + 5, sib + 1, int(L.off_trace_cap) + 3, sib + 3]
    if int(L.n_fri_layers):
        positions.append(int(L.off_fri_caps) + 2)
    for pos in positions:
        bad = proof.copy()
        bad[pos] = int(bad[pos]) | (1 << 56)  # still a field element, no longer 7 (or 4) bytes
        assert int(bad[pos]) < P
        assert cpu_code(air, cfg, bad) != 0, pos
        assert replay_code(air, cfg, bad) != 0, pos
        assert not mini_ok(blob, cfg, bad, K.KECCAK), pos


def test_handoff_refuses_a_keccak_proof(golden, oracle_cases):
    with pytest.raises(ValueError, match="Poseidon"):
        handoff.dumps(golden[3])
    assert handoff.dumps(oracle_cases[0][4])  # a Poseidon proof still goes through
