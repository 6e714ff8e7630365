"""Permutation arguments of registered AIRs (starky's permutation_pairs(); COMPAT.md P1 - P8) without a GPU: the program blob's
section through builder, validator and registry; the host replay of the Z polynomials and the constraint fold over an extension frame
against the Python reference of tests/permutation_ref.py; the golden proofs (tests/golden/permutation_small.json, one per hasher)
through the CPU verifier, the device verifier's replay and the Python mini-verifier, intact and with one word changed in each field
a proof gains with nZ > 0."""
import os
import re

import numpy as np
import pytest

import keccak_ref as K
import permutation_ref as R
import starky_bls12_381_amd as S
from permutation_util import cpu_code, golden_case, load_golden, perm_air, perm_config, perm_flips
from starky_bls12_381_amd.air_builder import AirBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P


def _base_builder(n_cols=6, degree=3):
    b = AirBuilder(n_cols, 0, degree)
    b.constraint(b.L(1) - b.L(0) * b.L(0))
    return b


def _section(blob):
    """index of the section's first word (its magic) in a blob that has one"""
    w = [int(x) for x in blob]
    return 8 + w[5] + (w[6] + 1) // 2 + w[7]


# ------------------------------------------------------------------------------------------------ blob, validator, registry
def test_builder_blob_validator_round_trip():
    for degree in (2, 3, 5):
        air, blob = perm_air(degree)
        assert S.air_check_program(blob) is None
        base, pairs = R.split_program(blob)
        B = max(1, degree - 1)
        assert len(pairs) == (B + 1 if B >= 2 else 1) and pairs[0] == [(0, 3), (1, 4), (2, 5)]
        assert S.air_permutation_pairs(air) == len(pairs)
        assert S.air_permutation_zs(air) == 2 * -(-len(pairs) // B)
        assert np.array_equal(S.air_program(air), blob)  # the registry keeps the caller's bytes
        assert S.register_air(blob) == air
    assert S.air_permutation_zs(perm_air(3)[0]) == 4  # the golden AIR: three pairs, B = 2, two batches


def test_a_program_without_pairs_keeps_its_bytes_and_its_id():
    legacy = _base_builder().finish()
    assert int(legacy[0]) == 0x3152495F52494153 and R.AIR_PERM_MAGIC not in [int(x) for x in legacy]
    assert len(legacy) == _section(legacy)  # nothing after the group table
    a = S.register_air(legacy)
    assert S.register_air(legacy.copy()) == a
    assert S.air_permutation_pairs(a) == 0 and S.air_permutation_zs(a) == 0
    b = _base_builder()
    b.permutation_pair([(0, 1)])
    with_pairs = b.finish()
    assert np.array_equal(with_pairs[:len(legacy)], legacy)  # the section is appended, nothing in front of it moves
    a2 = S.register_air(with_pairs)
    assert a2 != a and S.air_permutation_zs(a2) == 2
    for builtin in (S.AIR_TEST_FIBONACCI, S.AIR_FP12_MUL):
        assert S.air_permutation_pairs(builtin) == 0 and S.air_permutation_zs(builtin) == 0
        prog = S.air_program(builtin)
        assert len(prog) == _section(prog)
    with pytest.raises(S.StarkhipError):
        S.air_permutation_zs(999)


def _refused(blob, needle):
    why = S.air_check_program(blob)
    assert why is not None and needle in why, why
    with pytest.raises(S.StarkhipError) as e:
        S.register_air(blob)
    assert e.value.code == S.ERR_BAD_AIR


def test_every_refusal_of_the_section():
    good = _base_builder()
    good.permutation_pair([(0, 1), (2, 3)])
    blob = good.finish()
    assert S.air_check_program(blob) is None
    at = _section(blob)
    # a column >= n_cols, as lhs and as rhs
    for bad_word in (6 | (1 << 32), 0 | (6 << 32), 0xFFFFFFFF | (1 << 32)):
        t = blob.copy()
        t[at + 3] = bad_word
        _refused(t, "out of range")
    # an empty pair
    t = np.concatenate([blob[:at], np.array([R.AIR_PERM_MAGIC, 1, 0], dtype=np.uint64)])
    _refused(t, "empty pair")
    # more batches than challenge sets: degree 3 has B = 2, five pairs make three batches
    b = _base_builder()
    for _ in range(5):
        b.permutation_pair([(0, 1)])
    _refused(b.finish(), "batches")
    b = _base_builder()
    for _ in range(4):
        b.permutation_pair([(0, 1)])
    assert S.air_check_program(b.finish()) is None  # four pairs, two batches: the most degree 3 admits
    # trailing words
    _refused(np.concatenate([blob, np.array([0], dtype=np.uint64)]), "trailing")
    # more than 64 pairs (degree 8 would admit 49; the count is refused before the batches are) and more than 64 entries in one pair
    b = _base_builder(degree=8)
    for _ in range(65):
        b.permutation_pair([(0, 1)])
    _refused(b.finish(), "pairs")
    b = _base_builder()
    b.permutation_pair([(0, 1)] * 65)
    _refused(b.finish(), "entries")
    b = _base_builder()
    b.permutation_pair([(0, 1)] * 64)
    assert S.air_check_program(b.finish()) is None
    # a section cut short, and a pair that runs past the blob
    _refused(blob[:at + 1], "shorter")
    _refused(blob[:-1], "past the blob")
    # a degree-1 program cannot carry the Z constraints
    b = AirBuilder(2, 0, 1)
    b.constraint(b.L(0) - b.L(1))
    b.permutation_pair([(0, 1)])
    _refused(b.finish(), "degree")


def test_fuzzed_sections_that_pass_are_in_bounds():
    """single-word mutations of the section: whatever the validator accepts names columns of the trace and stays inside the limits"""
    b = _base_builder(n_cols=7, degree=3)
    b.permutation_pair([(0, 3), (1, 4), (2, 5)])
    b.permutation_pair([(6, 0)])
    b.permutation_pair([(1, 4)])
    blob = b.finish()
    at = _section(blob)
    rng = np.random.default_rng(20240607)
    interesting = [0, 1, 2, 3, 6, 7, 63, 64, 65, 1 << 32, 7 << 32, (6 << 32) | 6, (7 << 32) | 6, (1 << 64) - 1, R.AIR_PERM_MAGIC]
    passed = 0
    for trial in range(1500):
        t = blob.copy()
        i = int(rng.integers(at, len(t)))
        t[i] = interesting[int(rng.integers(len(interesting)))] if trial % 3 else int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 63))
        if S.air_check_program(t) is not None:
            continue
        passed += 1
        _, pairs = R.split_program(t)  # asserts the section's own length
        assert 1 <= len(pairs) <= 64 and -(-len(pairs) // 2) <= 2
        for pair in pairs:
            assert 1 <= len(pair) <= 64
            assert all(l < 7 and r < 7 for l, r in pair)
    assert passed >= 20  # (an unchanged word, another column in range, ...)


# ------------------------------------------------------------------------------------------------ Z polynomials, constraints
def _challenges(degree, seed):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, P, 4 * max(1, degree - 1), dtype=np.uint64)]


@pytest.mark.parametrize("n_rows", [2, 4, 64, 256])
@pytest.mark.parametrize("degree", [2, 3, 5])
def test_zs_replay_is_the_references(degree, n_rows):
    air, blob = perm_air(degree)
    _, pairs = R.split_program(blob)
    ch = _challenges(degree, 100 * degree + n_rows)
    trace, _ = R.make_trace(degree, n_rows, seed=n_rows + degree, noncanonical=True)
    ref_zs, ref_closing = R.zs_and_closing(pairs, degree, trace.tolist(), ch)
    assert ref_closing == [1] * len(ref_closing)  # a true permutation closes, says the reference
    for layout, t in ((0, trace), (1, np.ascontiguousarray(trace.T))):
        zs, closing = S.permutation_zs_replay(air, t, ch, layout=layout)
        assert zs.tolist() == ref_zs and closing.tolist() == ref_closing
    assert all(z[0] == 1 for z in ref_zs)
    bad = trace.copy()
    bad[n_rows // 2, 4] = (int(bad[n_rows // 2, 4]) + 1) % P  # one rhs cell: column 4 is in the first pair and, for B >= 2, in the last one
    ref_zs, ref_closing = R.zs_and_closing(pairs, degree, bad.tolist(), ch)
    assert ref_closing[0] != 1 and ref_closing[1] != 1  # the reference says the first batch does not close, under either challenge
    zs, closing = S.permutation_zs_replay(air, bad, ch)
    assert zs.tolist() == ref_zs and closing.tolist() == ref_closing


def test_zs_replay_refuses_what_it_should():
    air, _ = perm_air(3)
    trace, _ = R.make_trace(3, 8, 1)
    ch = _challenges(3, 1)
    for args, code in (((S.AIR_TEST_FIBONACCI, np.zeros((8, 2), dtype=np.uint64), ch), S.ERR_BAD_AIR),  # no pairs
                       ((air, trace[:6], ch), S.ERR_BAD_SHAPE),                                          # rows no power of two
                       ((air, trace[:, :5], ch), S.ERR_BAD_SHAPE),                                       # another column count
                       ((air, trace, [P] + ch[1:]), S.ERR_BAD_SHAPE)):                                   # a challenge that is no field element
        with pytest.raises(S.StarkhipError) as e:
            S.permutation_zs_replay(*args)
        assert e.value.code == code


@pytest.mark.parametrize("degree", [2, 3, 5])
def test_eval_frame_full_is_the_references(degree):
    air, blob = perm_air(degree)
    base, pairs = R.split_program(blob)
    nz = S.air_permutation_zs(air)
    rng = np.random.default_rng(degree)
    for trial in range(3):
        ext = lambda k: rng.integers(0, P, size=(k, 2), dtype=np.uint64)  # noqa: E731
        local, nxt, zs, zs_next, masks, alphas = ext(6), ext(6), ext(nz), ext(nz), ext(4), ext(2)
        pis = rng.integers(0, P, 1, dtype=np.uint64)
        ch = _challenges(degree, 10 * degree + trial)
        got = S.air_eval_frame_full(air, local, nxt, pis, masks, alphas, zs, zs_next, ch)
        tup = lambda a: [(int(x), int(y)) for x, y in a]  # noqa: E731
        per_kind = K.constraints_ext(base, tup(local), tup(nxt), pis)
        m = tup(masks)
        own = []
        for k in range(int(base[4])):
            v = (0, 0)
            for kind in range(4):
                v = K.eadd(v, K.emul(m[kind], per_kind[kind][k]))
            own.append(v)
        first, plain = R.perm_constraints_ext(pairs, degree, tup(local), tup(zs), tup(zs_next), ch)
        want = [R.fold_full(own, first, plain, m, a) for a in tup(alphas)]
        assert tup(got) == want
        # the AIR's own part carries alpha^(2 nZ): the full fold differs from the plain one exactly by the permutation constraints
        plain_fold = tup(S.air_eval_frame(air, local, nxt, pis, masks, alphas))
        for j, a in enumerate(tup(alphas)):
            rest = R.fold_full([], first, plain, m, a)
            assert want[j] == K.eadd(K.emul(plain_fold[j], K.epow(a, 2 * nz)), rest)


def test_eval_frame_full_without_pairs_is_eval_frame():
    rng = np.random.default_rng(4)
    ext = lambda k: rng.integers(0, P, size=(k, 2), dtype=np.uint64)  # noqa: E731
    cols = S.air_columns(S.AIR_TEST_FIBONACCI)
    local, nxt, masks, alphas = ext(cols), ext(cols), ext(4), ext(2)
    pis = rng.integers(0, P, S.air_public_inputs(S.AIR_TEST_FIBONACCI), dtype=np.uint64)
    a = S.air_eval_frame(S.AIR_TEST_FIBONACCI, local, nxt, pis, masks, alphas)
    b = S.air_eval_frame_full(S.AIR_TEST_FIBONACCI, local, nxt, pis, masks, alphas, ext(0), ext(0), _challenges(S.air_constraint_degree(S.AIR_TEST_FIBONACCI), 0))
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ the golden proofs
@pytest.fixture(scope="module")
def golden():
    air, blob, cfg, trace, pis = golden_case()
    return air, blob, cfg, load_golden()


def test_golden_layout(golden):
    air, blob, cfg, proofs = golden
    assert sorted(proofs) == [S.HASHER_POSEIDON, S.HASHER_KECCAK]
    for hasher, proof in proofs.items():
        assert S.proof_hasher(proof) == hasher and int(proof[13]) == 4
        L = S.proof_layout(proof)
        g = lambda f: int(getattr(L, f))  # noqa: E731
        ncap, C, Q, nZ, d0 = 1 << cfg.cap_height, 6, 4, 4, 5 + cfg.rate_bits - cfg.cap_height
        assert (g("n_columns"), g("n_quotient_polys"), g("degree_bits"), g("n_permutation_zs"), g("initial_sibling_count")) == (C, Q, 5, nZ, d0)
        assert g("off_trace_cap") == 16
        assert g("off_permutation_zs_cap") == 16 + 4 * ncap
        assert g("off_quotient_cap") == 16 + 8 * ncap
        assert g("off_local_values") == 16 + 12 * ncap
        assert g("off_next_values") == g("off_local_values") + 2 * C
        assert g("off_permutation_zs") == g("off_next_values") + 2 * C
        assert g("off_permutation_zs_next") == g("off_permutation_zs") + 2 * nZ
        assert g("off_quotient_openings") == g("off_permutation_zs_next") + 2 * nZ
        assert g("off_fri_caps") == g("off_quotient_openings") + 2 * Q
        assert (g("q_trace_leaf"), g("q_trace_siblings")) == (0, C)
        assert g("q_permutation_zs_leaf") == C + 4 * d0
        assert g("q_permutation_zs_siblings") == C + 4 * d0 + nZ
        assert g("q_quotient_leaf") == C + nZ + 8 * d0
        assert g("q_quotient_siblings") == g("q_quotient_leaf") + Q
        assert g("query_round_words") >= C + nZ + Q + 12 * d0
        assert g("total_words") == proof.size
        # the hand-off value has the three fields, and goes back to the same words
        if hasher == S.HASHER_POSEIDON:
            from starky_bls12_381_amd import handoff
            v = handoff.proof_to_value(proof)
            assert len(v["proof"]["permutation_zs_cap"]) == ncap
            assert len(v["proof"]["openings"]["permutation_zs"]) == nZ == len(v["proof"]["openings"]["permutation_zs_next"])
            assert len(v["proof"]["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"]["evals_proofs"]) == 3
            assert np.array_equal(handoff.value_to_proof(v, 5, cfg.rate_bits, cfg.arity_bits), proof)


def test_golden_proofs_are_accepted_by_all_three_verifiers(golden):
    air, blob, cfg, proofs = golden
    for hasher, proof in proofs.items():
        assert cpu_code(air, cfg, proof) == 0
        assert S.verify_batch_replay([(air, cfg, proof)]) == [0]
        R.verify_or_raise(blob, cfg, proof, hasher)
    both = [(air, cfg, proofs[0]), (air, cfg, proofs[1])]
    assert S.verify_batch_replay(both) == [0, 0]


def test_one_changed_word_in_each_new_field_is_rejected(golden):
    air, blob, cfg, proofs = golden
    for hasher, proof in proofs.items():
        bad = perm_flips(proof)
        assert sorted(bad) == ["zs_cap", "zs_leaf", "zs_next_opening", "zs_opening", "zs_sibling"]
        for name, t in bad.items():
            assert cpu_code(air, cfg, t) == S.ERR_VERIFY, (hasher, name)
            assert S.verify_batch_replay([(air, cfg, t)]) == [S.ERR_VERIFY], (hasher, name)
            with pytest.raises(K.Reject):
                R.verify_or_raise(blob, cfg, t, hasher)
        # a batch of the good proof and its tampered copies: the replay gives the CPU verifier's codes, proof by proof
        items = [(air, cfg, proof)] + [(air, cfg, t) for t in bad.values()]
        assert S.verify_batch_replay(items) == [cpu_code(*it) for it in items] == [0] + [S.ERR_VERIFY] * 5


def test_header_word_13_is_part_of_the_shape(golden):
    air, blob, cfg, proofs = golden
    for proof in proofs.values():
        for v in (0, 2, 3, 5, 129, 1 << 40):
            t = proof.copy()
            t[13] = v
            assert cpu_code(air, cfg, t) == S.ERR_BAD_SHAPE
            assert S.verify_batch_replay([(air, cfg, t)]) == [S.ERR_BAD_SHAPE]
            with pytest.raises(S.StarkhipError):
                S.proof_layout(t)
    # ... and a proof of an AIR without pairs must say 0 there
    legacy, _ = R.split_program(blob)
    plain_air = S.register_air(legacy)
    assert cpu_code(plain_air, cfg, proofs[0]) == S.ERR_BAD_SHAPE


def _header(C, Q, nZ, L, cap_h, n_queries, log_n=4, rate_bits=2, arity_bits=1, n_pis=3):
    return [0x3130304652505353, C, Q, log_n, rate_bits, cap_h, L, n_queries, 1 << (log_n - L * arity_bits), n_pis, arity_bits, 2, 0, nZ, 0, 0]


@pytest.mark.parametrize("n_queries", [0, 3])
@pytest.mark.parametrize("cap_h", [0, 2])
@pytest.mark.parametrize("L", [0, 2])
@pytest.mark.parametrize("C,Q,nZ", [(2, 2, 0), (6, 4, 2), (6, 8, 4), (0, 2, 0), (2, 0, 0), (0, 0, 2)])  # (the header check lets 0 columns pass)
def test_layout_of_a_bare_header_is_the_documented_walk(C, Q, nZ, L, cap_h, n_queries):
    """starkhip_proof_layout reads the header and the length alone: every offset and every q_* field against the field list of the
    layout comment in include/starkhip.h, walked here in its order -- (name, words) of the blob, then of one query round."""
    h = _header(C, Q, nZ, L, cap_h, n_queries)
    log_N, ab, final_len, n_pis = h[3] + h[4], h[10], h[8], h[9]
    ncap, d0 = 1 << cap_h, log_N - cap_h
    depth = [log_N - (l + 1) * ab - cap_h for l in range(L)]
    zs = nZ > 0
    round_fields = [("q_trace_leaf", C), ("q_trace_siblings", 4 * d0)]
    round_fields += [("q_permutation_zs_leaf", nZ), ("q_permutation_zs_siblings", 4 * d0)] if zs else []
    round_fields += [("q_quotient_leaf", Q), ("q_quotient_siblings", 4 * d0)]
    for l in range(L):
        round_fields += [(("q_step_evals", l), 2 * (1 << ab)), (("q_step_siblings", l), 4 * depth[l])]
    round_words = sum(w for _, w in round_fields)
    blob_fields = [("off_trace_cap", 4 * ncap)] + ([("off_permutation_zs_cap", 4 * ncap)] if zs else []) + [("off_quotient_cap", 4 * ncap)]
    blob_fields += [("off_local_values", 2 * C), ("off_next_values", 2 * C)]
    blob_fields += [("off_permutation_zs", 2 * nZ), ("off_permutation_zs_next", 2 * nZ)] if zs else []
    blob_fields += [("off_quotient_openings", 2 * Q), ("off_fri_caps", L * 4 * ncap), ("off_query_rounds", n_queries * round_words),
                    ("off_final_poly", 2 * final_len), ("off_pow_witness", 1), ("off_public_inputs", n_pis)]
    want, o = {}, 16
    for name, w in blob_fields:
        want[name], o = o, o + w
    total, o = o, 0
    for name, w in round_fields:
        want[name], o = o, o + w
    want.update(total_words=total, query_round_words=round_words, initial_sibling_count=d0, n_permutation_zs=nZ, n_columns=C, n_quotient_polys=Q,
                degree_bits=h[3], rate_bits=h[4], cap_height=cap_h, n_fri_layers=L, n_query_rounds=n_queries, final_poly_len=final_len,
                n_public_inputs=n_pis, arity_bits=ab)
    for l in range(L):
        want[("step_sibling_count", l)] = depth[l]
    blob = np.zeros(total, dtype=np.uint64)
    blob[:16] = h
    got_struct = S.proof_layout(blob)
    got = {}
    for name, _ in S.ProofLayout._fields_:
        v = getattr(got_struct, name)
        if isinstance(v, int):
            got[name] = v
        else:
            got.update({(name, l): int(x) for l, x in enumerate(v)})
    # what the comment's walk does not name is 0: the Z fields of a proof without Zs, the step entries past L
    assert got == {k: want.get(k, 0) for k in got}
    assert set(want) <= set(got)
    for words in (total - 1, total + 1):  # a length one word off
        with pytest.raises(S.StarkhipError):
            S.proof_layout(np.concatenate([blob, np.zeros(1, dtype=np.uint64)])[:words])
    over = blob.copy()
    over[13] = 129  # nZ > 128 is no header, whatever the length
    for words in (total, total + (129 - nZ) * (4 + n_queries) + (0 if zs else 4 * ncap + 4 * d0 * n_queries)):  # ... the one 129 Zs would give too
        t = np.zeros(words, dtype=np.uint64)
        t[:16] = over[:16]
        with pytest.raises(S.StarkhipError):
            S.proof_layout(t)


def test_rust_mirror_has_the_new_names():
    rs = open(os.path.join(ROOT, "bindings", "rust", "starkhip-sys", "src", "lib.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("starkhip_air_permutation_pairs", "starkhip_air_permutation_zs", "starkhip_permutation_zs", "starkhip_permutation_zs_replay",
                 "starkhip_air_eval_frame_full"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
    for field in ("n_permutation_zs", "off_permutation_zs_cap", "off_permutation_zs", "off_permutation_zs_next", "q_permutation_zs_leaf",
                  "q_permutation_zs_siblings"):
        assert re.search(r"\b%s\b" % field, hdr) and re.search(r"pub %s: usize" % field, rs), field
    assert "STARKHIP_AIR_MAX_PERMUTATION_PAIRS 64u" in hdr
