"""LogUp lookups of registered AIRs (starky >= 0.2's Lookup; COMPAT.md L1 - L7) without a GPU: the program blob's section through
builder, validator and registry; the host replay of the auxiliary polynomials and the constraint fold over an extension frame against
the Python reference of tests/logup_ref.py; the golden proofs (tests/golden/logup_small.json, one per hasher) through the CPU
verifier, the device verifier's replay and the Python mini-verifier, intact and with one word changed in each field a proof gains
with nA > 0."""
import os
import re
import subprocess

import numpy as np
import pytest

import keccak_ref as K
import logup_ref as R
import starky_bls12_381_amd as S
from logup_util import cpu_code, golden_case, load_golden, logup_air, logup_flips, m_cases
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
        for m in m_cases(degree):
            air, blob = logup_air(degree, m, 2)
            assert S.air_check_program(blob) is None
            base, lookups = R.split_program(blob)
            assert lookups == [(list(range(4, 4 + m)), 3, 4 + m), (list(range(5 + m, 5 + 2 * m)), 3, 5 + 2 * m)]
            at = _section(blob)
            assert int(blob[at]).to_bytes(8, "little") == b"LOGUPS01" and int(blob[at + 1]) == 2
            assert [int(x) for x in blob[at + 2:at + 4 + m]] == [m, 3 | ((4 + m) << 32)] + list(range(4, 4 + m))
            assert S.air_logups(air) == 2
            H = -(-m // (degree - 1))
            assert S.air_logup_polys(air) == 4 * (H + 1) == R.n_polys(lookups, degree)
            assert S.air_permutation_pairs(air) == 0 and S.air_permutation_zs(air) == 0
            assert np.array_equal(S.air_program(air), blob)  # the registry keeps the caller's bytes
            assert S.register_air(blob) == air


CPP_BUILDER = r"""
#include <stdio.h>
#include "air_ir.h"
using namespace starkhip;
int main() {
    for (uint32_t degree : {2u, 3u, 5u})
        for (uint32_t m : {1u, degree - 1, degree}) {
            AirBuilder b(4 + 2 * (m + 1), 1, degree);
            b.constraint(b.L(1) - b.L(0) * b.L(0));
            if (degree == 2) b.constraint(b.L(2) - b.L(0) * b.L(1));
            else if (degree == 3) b.constraint(b.L(2) - b.L(0) * b.L(0) * b.L(0));
            else {
                b.constraint(b.L(2) - b.L(1) * b.L(1) * b.L(0));
                b.constraint(b.L(0) * b.L(1) * (b.L(2) - b.L(1) * b.L(1) * b.L(0)));
            }
            b.transition(b.N(0) - b.L(0) - 1);
            b.first_row(b.L(0) - b.PI(0));
            for (uint32_t l = 0; l < 2; l++) {
                std::vector<uint32_t> cols;
                for (uint32_t c = 0; c < m; c++) cols.push_back(4 + l * (m + 1) + c);
                b.logup(cols, 3, 4 + l * (m + 1) + m);
            }
            printf("%u %u", degree, m);
            for (uint64_t w : b.finish().serialize()) printf(" %llx", (unsigned long long)w);
            printf("\n");
        }
    return 0;
}
"""


def test_cpp_and_python_builders_emit_the_same_words(tmp_path):
    src = tmp_path / "logup_builder.cpp"
    src.write_text(CPP_BUILDER)
    exe = tmp_path / "logup_builder"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "starky_bls12_381_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert len(lines) == 9
    for line in lines:
        f = line.split()
        degree, m = int(f[0]), int(f[1])
        assert [int(x, 16) for x in f[2:]] == [int(x) for x in R.make_air(degree, m, 2)], (degree, m)


def test_a_program_without_the_section_keeps_its_bytes_and_its_id():
    legacy = _base_builder().finish()
    assert int(legacy[0]) == 0x3152495F52494153 and R.AIR_LOGUP_MAGIC not in [int(x) for x in legacy]
    assert len(legacy) == _section(legacy)  # nothing after the group table
    a = S.register_air(legacy)
    assert S.register_air(legacy.copy()) == a
    assert S.air_logups(a) == 0 and S.air_logup_polys(a) == 0
    b = _base_builder()
    b.logup([0, 1], 2, 3)
    with_lookups = b.finish()
    assert np.array_equal(with_lookups[:len(legacy)], legacy)  # the section is appended, nothing in front of it moves
    a2 = S.register_air(with_lookups)
    assert a2 != a and S.air_logups(a2) == 1 and S.air_logup_polys(a2) == 4
    for builtin in (S.AIR_TEST_FIBONACCI, S.AIR_FP12_MUL):
        assert S.air_logups(builtin) == 0 and S.air_logup_polys(builtin) == 0
        prog = S.air_program(builtin)
        assert len(prog) == _section(prog)
    with pytest.raises(S.StarkhipError):
        S.air_logup_polys(999)
    # a program with pairs keeps its bytes too: the builder emits one section or the other
    b = _base_builder()
    b.permutation_pair([(0, 1)])
    pairs = b.finish()
    assert R.AIR_LOGUP_MAGIC not in [int(x) for x in pairs] and S.air_check_program(pairs) is None


def _refused(blob, needle):
    why = S.air_check_program(blob)
    assert why is not None and needle in why, why
    with pytest.raises(S.StarkhipError) as e:
        S.register_air(blob)
    assert e.value.code == S.ERR_BAD_AIR


def test_every_refusal_of_the_section():
    good = _base_builder()
    good.logup([0, 1], 2, 3)
    blob = good.finish()
    assert S.air_check_program(blob) is None
    at = _section(blob)
    u = lambda *w: np.array(w, dtype=np.uint64)  # noqa: E731
    # a column >= n_cols: a looked-up column, the table, the frequencies
    for i, bad_word in ((at + 4, 6), (at + 5, 1 << 32), (at + 3, 6 | (3 << 32)), (at + 3, 2 | (6 << 32)), (at + 3, 0xFFFFFFFF | (3 << 32))):
        t = blob.copy()
        t[i] = bad_word
        _refused(t, "out of range")
    # an empty lookup
    _refused(np.concatenate([blob[:at], u(R.AIR_LOGUP_MAGIC, 1, 0, 2 | (3 << 32))]), "empty lookup")
    # no lookups, more than 64 lookups, more than 64 columns in one
    _refused(np.concatenate([blob[:at], u(R.AIR_LOGUP_MAGIC, 0)]), "lookups")
    b = _base_builder()
    for _ in range(65):
        b.logup([0], 2, 3)
    _refused(b.finish(), "lookups")
    b = _base_builder()
    b.logup([0] * 65, 2, 3)
    _refused(b.finish(), "columns")
    b = _base_builder()
    b.logup([0] * 64, 2, 3)
    assert S.air_check_program(b.finish()) is None
    # nA above 1024: at degree 2 a lookup of 64 columns has 65 polynomials per challenge -- seven are 910, eight 1040
    for n, ok in ((7, True), (8, False)):
        b = _base_builder(degree=2)
        for _ in range(n):
            b.logup([0] * 64, 2, 3)
        if ok:
            assert S.air_check_program(b.finish()) is None
        else:
            _refused(b.finish(), "auxiliary polynomials")
    # degree 1
    b = AirBuilder(4, 0, 1)
    b.constraint(b.L(0) - b.L(1))
    b.logup([0], 2, 3)
    _refused(b.finish(), "degree")
    # pairs and LogUp together, in either order
    b = _base_builder()
    b.permutation_pair([(0, 1)])
    pairs = b.finish()
    _refused(np.concatenate([pairs, blob[at:]]), "together")
    _refused(np.concatenate([blob, pairs[_section(pairs):]]), "together")
    # trailing words, a section cut short, a lookup that runs past the blob
    _refused(np.concatenate([blob, u(0)]), "trailing")
    _refused(blob[:at + 1], "shorter")
    _refused(blob[:at + 3], "past the blob")
    _refused(blob[:-1], "past the blob")


def test_fuzzed_sections_that_pass_are_in_bounds():
    """single-word mutations of the section: whatever the validator accepts names columns of the trace and stays inside the limits"""
    b = _base_builder(n_cols=7, degree=3)
    b.logup([0, 3, 5], 1, 2)
    b.logup([6], 0, 4)
    b.logup([1, 4], 6, 6)
    blob = b.finish()
    at = _section(blob)
    rng = np.random.default_rng(20241021)
    interesting = [0, 1, 2, 3, 6, 7, 63, 64, 65, 1 << 32, 7 << 32, (6 << 32) | 6, (7 << 32) | 6, (1 << 64) - 1, R.AIR_LOGUP_MAGIC, 0x3153524941504D50]
    passed = 0
    for trial in range(1500):
        t = blob.copy()
        i = int(rng.integers(at, len(t)))
        t[i] = interesting[int(rng.integers(len(interesting)))] if trial % 3 else int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 63))
        if S.air_check_program(t) is not None:
            continue
        if int(t[at]) != R.AIR_LOGUP_MAGIC:  # the magic became the pairs': a program of permutation pairs, test_permutation_cpu's ground
            assert S.air_logups(S.register_air(t)) == 0
            continue
        passed += 1
        _, lookups = R.split_program(t)  # asserts the section's own length
        assert 1 <= len(lookups) <= 64 and R.n_polys(lookups, 3) <= 1024
        for cols, table, freq in lookups:
            assert 1 <= len(cols) <= 64 and table < 7 and freq < 7 and all(c < 7 for c in cols)
    assert passed >= 20  # (an unchanged word, another column in range, ...)


# ------------------------------------------------------------------------------------------------ polynomials, constraints
def _challenges(seed):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, P, 2, dtype=np.uint64)]


@pytest.mark.parametrize("n_rows", [2, 4, 64, 256])
@pytest.mark.parametrize("degree", [2, 3, 5])
def test_polys_replay_is_the_references(degree, n_rows):
    for m in m_cases(degree):  # 1, a full batch, a full batch and a batch of one
        air, blob = logup_air(degree, m, 2)
        _, lookups = R.split_program(blob)
        ch = _challenges(100 * degree + n_rows + m)
        trace, _ = R.make_trace(degree, m, 2, n_rows, seed=n_rows + degree + m, noncanonical=True)
        assert (trace >= np.uint64(P)).any()
        ref_polys, ref_closing, ref_zeros = R.polys_and_closing(lookups, degree, trace.tolist(), ch)
        assert ref_closing == [[0, 0], [0, 0]] and ref_zeros == 0  # true multiplicities close, says the reference
        for layout, t in ((0, trace), (1, np.ascontiguousarray(trace.T))):
            polys, closing, zeros = S.logup_polys_replay(air, t, ch, layout=layout)
            assert polys.tolist() == ref_polys and closing.tolist() == ref_closing and zeros == 0
        H = -(-m // (degree - 1))
        assert all(ref_polys[i * 2 * (H + 1) + l * (H + 1) + H][0] == 0 for i in range(2) for l in range(2))  # Z(0) = 0
        bad = trace.copy()
        bad[n_rows // 2, lookups[1][2]] = (int(bad[n_rows // 2, lookups[1][2]]) + 1) % P  # the second lookup's frequencies, off by one in one row
        ref_polys, ref_closing, _ = R.polys_and_closing(lookups, degree, bad.tolist(), ch)
        assert ref_closing[0][0] == 0 and ref_closing[1][0] == 0 and ref_closing[0][1] != 0 and ref_closing[1][1] != 0
        polys, closing, zeros = S.logup_polys_replay(air, bad, ch)
        assert polys.tolist() == ref_polys and closing.tolist() == ref_closing and zeros == 0


def test_a_zero_denominator_is_counted_and_its_inverse_is_zero():
    air, blob = logup_air(3, 3, 2)
    _, lookups = R.split_program(blob)
    trace, _ = R.make_trace(3, 3, 2, 64, seed=5)
    cols, table, freq = lookups[0]
    cell = int(trace[9, cols[2]])
    ch = [(P - cell) % P, _challenges(1)[1]]
    ref_polys, ref_closing, ref_zeros = R.polys_and_closing(lookups, 3, trace.tolist(), ch)
    polys, closing, zeros = S.logup_polys_replay(air, trace, ch)
    assert zeros == ref_zeros >= 1
    assert polys.tolist() == ref_polys and closing.tolist() == ref_closing
    # row 9's second helper (the batch of one: column cols[2]) under chi_0 is the inverse of zero
    assert int(polys[1, 9]) == 0
    # ... and the table's: chi_1 = p - a table cell
    ch = [_challenges(2)[0], (P - int(trace[3, table])) % P]
    ref = R.polys_and_closing(lookups, 3, trace.tolist(), ch)
    got = S.logup_polys_replay(air, trace, ch)
    assert got[2] == ref[2] >= 1 and got[0].tolist() == ref[0] and got[1].tolist() == ref[1]


def test_polys_replay_refuses_what_it_should():
    air, _ = logup_air(3, 3, 2)
    trace, _ = R.make_trace(3, 3, 2, 8, 1)
    ch = _challenges(1)
    for args, code in (((S.AIR_TEST_FIBONACCI, np.zeros((8, 2), dtype=np.uint64), ch), S.ERR_BAD_AIR),  # no lookups
                       ((air, trace[:6], ch), S.ERR_BAD_SHAPE),                                          # rows no power of two
                       ((air, trace[:, :5], ch), S.ERR_BAD_SHAPE),                                       # another column count
                       ((air, trace, [P, ch[1]]), S.ERR_BAD_SHAPE),                                      # a challenge that is no field element
                       ((air, trace, ch + [1]), S.ERR_BAD_SHAPE)):                                       # three challenges
        with pytest.raises(S.StarkhipError) as e:
            S.logup_polys_replay(*args)
        assert e.value.code == code


@pytest.mark.parametrize("degree", [2, 3, 5])
def test_eval_frame_logup_is_the_references(degree):
    for m in m_cases(degree):
        air, blob = logup_air(degree, m, 2)
        base, lookups = R.split_program(blob)
        na, cols = S.air_logup_polys(air), S.air_columns(air)
        nl = R.n_constraints(lookups, degree)
        rng = np.random.default_rng(degree + 10 * m)
        for trial in range(2):
            ext = lambda k: rng.integers(0, P, size=(k, 2), dtype=np.uint64)  # noqa: E731
            local, nxt, aux, aux_next, masks, alphas = ext(cols), ext(cols), ext(na), ext(na), ext(4), ext(2)
            pis = rng.integers(0, P, 1, dtype=np.uint64)
            ch = _challenges(10 * degree + trial)
            got = S.air_eval_frame_logup(air, local, nxt, pis, masks, alphas, aux, aux_next, ch)
            tup = lambda a: [(int(x), int(y)) for x, y in a]  # noqa: E731
            mk = tup(masks)
            own = R.own_values_ext(base, tup(local), tup(nxt), pis, mk)
            lc = R.logup_constraints_ext(lookups, degree, tup(local), tup(aux), tup(aux_next), ch)
            assert len(lc) == nl
            want = [R.fold_full(own, lc, mk, a) for a in tup(alphas)]
            assert tup(got) == want
            # the AIR's own part carries alpha^nL: the full fold differs from the plain one exactly by the LogUp constraints
            plain_fold = tup(S.air_eval_frame(air, local, nxt, pis, masks, alphas))
            for j, a in enumerate(tup(alphas)):
                assert want[j] == K.eadd(K.emul(plain_fold[j], K.epow(a, nl)), R.fold_full([], lc, mk, a))


def test_eval_frame_logup_without_lookups_is_eval_frame():
    rng = np.random.default_rng(4)
    ext = lambda k: rng.integers(0, P, size=(k, 2), dtype=np.uint64)  # noqa: E731
    cols = S.air_columns(S.AIR_TEST_FIBONACCI)
    local, nxt, masks, alphas = ext(cols), ext(cols), ext(4), ext(2)
    pis = rng.integers(0, P, S.air_public_inputs(S.AIR_TEST_FIBONACCI), dtype=np.uint64)
    a = S.air_eval_frame(S.AIR_TEST_FIBONACCI, local, nxt, pis, masks, alphas)
    b = S.air_eval_frame_logup(S.AIR_TEST_FIBONACCI, local, nxt, pis, masks, alphas, ext(0), ext(0), _challenges(0))
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ the golden proofs
@pytest.fixture(scope="module")
def golden():
    air, blob, cfg, trace, pis = golden_case()
    return air, blob, cfg, load_golden()


def test_golden_file_is_small_and_its_trace_closes(golden):
    air, blob, cfg, proofs = golden
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "logup_small.json")) < 1 << 20
    _, _, _, trace, _ = golden_case()
    assert trace.shape[0] == 16 and int(blob[3]) == 3 and S.air_logups(air) == 2 and cfg.num_query_rounds == 3


def test_golden_layout(golden):
    air, blob, cfg, proofs = golden
    assert sorted(proofs) == [S.HASHER_POSEIDON, S.HASHER_KECCAK]
    for hasher, proof in proofs.items():
        assert S.proof_hasher(proof) == hasher and int(proof[13]) == 0 and int(proof[14]) == 12
        L = S.proof_layout(proof)
        g = lambda f: int(getattr(L, f))  # noqa: E731
        ncap, C, Q, nA, d0 = 1 << cfg.cap_height, 12, 4, 12, 4 + cfg.rate_bits - cfg.cap_height
        assert (g("n_columns"), g("n_quotient_polys"), g("degree_bits"), g("n_permutation_zs"), g("n_logup_polys"), g("initial_sibling_count")) == (C, Q, 4, 0, nA, d0)
        assert g("off_trace_cap") == 16
        assert g("off_permutation_zs_cap") == 16 + 4 * ncap
        assert g("off_quotient_cap") == 16 + 8 * ncap
        assert g("off_local_values") == 16 + 12 * ncap
        assert g("off_next_values") == g("off_local_values") + 2 * C
        assert g("off_permutation_zs") == g("off_next_values") + 2 * C
        assert g("off_permutation_zs_next") == g("off_permutation_zs") + 2 * nA
        assert g("off_quotient_openings") == g("off_permutation_zs_next") + 2 * nA
        assert g("off_fri_caps") == g("off_quotient_openings") + 2 * Q
        assert (g("q_trace_leaf"), g("q_trace_siblings")) == (0, C)
        assert g("q_permutation_zs_leaf") == C + 4 * d0
        assert g("q_permutation_zs_siblings") == C + 4 * d0 + nA
        assert g("q_quotient_leaf") == C + nA + 8 * d0
        assert g("q_quotient_siblings") == g("q_quotient_leaf") + Q
        assert g("query_round_words") >= C + nA + Q + 12 * d0
        assert g("total_words") == proof.size
        # the hand-off value has the three fields under starky >= 0.2's names, and goes back to the same words
        if hasher == S.HASHER_POSEIDON:
            from starky_bls12_381_amd import handoff
            v = handoff.proof_to_value(proof)
            assert len(v["proof"]["auxiliary_polys_cap"]) == ncap and "permutation_zs_cap" not in v["proof"]
            assert len(v["proof"]["openings"]["auxiliary_polys"]) == nA == len(v["proof"]["openings"]["auxiliary_polys_next"])
            assert "permutation_zs" not in v["proof"]["openings"]
            assert len(v["proof"]["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"]["evals_proofs"]) == 3
            assert np.array_equal(handoff.value_to_proof(v, 4, cfg.rate_bits, cfg.arity_bits), proof)
            assert np.array_equal(handoff.loads(handoff.dumps(proof), 4, cfg.rate_bits, cfg.arity_bits), proof)


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
        bad = logup_flips(proof)
        assert sorted(bad) == ["aux_cap", "aux_leaf", "aux_next_opening", "aux_opening", "aux_sibling"]
        for name, t in bad.items():
            assert cpu_code(air, cfg, t) == S.ERR_VERIFY, (hasher, name)
            assert S.verify_batch_replay([(air, cfg, t)]) == [S.ERR_VERIFY], (hasher, name)
            with pytest.raises(K.Reject):
                R.verify_or_raise(blob, cfg, t, hasher)
        # a batch of the good proof and its tampered copies: the replay gives the CPU verifier's codes, proof by proof
        items = [(air, cfg, proof)] + [(air, cfg, t) for t in bad.values()]
        assert S.verify_batch_replay(items) == [cpu_code(*it) for it in items] == [0] + [S.ERR_VERIFY] * 5


def test_every_opening_of_a_helper_and_of_a_z_matters(golden):
    """each of the nA openings at zeta enters the quotient identity: changing any one is rejected by the C++ and the Python verifier"""
    air, blob, cfg, proofs = golden
    proof = proofs[S.HASHER_POSEIDON]
    off = int(S.proof_layout(proof).off_permutation_zs)
    for i in range(12):
        t = proof.copy()
        t[off + 2 * i] = (int(t[off + 2 * i]) + 1) % P
        assert cpu_code(air, cfg, t) == S.ERR_VERIFY, i
        assert not R.verify(blob, cfg, t, S.HASHER_POSEIDON), i


def test_header_word_14_is_part_of_the_shape(golden):
    air, blob, cfg, proofs = golden
    for proof in proofs.values():
        for v in (0, 2, 11, 13, 1025, 1 << 40):
            t = proof.copy()
            t[14] = v
            assert cpu_code(air, cfg, t) == S.ERR_BAD_SHAPE
            assert S.verify_batch_replay([(air, cfg, t)]) == [S.ERR_BAD_SHAPE]
            with pytest.raises(S.StarkhipError):
                S.proof_layout(t)
        t = proof.copy()  # the count moved to word 13: a proof of Zs, which this AIR has none of
        t[13], t[14] = 12, 0
        assert cpu_code(air, cfg, t) == S.ERR_BAD_SHAPE and S.verify_batch_replay([(air, cfg, t)]) == [S.ERR_BAD_SHAPE]
        assert int(S.proof_layout(t).n_permutation_zs) == 12  # (a layout it does have: the two kinds share the shape)
    # ... and a proof of an AIR without LogUp lookups must say 0 there
    legacy, _ = R.split_program(blob)
    plain_air = S.register_air(legacy)
    assert cpu_code(plain_air, cfg, proofs[0]) == S.ERR_BAD_SHAPE


def _header(C, Q, nZ, nA, L, cap_h, n_queries, log_n=4, rate_bits=2, arity_bits=1, n_pis=3):
    return [0x3130304652505353, C, Q, log_n, rate_bits, cap_h, L, n_queries, 1 << (log_n - L * arity_bits), n_pis, arity_bits, 2, 0, nZ, nA, 0]


def test_a_header_with_both_counts_is_refused():
    for nZ, nA in ((2, 4), (128, 1024), (1, 1)):
        h = _header(6, 4, nZ, nA, 0, 0, 0)
        for mid in (nZ, nA, nZ + nA):  # whichever length one reads it with
            total = 16 + 12 + 2 * (6 + 6 + 2 * mid + 4) + 2 * 16 + 1 + 3
            t = np.zeros(total, dtype=np.uint64)
            t[:16] = h
            with pytest.raises(S.StarkhipError) as e:
                S.proof_layout(t)
            assert e.value.code == S.ERR_BAD_SHAPE


@pytest.mark.parametrize("n_queries", [0, 3])
@pytest.mark.parametrize("cap_h", [0, 2])
@pytest.mark.parametrize("L", [0, 2])
@pytest.mark.parametrize("C,Q,nA", [(2, 2, 0), (6, 4, 4), (6, 8, 18), (0, 2, 0), (0, 0, 4), (3, 2, 1024)])
def test_layout_of_a_bare_header_is_the_documented_walk(C, Q, nA, L, cap_h, n_queries):
    """starkhip_proof_layout reads the header and the length alone: every offset and every q_* field against the field list of the
    layout comment in include/starkhip.h, walked here in its order -- (name, words) of the blob, then of one query round -- with the
    auxiliary polynomials in the Zs' place."""
    h = _header(C, Q, 0, nA, L, cap_h, n_queries)
    log_N, ab, final_len, n_pis = h[3] + h[4], h[10], h[8], h[9]
    ncap, d0 = 1 << cap_h, log_N - cap_h
    depth = [log_N - (l + 1) * ab - cap_h for l in range(L)]
    aux = nA > 0
    round_fields = [("q_trace_leaf", C), ("q_trace_siblings", 4 * d0)]
    round_fields += [("q_permutation_zs_leaf", nA), ("q_permutation_zs_siblings", 4 * d0)] if aux else []
    round_fields += [("q_quotient_leaf", Q), ("q_quotient_siblings", 4 * d0)]
    for l in range(L):
        round_fields += [(("q_step_evals", l), 2 * (1 << ab)), (("q_step_siblings", l), 4 * depth[l])]
    round_words = sum(w for _, w in round_fields)
    blob_fields = [("off_trace_cap", 4 * ncap)] + ([("off_permutation_zs_cap", 4 * ncap)] if aux else []) + [("off_quotient_cap", 4 * ncap)]
    blob_fields += [("off_local_values", 2 * C), ("off_next_values", 2 * C)]
    blob_fields += [("off_permutation_zs", 2 * nA), ("off_permutation_zs_next", 2 * nA)] if aux else []
    blob_fields += [("off_quotient_openings", 2 * Q), ("off_fri_caps", L * 4 * ncap), ("off_query_rounds", n_queries * round_words),
                    ("off_final_poly", 2 * final_len), ("off_pow_witness", 1), ("off_public_inputs", n_pis)]
    want, o = {}, 16
    for name, w in blob_fields:
        want[name], o = o, o + w
    total, o = o, 0
    for name, w in round_fields:
        want[name], o = o, o + w
    want.update(total_words=total, query_round_words=round_words, initial_sibling_count=d0, n_permutation_zs=0, n_logup_polys=nA, n_columns=C,
                n_quotient_polys=Q, degree_bits=h[3], rate_bits=h[4], cap_height=cap_h, n_fri_layers=L, n_query_rounds=n_queries,
                final_poly_len=final_len, n_public_inputs=n_pis, arity_bits=ab)
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
    assert got == {k: want.get(k, 0) for k in got}
    assert set(want) <= set(got)
    for words in (total - 1, total + 1):  # a length one word off
        with pytest.raises(S.StarkhipError):
            S.proof_layout(np.concatenate([blob, np.zeros(1, dtype=np.uint64)])[:words])
    over = blob.copy()
    over[14] = 1025  # nA > 1024 is no header, whatever the length
    for words in (total, total + (1025 - nA) * (4 + n_queries) + (0 if aux else 4 * ncap + 4 * d0 * n_queries)):  # ... the one 1025 polynomials would give too
        t = np.zeros(words, dtype=np.uint64)
        t[:16] = over[:16]
        with pytest.raises(S.StarkhipError):
            S.proof_layout(t)


def test_rust_mirror_has_the_new_names():
    rs = open(os.path.join(ROOT, "bindings", "rust", "starkhip-sys", "src", "lib.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("starkhip_air_logups", "starkhip_air_logup_polys", "starkhip_logup_polys", "starkhip_logup_polys_replay", "starkhip_air_eval_frame_logup"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
    assert re.search(r"\bn_logup_polys\b", hdr) and re.search(r"pub n_logup_polys: usize", rs)
    assert "STARKHIP_AIR_MAX_LOGUP_POLYS 1024u" in hdr and "STARKHIP_AIR_MAX_LOGUP_LOOKUPS 64u" in hdr and "STARKHIP_AIR_MAX_LOGUP_COLUMNS 64u" in hdr
