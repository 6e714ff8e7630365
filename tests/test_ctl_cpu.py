"""Cross-table lookups (COMPAT.md §2d) without a GPU: every refusal of a system's registration with its reason; the host replay of the
CTL polynomials and the constraint fold over an extension frame against the Python reference of tests/ctl_ref.py, word for word; the
golden system proofs (tests/golden/ctl_small.json, one per hasher) through the CPU system verifier and the Python mini-verifier, intact
and tampered with; a lone table proof at the single-proof verifier."""
import numpy as np
import pytest

import ctl_ref as X
import logup_columns_ref as G
import logup_ref as R
import starky_bls12_381_amd as S
from ctl_util import configs, cpu_code, ctl_system, golden_case, golden_two_case, load_golden, system_blob
from starky_bls12_381_amd.air_builder import AirBuilder, Column, Filter, SystemBuilder

P = X.P
CASES = sorted(X.CASES)


def _rows(name):
    return {"two_lookers": (8, 16, 4), "chain": (16, 8, 4)}.get(name, (16, 8))


# ------------------------------------------------------------------------------------------------ registration
def _air(n_cols=5, degree=2, pairs=False):
    b = AirBuilder(n_cols, 1, degree)
    if degree == 1:
        b.transition(b.N(0) - b.L(0) - 1)
    else:
        G.own_constraints(b, degree)
    if pairs:
        b.permutation_pair([(3, 4)])
    return S.register_air(b.finish())


def test_every_refusal_names_its_reason():
    a, wide = _air(), _air(7, 3)
    ok = SystemBuilder([a, wide])
    ok.ctl((1, [3], Filter(sums=[4])), [(0, [3], None)])
    assert S.system_check(ok.finish()) is None
    sid = S.register_system(ok.finish())
    assert S.register_system(ok.finish()) == sid and S.system_tables(sid) == [a, wide] and S.system_ctls(sid) == 1
    assert [S.system_table_endpoints(sid, t) for t in range(2)] == [1, 1]

    def why(tables, ctls, patch=None):
        sb = SystemBuilder(tables)
        for looked, looking in ctls:
            sb.ctl(looked, looking)
        blob = sb.finish()
        if patch:
            blob = patch(blob)
        reason = S.system_check(blob)
        assert reason is not None
        with pytest.raises(S.StarkhipError) as e:
            S.register_system(blob)
        assert e.value.code == S.ERR_BAD_AIR
        return reason
    one = [((1, [3], None), [(0, [3], None)])]
    assert "not a registered AIR" in why([a, 999999], one)  # table ids
    assert "not a registered AIR" in why([a, S.AIR_TEST_FIBONACCI], one)  # (a built-in AIR is no table)
    assert "2..64" in why([a], [])
    assert "table 2 out of range" in why([a, wide], [((2, [3], None), [(0, [3], None)])])

    def narrow(blob):  # the looking endpoint declares one column fewer than the CTL's width
        w = [int(x) for x in blob]
        at = 2 + 2 + 1 + 2  # magic, T, ids, K, (width, L)
        looked_len = 2 + 2 * 4 + 1
        assert w[at + looked_len + 1] == 2
        w[at + looked_len + 1] = 1
        return np.array(w, dtype=np.uint64)
    assert "width mismatch" in why([a, wide], [((1, [3, 4], None), [(0, [3, 4], None)])], narrow)
    assert "column 5 out of range" in why([a, wide], [((1, [3], None), [(0, [5], None)])])  # against each table's own n_cols
    assert S.system_check(system_blob([a, wide], [((1, [X.plain(6)], ([], [])), [(0, [X.plain(4)], ([], []))])])) is None
    assert "column 6 out of range" in why([a, wide], [((1, [3], None), [(0, [3], Filter(sums=[6]))])])
    many = Column([(k % 5, 1) for k in range(17)])
    assert "17 terms" in why([a, wide], [((1, [many], None), [(0, [3], None)])])  # the term limits
    assert "5 products" in why([a, wide], [((1, [3], Filter(products=[(3, 4)] * 5)), [(0, [3], None)])])
    assert "5 sums" in why([a, wide], [((1, [3], Filter(sums=[3] * 5)), [(0, [3], None)])])
    assert "nA + nC above 1024" in why([a, wide], [((1, [3], None), [(0, [3], None)] * 64)] * 5)  # 320 endpoints of table 0: 1280 polynomials
    assert "degree >= 2" in why([a, _air(5, 1)], one)
    assert "permutation pairs" in why([a, _air(5, 3, pairs=True)], one)
    assert "trailing words" in why([a, wide], one, lambda b: np.concatenate([b, np.zeros(1, dtype=np.uint64)]))
    assert "past the blob" in why([a, wide], one, lambda b: b[:-1])
    assert "bad magic" in why([a, wide], one, lambda b: np.concatenate([[np.uint64(1)], b[1:]]).astype(np.uint64))


# ------------------------------------------------------------------------------------------------ the host mirror against the reference
@pytest.mark.parametrize("name", CASES)
def test_the_reference_traces_balance(name):
    case = X.CASES[name]
    traces = X.make_traces(case, _rows(name), seed=3)
    sums_of = []
    for t in range(len(case.tables)):
        _, sums, zeros = X.polys_and_sums(X.table_endpoints(case.ctls, t), traces[t][0].tolist(), X.CHALLENGES)
        assert zeros == 0
        sums_of.append(sums)
    assert X.first_unbalanced(case.ctls, sums_of) == -1
    sums_of[0][0] = (sums_of[0][0] + 1) % P
    assert X.first_unbalanced(case.ctls, sums_of) == 0


@pytest.mark.parametrize("name", CASES)
def test_polys_replay_word_for_word(name):
    system, airs, _, case = ctl_system(name)
    traces = X.make_traces(case, _rows(name), seed=4)
    for t in range(len(airs)):
        eps = X.table_endpoints(case.ctls, t)
        assert S.system_table_endpoints(system, t) == len(eps)
        trace = traces[t][0].copy()
        trace[::3, 3:] += np.uint64(P)  # cells at or above p are read mod p (every value behind column 2 is small)
        want = X.polys_and_sums(eps, trace.tolist(), X.CHALLENGES)
        for layout, arg in ((0, trace), (1, np.ascontiguousarray(trace.T))):
            polys, sums, zeros = S.ctl_polys_replay(system, t, arg, X.CHALLENGES, layout=layout)
            assert np.array_equal(polys, np.array(want[0], dtype=np.uint64)) and sums.tolist() == want[1] and zeros == want[2] == 0


def test_polys_replay_counts_zero_denominators():
    system, _, _, case = ctl_system("range")
    trace = X.make_traces(case, (16, 8), seed=5)[0][0]
    chal = list(X.CHALLENGES)
    chal[1] = (P - int(trace[5, 3])) % P  # gamma_0 = -value of row 5: every row holding that value has a zero denominator under challenge 0
    hits = int((trace[:, 3] == trace[5, 3]).sum())
    want = X.polys_and_sums(X.table_endpoints(case.ctls, 0), trace.tolist(), chal)
    polys, sums, zeros = S.ctl_polys_replay(system, 0, trace, chal)
    assert zeros == want[2] == hits and int(polys[0, 5]) == 0 and np.array_equal(polys, np.array(want[0], dtype=np.uint64)) and sums.tolist() == want[1]


@pytest.mark.parametrize("name", CASES)
def test_eval_frame_ctl_word_for_word(name):
    system, airs, blobs, case = ctl_system(name)
    rng = np.random.default_rng(11)
    ext = lambda k: rng.integers(0, P, size=(k, 2), dtype=np.uint64)  # noqa: E731
    for t, air in enumerate(airs):
        eps = X.table_endpoints(case.ctls, t)
        head, lookups = G.split_program(blobs[t])
        degree, nA, nC = case.tables[t].degree, S.air_logup_polys(air), 4 * len(eps)
        assert nA == G.n_polys(lookups, degree)
        local, nxt, masks, alphas, aux, auxn = ext(case.tables[t].n_cols), ext(case.tables[t].n_cols), ext(4), ext(2), ext(nA + nC), ext(nA + nC)
        pis, chis = ext(1)[0][:1], [int(x) for x in ext(1)[0]]
        sums = [int(x) for x in rng.integers(0, P, size=nC // 2, dtype=np.uint64)]
        tup = lambda a: [(int(x), int(y)) for x, y in a]  # noqa: E731
        own = R.own_values_ext(head, tup(local), tup(nxt), pis, tup(masks))
        lc = G.logup_constraints_ext(lookups, degree, tup(local), tup(nxt), tup(aux[:nA]), tup(auxn[:nA]), chis) if nA else []
        cc = X.ctl_constraints_ext(eps, tup(local), tup(nxt), tup(aux[nA:]), tup(auxn[nA:]), X.CHALLENGES, sums)
        assert len(cc) == 8 * len(eps)
        want = [X.fold_all(own, lc, cc, tup(masks), (int(a), int(b))) for a, b in alphas]
        got = S.system_eval_frame_ctl(system, t, local, nxt, pis, masks, alphas, aux, auxn, chis, X.CHALLENGES, sums)
        assert tup(got) == want


# ------------------------------------------------------------------------------------------------ the golden proofs
def _other_golden():
    return load_golden("other_proofs_hex")


@pytest.mark.parametrize("hasher", [S.HASHER_POSEIDON, S.HASHER_KECCAK])
def test_golden_system_proofs_verify(hasher):
    system, blobs, case, cfgs, _ = golden_case()
    proof = load_golden()[hasher]
    tables = S.system_proof_tables(proof)
    assert [int(t[15]) for t in tables] == [4, 4] and [int(S.proof_layout(t).n_ctl_polys) for t in tables] == [4, 4]
    assert all(int(S.proof_layout(t).off_ctl_sums) == t.size - 2 for t in tables)
    assert cpu_code(system, cfgs, proof) == 0
    X.verify_system_or_raise(blobs, case.ctls, cfgs, proof, hasher)
    assert np.array_equal(S.system_proof_join(tables), proof)


def _tampered(proof, other):
    """{name: a system proof both verifiers must reject}"""
    tables = [t.copy() for t in S.system_proof_tables(proof)]
    lay = [S.proof_layout(t) for t in tables]

    def with_words(changes):
        ts = [t.copy() for t in tables]
        for t, pos, delta in changes:
            ts[t][pos] = (int(ts[t][pos]) + delta) % P
        return S.system_proof_join(ts)
    s0, s1 = int(lay[0].off_ctl_sums), int(lay[1].off_ctl_sums)
    out = {"a sum changed": with_words([(0, s0, 1)]),
           # the looking sum and the looked sum moved alike: the CTL still balances, the last-row constraints do not hold
           "balanced shift of two sums": with_words([(0, s0, 5), (1, s1, 5), (0, s0 + 1, 5), (1, s1 + 1, 5)]),
           "two table proofs swapped": S.system_proof_join([tables[1], tables[0]]),
           "a table proof from a run with another table trace": S.system_proof_join([S.system_proof_tables(other)[0], tables[1]]),
           "an auxiliary opening changed": with_words([(0, int(lay[0].off_permutation_zs) + 2, 1)])}
    bad = [t.copy() for t in tables]
    bad[0][15] = 8
    out["nC changed"] = S.system_proof_join(bad)
    return out


@pytest.mark.parametrize("hasher", [S.HASHER_POSEIDON, S.HASHER_KECCAK])
def test_tampered_system_proofs_are_rejected_by_both_verifiers(hasher):
    system, blobs, case, cfgs, _ = golden_case()
    proof, other = load_golden()[hasher], _other_golden()[hasher]
    assert cpu_code(system, cfgs, other) == 0  # the other run is a good proof of its own
    assert np.array_equal(S.system_proof_tables(proof)[0][-3:-2], S.system_proof_tables(other)[0][-3:-2])  # ... of the same looking trace (its public input)
    for name, bad in _tampered(proof, other).items():
        assert cpu_code(system, cfgs, bad) in (S.ERR_VERIFY, S.ERR_BAD_SHAPE), name
        assert not X.verify_system(blobs, case.ctls, cfgs, bad, hasher), name


@pytest.mark.parametrize("hasher", [S.HASHER_POSEIDON, S.HASHER_KECCAK])
def test_plus_delta_on_one_looking_sum_and_minus_delta_on_another(hasher):
    """the balance holds, a last-row constraint of each of the two tables does not -- and the sums are bound in each table's transcript,
    so whichever check comes first fails: both verifiers reject"""
    system, blobs, case, cfgs, _ = golden_two_case()
    proof = load_golden("two_lookers_proofs_hex")[hasher]
    assert cpu_code(system, cfgs, proof) == 0
    X.verify_system_or_raise(blobs, case.ctls, cfgs, proof, hasher)
    tables = [t.copy() for t in S.system_proof_tables(proof)]
    for t, delta in ((0, 9), (1, P - 9)):  # under both challenges
        at = int(S.proof_layout(tables[t]).off_ctl_sums)
        for i in range(2):
            tables[t][at + i] = (int(tables[t][at + i]) + delta) % P
    bad = S.system_proof_join(tables)
    sums_of = [[int(x) for x in t[int(S.proof_layout(t).off_ctl_sums):]] for t in tables]
    assert X.first_unbalanced(case.ctls, sums_of) == -1  # the CTL still balances
    assert cpu_code(system, cfgs, bad) == S.ERR_VERIFY and not X.verify_system(blobs, case.ctls, cfgs, bad, hasher)


@pytest.mark.parametrize("hasher", [S.HASHER_POSEIDON, S.HASHER_KECCAK])
def test_a_lone_table_proof_is_bad_shape(hasher):
    system, _, _, cfgs, _ = golden_case()
    airs = S.system_tables(system)
    for t, table in enumerate(S.system_proof_tables(load_golden()[hasher])):
        with pytest.raises(S.StarkhipError) as e:
            S.verify_stark_proof(airs[t], cfgs[t], table)
        assert e.value.code == S.ERR_BAD_SHAPE
        assert S.verify_batch_replay([(airs[t], cfgs[t], table)]) == [S.ERR_BAD_SHAPE]


def test_system_configs_may_differ_in_rate_bits_only():
    system, _, _, cfgs, _ = golden_case()
    proof = load_golden()[S.HASHER_POSEIDON]
    other = [cfgs[0], S.StarkConfig.standard_fast_config()]
    other[1].num_query_rounds = 4
    assert cpu_code(system, other, proof) == S.ERR_BAD_SHAPE
