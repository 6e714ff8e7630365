"""StarkConfigs other than standard_fast on the CPU: the one config rule (starkhip_fri_geometry, FriGeometry::make) against a plain
restatement of plonky2's, the same verdict from the oracle, oracle proofs over a grid of configs checked by the CPU verifier, the
device verifier's CPU replay and the proof parser, tamper sweeps at unusual FRI shapes, and configs every entry point refuses."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from config_cases import CASES, bump, case_air, case_config, case_id, expected_geometry, make_config, qdb_of, sweep_positions


def oracle_rc(blob, cfg, trace_rows, pis):
    """oracle_prove's return code (the proof is freed)."""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    t = np.ascontiguousarray(np.asarray(trace_rows, dtype=np.uint64).T)
    p = np.ascontiguousarray(pis, dtype=np.uint64)
    ocfg = O.OracleConfig(*[getattr(cfg, n) for n, _ in O.OracleConfig._fields_])
    out, words = O._u64p(), C.c_size_t()
    rc = O.lib.oracle_prove(O._p(blob), blob.size, C.byref(ocfg), O._p(t), t.shape[1], O._p(p), 0, C.byref(out), C.byref(words))
    if out:
        O.lib.oracle_free(out)
    return rc


def code_of(fn, *args):
    try:
        fn(*args)
        return 0
    except S.StarkhipError as e:
        return e.code


# ---------------------------------------------------------------------------------------------------------- the rule itself
def test_geometry_table_matches_plonky2():
    """log_n 1..13 x rate 0..9 x cap 0..17 x arity 0..9 x final bits 0..14: acceptance, the arity list and the final polynomial's
    length equal the restatement of plonky2's rule with the header's limits."""
    cfg = make_config(1, 4, 4, 5, 84, 16)
    bad = []
    n_ok = 0
    for log_n in range(1, 14):
        for rate in range(10):
            for cap in range(18):
                for arity in range(10):
                    for final in range(15):
                        cfg.rate_bits, cfg.cap_height, cfg.arity_bits, cfg.final_poly_bits = rate, cap, arity, final
                        want = expected_geometry(cfg, log_n)
                        try:
                            got = S.fri_geometry(cfg, log_n)
                        except S.StarkhipError as e:
                            assert e.code == S.ERR_BAD_SHAPE
                            got = None
                        n_ok += got is not None
                        if got != want and len(bad) < 10:
                            bad.append((f"log_n={log_n}, rate={rate}, cap={cap}, arity={arity}, final={final}", want, got))
    assert not bad, bad
    assert n_ok > 10000


def test_underflow_class_is_refused():
    """The configs whose FRI loop would take degree_bits below zero (plonky2's assert), e.g. log_n=1, rate=1, cap=0, arity=2,
    final=0 -- refused, not a final polynomial of 2^61 and more."""
    for log_n, rate, cap, arity, final in ((1, 1, 0, 2, 0), (3, 2, 0, 5, 0), (7, 1, 0, 2, 0), (13, 4, 0, 8, 0), (2, 5, 3, 4, 1)):
        cfg = make_config(rate, cap, arity, final, 2, 0)
        with pytest.raises(S.StarkhipError) as e:
            S.fri_geometry(cfg, log_n)
        assert e.value.code == S.ERR_BAD_SHAPE, (log_n, rate, cap, arity, final)


def test_other_limits_of_the_rule():
    ok = make_config(1, 4, 4, 5, 84, 16)
    assert S.fri_geometry(ok, 13) == ([4, 4], 32)
    for field, value in (("num_challenges", 1), ("num_challenges", 3), ("rate_bits", 9), ("cap_height", 17), ("arity_bits", 0),
                         ("arity_bits", 9), ("proof_of_work_bits", 65)):
        cfg = make_config(1, 4, 4, 5, 84, 16)
        setattr(cfg, field, value)
        with pytest.raises(S.StarkhipError):
            S.fri_geometry(cfg, 13)
    assert S.fri_geometry(make_config(8, 6, 8, 0, 0, 64), 13) == ([8], 32)    # rate, arity and pow bits at their largest
    assert S.fri_geometry(make_config(8, 16, 8, 0, 0, 64), 13) == ([], 8192)  # and the cap
    assert S.fri_geometry(make_config(1, 14, 4, 5, 0, 0), 13) == ([], 8192)  # cap_height == log_N: no layers
    with pytest.raises(S.StarkhipError):
        S.fri_geometry(make_config(1, 15, 4, 5, 0, 0), 13)                    # cap_height > log_N


def test_oracle_gives_the_same_verdict():
    """oracle_prove refuses exactly the configs the rule refuses (every refused one of the table on a degree-2 AIR, so that rate 0
    has no quotient objection) and proves the ones it accepts with the rule's geometry (a sample, one query, no grinding)."""
    traces = {}
    from random_air import random_air
    cfg = make_config(1, 4, 4, 5, 1, 0)
    bad = []
    k = 0
    for log_n in range(1, 14):
        if log_n not in traces:
            traces[log_n] = random_air(40 + log_n, 2, 2, 1 << log_n)
        blob, t, pis = traces[log_n]
        for rate in range(10):
            for cap in range(18):
                for arity in range(10):
                    for final in range(15):
                        cfg.rate_bits, cfg.cap_height, cfg.arity_bits, cfg.final_poly_bits = rate, cap, arity, final
                        want = expected_geometry(cfg, log_n)
                        if want is None:
                            rc = oracle_rc(blob, cfg, t, pis)
                            if rc != S.ERR_BAD_SHAPE:
                                bad.append((log_n, rate, cap, arity, final, rc))
                            continue
                        k += 1
                        if log_n > 6 or rate > 3 or k % 37:
                            continue
                        proof = O.prove(blob, cfg, t.T.copy(), pis)
                        L = S.proof_layout(proof)
                        got = ([int(arity)] * int(L.n_fri_layers), int(L.final_poly_len))
                        if got != want:
                            bad.append((log_n, rate, cap, arity, final, got, want))
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------------------------------------- proofs at the grid
def test_config_grid_covers_the_required_values():
    seen = {k: set() for k in ("rate", "cap", "arity", "final", "nq", "pow", "log_n", "cols", "diff1", "diff2")}
    last_depth_zero = no_layers_full_cap = False
    for case in CASES:
        air, log_n, rate, cap, arity, final, nq, pw = case
        cols, degree = (4, 3) if air == "fib" else air[1:]
        ar, _ = expected_geometry(case_config(case), log_n)
        for k, v in (("rate", rate), ("cap", cap), ("arity", arity), ("nq", nq), ("pow", pw), ("log_n", log_n), ("cols", cols)):
            seen[k].add(v)
        seen["final"].add("ge" if final >= log_n else final)
        if qdb_of(degree) in (1, 2):
            seen[f"diff{qdb_of(degree)}"].add(rate - qdb_of(degree))
        assert rate > 0 or degree == 2
        last_depth_zero |= bool(ar) and log_n + rate - sum(ar) == cap
        no_layers_full_cap |= not ar and cap == log_n + rate
    assert {0, 1, 2, 3, 4, 5} <= seen["rate"] and {0, 1, 4} <= seen["cap"] and {1, 2, 3, 5, 6} <= seen["arity"]
    assert {0, 2, "ge"} <= seen["final"] and {0, 1, 2, 28, 150} <= seen["nq"] and {0, 1, 8, 20} <= seen["pow"]
    assert {1, 3, 7, 8, 10, 13} <= seen["log_n"] and {1, 4, 5} <= seen["cols"] and max(seen["cols"]) >= 300
    assert {0, 1, 2, 3} <= seen["diff1"] and {0, 1, 2, 3} <= seen["diff2"]
    assert last_depth_zero and no_layers_full_cap


_PROOFS = {}


def grid_proof(case):
    if case not in _PROOFS:
        air, blob, t, pis, _ = case_air(case)
        _PROOFS[case] = O.prove(blob, case_config(case), t.T.copy(), pis)
    return _PROOFS[case]


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_oracle_proof_at_config_is_accepted_by_every_verifier(case):
    air, blob, t, pis, _ = case_air(case)
    cfg = case_config(case)
    log_n = case[1]
    proof = grid_proof(case)
    S.verify_stark_proof(air, cfg, proof)
    assert S.verify_batch_replay([(air, cfg, proof)]) == [0]
    arities, final_len = S.fri_geometry(cfg, log_n)
    L = S.proof_layout(proof)
    log_N = log_n + cfg.rate_bits
    assert (int(L.degree_bits), int(L.rate_bits), int(L.cap_height), int(L.arity_bits)) == (log_n, cfg.rate_bits, cfg.cap_height, cfg.arity_bits)
    assert int(L.n_fri_layers) == len(arities) and int(L.final_poly_len) == final_len and int(L.n_query_rounds) == cfg.num_query_rounds
    assert int(L.initial_sibling_count) == log_N - cfg.cap_height
    depths = [log_N - sum(arities[:l + 1]) - cfg.cap_height for l in range(len(arities))]
    assert [int(L.step_sibling_count[l]) for l in range(len(arities))] == depths
    C_, Q = int(L.n_columns), int(L.n_quotient_polys)
    want_qw = C_ + Q + 8 * (log_N - cfg.cap_height) + sum(2 * (1 << a) + 4 * d for a, d in zip(arities, depths))
    assert int(L.query_round_words) == want_qw
    ncap = 1 << cfg.cap_height
    words = 16 + 8 * ncap + 4 * C_ + 2 * Q + len(arities) * 4 * ncap + cfg.num_query_rounds * want_qw + 2 * final_len + 1 + pis.size
    assert int(L.total_words) == proof.size == words
    if cfg.proof_of_work_bits:  # the witness the oracle ground satisfies the stated bits and the rule is what the verifier checked
        assert int(L.off_pow_witness) == proof.size - 1 - pis.size


# ---------------------------------------------------------------------------------------------------------- tamper sweeps
# arity 1 and 5, cap 0 and the largest cap (a FRI layer without siblings); every one with log_N >= 5, so that a changed PoW witness
# cannot give the same query indices by chance
SWEEP = [CASES[i] for i in (3, 5, 8, 19, 26, 20)]


@pytest.mark.parametrize("case", SWEEP, ids=[case_id(c) for c in SWEEP])
def test_tamper_sweep_cpu_verifier_and_replay_agree(case):
    air, _, _, _, _ = case_air(case)
    cfg = case_config(case)
    proof = grid_proof(case)
    pos = sweep_positions(proof)
    items = [(air, cfg, bump(proof, p)) for p in pos]
    want = [code_of(S.verify_stark_proof, *it) for it in items]
    assert all(w != 0 for w in want), [p for p, w in zip(pos, want) if w == 0]
    assert S.verify_batch_replay(items + [(air, cfg, proof)]) == want + [0]


def test_sweep_covers_the_shapes_it_should():
    arities = {c[4] for c in SWEEP}
    caps = {c[3] for c in SWEEP}
    assert {1, 5} <= arities and 0 in caps
    assert any(expected_geometry(case_config(c), c[1])[0] and c[1] + c[2] - sum(expected_geometry(case_config(c), c[1])[0]) == c[3]
               for c in SWEEP)  # a case at the largest cap: a FRI layer with no siblings


# ---------------------------------------------------------------------------------------------------------- refused configs
def refused_configs():
    """(name, base case, config changes): each changes a neighbouring grid case into a config every entry point refuses."""
    fib = ("fib", 7, 2, 3, 2, 0, 28, 8)
    d2 = ((12, 4, 2), 3, 0, 1, 2, 0, 28, 1)
    d5 = ((16, 5, 5), 7, 3, 4, 2, 0, 28, 0)
    return [
        ("underflow_fib", fib, dict(cap_height=0, final_poly_bits=0)),               # 7 -> 5 -> 3 -> 1, then arity 2 > 1
        ("underflow_d2", d2, dict(rate_bits=1, cap_height=0, final_poly_bits=0)),     # 3 -> 1, then 1 + 1 - 2 >= 0 with arity 2 > 1
        ("underflow_arity5", d5, dict(arity_bits=5, cap_height=0)),                   # 7 -> 2, then 2 + 3 - 5 >= 0 with arity 5 > 2
        ("arity0", fib, dict(arity_bits=0)),
        ("arity9", fib, dict(arity_bits=9)),
        ("challenges1", fib, dict(num_challenges=1)),
        ("challenges3", fib, dict(num_challenges=3)),
        ("cap_above_log_N", fib, dict(cap_height=10)),
        ("qdb_above_rate", d5, dict(rate_bits=1)),
        ("rate9", d2, dict(rate_bits=9)),
        ("cap17", fib, dict(cap_height=17)),
        ("pow65", fib, dict(proof_of_work_bits=65)),
    ]


@pytest.mark.parametrize("name,base,change", refused_configs(), ids=[r[0] for r in refused_configs()])
def test_refused_config_is_bad_shape_everywhere(name, base, change):
    air, blob, t, pis, degree = case_air(base)
    proof = grid_proof(base)
    cfg = case_config(base)
    for k, v in change.items():
        setattr(cfg, k, v)
    geo = expected_geometry(cfg, base[1])
    assert geo is None or qdb_of(degree) > cfg.rate_bits, name
    if geo is None:
        assert code_of(S.fri_geometry, cfg, base[1]) == S.ERR_BAD_SHAPE
    assert code_of(S.verify_stark_proof, air, cfg, proof) == S.ERR_BAD_SHAPE
    assert S.verify_batch_replay([(air, cfg, proof), (air, case_config(base), proof)]) == [S.ERR_BAD_SHAPE, 0]
    assert oracle_rc(blob, cfg, t, pis) == S.ERR_BAD_SHAPE


def test_pow_bits_are_checked_before_the_proof_is_read():
    """A proof's header does not carry proof_of_work_bits: 64 is the largest a verifier can test (the whole response zero) and
    65 is refused as a config, not shifted by a negative amount."""
    base = ("fib", 7, 2, 3, 2, 0, 28, 8)
    air = case_air(base)[0]
    proof = grid_proof(base)
    cfg = case_config(base)
    cfg.proof_of_work_bits = 64
    assert code_of(S.verify_stark_proof, air, cfg, proof) == S.ERR_VERIFY
    cfg.proof_of_work_bits = 65
    assert code_of(S.verify_stark_proof, air, cfg, proof) == S.ERR_BAD_SHAPE
