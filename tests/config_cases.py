"""StarkConfigs away from standard_fast, shared by the CPU and GPU config tests: a plain restatement of plonky2's FRI reduction
rule, and a grid of small proofs that between them take every FRI arity, cap height, rate, query count and proof-of-work setting
the tests name.  Test code."""
import random

import numpy as np

import starky_bls12_381_amd as S
from random_air import random_air
from starky_bls12_381_amd.air_builder import AirBuilder


def plonky2_reduction_arity_bits(log_n, rate_bits, cap_height, arity_bits, final_poly_bits):
    """plonky2 FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits).reduction_arity_bits, over Python's integers:
    the list of arity bits, or None where its assert!(degree_bits >= arity_bits) fires."""
    result = []
    degree_bits = log_n
    while degree_bits > final_poly_bits and degree_bits + rate_bits - arity_bits >= cap_height:
        result.append(arity_bits)
        if degree_bits < arity_bits:
            return None
        degree_bits -= arity_bits
    return result


def expected_geometry(cfg, log_n):
    """(arities, final_poly_len) the project accepts for `cfg` at 2^log_n rows, or None (include/starkhip.h, starkhip_config_t)."""
    if cfg.num_challenges != 2 or cfg.rate_bits > 8 or cfg.cap_height > 16 or not 1 <= cfg.arity_bits <= 8 or \
            cfg.proof_of_work_bits > 64 or log_n + cfg.rate_bits < cfg.cap_height:
        return None
    ar = plonky2_reduction_arity_bits(log_n, cfg.rate_bits, cfg.cap_height, cfg.arity_bits, cfg.final_poly_bits)
    if ar is None or len(ar) > 16:
        return None
    return ar, 1 << (log_n - sum(ar))


def make_config(rate, cap, arity, final, queries, pow_bits, challenges=2):
    cfg = S.StarkConfig.standard_fast_config()
    cfg.num_challenges, cfg.rate_bits, cfg.cap_height, cfg.arity_bits = challenges, rate, cap, arity
    cfg.final_poly_bits, cfg.num_query_rounds, cfg.proof_of_work_bits = final, queries, pow_bits
    return cfg


def qdb_of(degree):
    factor = max(degree - 1, 1)
    return (factor - 1).bit_length()


# (air, log_n, rate_bits, cap_height, arity_bits, final_poly_bits, num_query_rounds, proof_of_work_bits); air is "fib" (the
# Fibonacci toy AIR: 4 columns, degree 3) or (seed, columns, degree) of tests/random_air.py.  Chosen so that every value the
# config tests require appears, each in several different combinations with the others: rate 0..5 (rate - qdb 0..3 at qdb 1 and
# 2), cap 0 / 1 / 4 / the largest the rule allows (a last FRI layer of path depth 0) / log_N with no FRI layers, arity 1 2 3 5 6,
# final bits 0 / 2 / >= log_n, queries 0 1 2 28 150, pow bits 0 1 8 20, log_n 1 3 7 8 10 13, columns 1 4 5 300.
CASES = [
    ((11, 1, 2), 1, 0, 0, 1, 0, 2, 0),
    ((12, 4, 2), 3, 0, 1, 2, 0, 28, 1),
    ((13, 5, 2), 8, 1, 4, 3, 2, 1, 8),
    ((14, 300, 2), 7, 2, 0, 5, 0, 2, 0),
    ("fib", 3, 1, 4, 2, 3, 2, 0),
    ("fib", 7, 2, 3, 2, 0, 28, 8),
    ("fib", 8, 1, 1, 3, 2, 150, 0),
    ("fib", 10, 3, 4, 6, 0, 2, 1),
    ("fib", 3, 4, 0, 1, 0, 1, 0),
    ((15, 4, 4), 3, 2, 1, 1, 2, 2, 0),
    ((16, 5, 5), 7, 3, 4, 2, 0, 28, 0),
    ((17, 300, 4), 3, 4, 4, 2, 0, 1, 0),
    ((18, 1, 5), 8, 5, 0, 3, 2, 2, 20),
    ((19, 4, 2), 13, 1, 4, 3, 5, 2, 0),
    ((20, 4, 5), 10, 2, 1, 2, 2, 1, 0),
    ((21, 4, 4), 1, 2, 3, 2, 0, 2, 0),
    ((22, 1, 2), 10, 0, 0, 6, 0, 150, 0),
    ("fib", 8, 2, 1, 5, 0, 0, 8),
    ((23, 4, 2), 7, 0, 0, 2, 0, 0, 0),
    ((24, 300, 5), 3, 5, 7, 1, 2, 2, 1),
    ((25, 1, 4), 10, 3, 0, 1, 5, 1, 0),
    ("fib", 10, 1, 0, 2, 2, 2, 0),
    ((26, 300, 2), 8, 1, 4, 4, 5, 2, 0),
    ((27, 4, 5), 13, 2, 4, 4, 5, 1, 0),
    ((28, 1, 2), 3, 1, 0, 6, 0, 28, 0),
    ("fib", 7, 5, 4, 3, 0, 2, 1),
    ((29, 5, 4), 8, 2, 2, 5, 0, 2, 0),
    ((30, 5, 2), 1, 3, 2, 1, 0, 150, 0),
    ((31, 5, 2), 13, 0, 0, 2, 14, 2, 0),
    ((32, 4, 3), 7, 1, 0, 2, 3, 28, 8),
]


def case_id(case):
    air, log_n, rate, cap, arity, final, nq, pw = case
    name = "fib" if air == "fib" else f"c{air[1]}d{air[2]}"
    return f"{name}-n{log_n}-r{rate}-cap{cap}-a{arity}-f{final}-q{nq}-pow{pw}"


_AIRS = {}


def case_air(case):
    """(air id, program blob, row-major trace, public inputs, degree) of a case; random AIRs are registered once per process."""
    air, log_n = case[0], case[1]
    key = (air, log_n)
    if key not in _AIRS:
        if air == "fib":
            t, pis = S.trace_fibonacci(3, 5, 1 << log_n)
            _AIRS[key] = (S.AIR_TEST_FIBONACCI, S.air_program(S.AIR_TEST_FIBONACCI), t, pis, 3)
        else:
            seed, cols, degree = air
            blob, t, pis = random_air(seed, cols, degree, 1 << log_n)
            _AIRS[key] = (S.register_air(blob, name=f"cfg{seed}"), blob, t, pis, degree)
    return _AIRS[key]


def case_config(case):
    return make_config(*case[2:])


def small_cell_air(n_cols, degree, log_n, seed):
    """(blob, row-major trace, public inputs) of an AIR over 0/1 columns -- every cell fits the 32 bits a trace recording holds:
    each column boolean, a transition tying column 0 to the last column, and a product of degree `degree` that the booleans zero."""
    assert n_cols >= degree >= 2
    n = 1 << log_n
    rng = random.Random(seed)
    t = np.array([[rng.randrange(2) for _ in range(n_cols)] for _ in range(n)], dtype=np.uint64)
    t[:, n_cols - 1] = np.roll(t[:, 0], -1)
    b = AirBuilder(n_cols, 1, degree)
    one = AirBuilder.one()
    for c in range(n_cols):
        b.constraint(b.L(c) * (one - b.L(c)))
    b.transition(b.N(0) - b.L(n_cols - 1))
    e = b.L(0) * (one - b.L(0))
    for c in range(1, degree - 1):
        e = e * b.L(c)
    b.constraint(e)
    b.first_row(b.L(1) - b.PI(0))
    return b.finish(), t, np.array([int(t[0, 1])], dtype=np.uint64)


def sweep_positions(proof):
    """One word of each section: both caps, the three openings, every FRI cap, every kind of word of one query round (trace leaf
    and siblings, quotient leaf and siblings, each FRI layer's evaluations and siblings), the final polynomial, the PoW witness and
    a public input."""
    L = S.proof_layout(proof)
    g = lambda f: int(getattr(L, f))  # noqa: E731
    pos = [g("off_trace_cap") + 1, g("off_quotient_cap") + 2, g("off_local_values"), g("off_next_values") + 1,
           g("off_quotient_openings") + 1]
    pos += [g("off_fri_caps") + 4 * (1 << g("cap_height")) * l + 3 for l in range(g("n_fri_layers"))]
    nq = g("n_query_rounds")
    if nq:
        base = g("off_query_rounds") + (nq // 2) * g("query_round_words")
        pos += [base + g("q_trace_leaf"), base + g("q_trace_leaf") + g("n_columns") - 1, base + g("q_quotient_leaf")]
        pos += [base + g("q_trace_siblings") + k for k in range(0, 4 * g("initial_sibling_count"), 3)]
        pos += [base + g("q_quotient_siblings") + k for k in range(0, 4 * g("initial_sibling_count"), 5)]
        for l in range(g("n_fri_layers")):
            pos += [base + int(L.q_step_evals[l]), base + int(L.q_step_evals[l]) + (2 << g("arity_bits")) - 1]
            pos += [base + int(L.q_step_siblings[l]) + k for k in range(0, 4 * int(L.step_sibling_count[l]), 3)]
    pos += [g("off_final_poly"), g("off_final_poly") + 2 * g("final_poly_len") - 1, g("off_pow_witness")]
    if g("n_public_inputs"):
        pos.append(g("off_public_inputs"))
    return pos


def bump(proof, p):
    bad = proof.copy()
    bad[p] = (int(bad[p]) + 1) % S.P
    return bad
