"""CPU tests of the device verifier's host side (starkhip_verify_batch_replay): the same preludes, chunks, leaf descriptors and
per-query routine (csrc/verify_query.h) as starkhip_verify_batch, with the device's part replayed on the CPU.  Every proof's code
must be exactly the CPU verifier's (starkhip_verify)."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AIR = S.AIR_TEST_FIBONACCI
SHAPES = [(16, 1), (64, 1), (64, 2), (1024, 2), (1024, 1)]  # test_toy_air_cpu.py::test_oracle_proof_is_accepted_by_product_verifier


def _case(n, rate_bits):
    cfg = S.StarkConfig.standard_fast_config()
    cfg.rate_bits = rate_bits
    t, pis = S.trace_fibonacci(3, 5, n)
    return cfg, O.prove(S.air_program(AIR), cfg, S.trace_rows_to_poly_values(t), pis)


def _cpu_code(air, cfg, proof):
    try:
        S.verify_stark_proof(air, cfg, proof)
        return 0
    except S.StarkhipError as e:
        return e.code


def _layout(proof):
    L = S.proof_layout(proof)
    return {f: int(getattr(L, f)) for f in ("off_trace_cap", "off_query_rounds", "query_round_words", "n_query_rounds", "off_final_poly",
                                            "off_pow_witness")}


@pytest.mark.parametrize("n,rate_bits", SHAPES)
def test_replay_accepts_oracle_proofs(n, rate_bits):
    cfg, proof = _case(n, rate_bits)
    assert S.verify_batch_replay([(AIR, cfg, proof)]) == [0]


def test_replay_matches_cpu_verifier_on_a_mixed_batch():
    items = [(AIR,) + _case(n, rb) for n, rb in SHAPES]
    cfg, proof = _case(64, 2)
    rng = np.random.default_rng(5)
    # test_toy_air_cpu.py::test_verifier_rejects_tampering_everywhere's positions: caps, openings, queries, final poly, pow, public inputs
    positions = list(range(16, 16 + 160, 13)) + [int(x) for x in rng.integers(16, proof.size, size=40)] + [proof.size - 1, proof.size - 4]
    for pos in positions:
        bad = proof.copy()
        bad[pos] = (int(bad[pos]) + 1) % S.P
        items.append((AIR, cfg, bad))
    L = _layout(proof)
    q0 = L["off_query_rounds"]
    # every kind of word of one query round, and one of the last round
    for off in range(0, L["query_round_words"], 3):
        bad = proof.copy()
        bad[q0 + off] = (int(bad[q0 + off]) + 1) % S.P
        items.append((AIR, cfg, bad))
    last = q0 + (L["n_query_rounds"] - 1) * L["query_round_words"]
    bad = proof.copy()
    bad[last] = (int(bad[last]) + 1) % S.P
    items.append((AIR, cfg, bad))
    # a word >= p: in a query round (the device's range check), in the final polynomial and in a cap (the host's)
    for pos in (q0 + 5, L["off_final_poly"], L["off_trace_cap"] + 1):
        bad = proof.copy()
        bad[pos] = S.P + 3
        items.append((AIR, cfg, bad))
    # a failed proof of work AND a word >= p in the query rounds: BAD_SHAPE wins over VERIFY
    bad = proof.copy()
    bad[L["off_pow_witness"]] = (int(bad[L["off_pow_witness"]]) + 1) % S.P
    items.append((AIR, cfg, bad.copy()))
    bad[q0 + 7] = S.P
    items.append((AIR, cfg, bad))
    # truncated, too short for a header, a mismatched config, a mismatched and an unknown AIR
    items.append((AIR, cfg, proof[:-1]))
    items.append((AIR, cfg, proof[:10]))
    other = S.StarkConfig.standard_fast_config()
    other.rate_bits = 1
    items.append((AIR, other, proof))
    items.append((S.AIR_FP12_MUL, S.StarkConfig.for_air(S.AIR_FP12_MUL), proof))
    items.append((9999, cfg, proof))
    # an accepted proof between the rejected ones
    items.append((AIR, cfg, proof))

    want = [_cpu_code(a, c, p) for a, c, p in items]
    got = S.verify_batch_replay(items)
    assert got == want
    assert want[-1] == 0 and want.count(0) == len(SHAPES) + 1
    for code in (S.ERR_VERIFY, S.ERR_BAD_SHAPE, S.ERR_BAD_AIR):
        assert code in want


def test_replay_of_an_empty_batch():
    assert S.verify_batch_replay([]) == []


def test_rust_binding_and_header_declare_the_device_verifier():
    hdr = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "starkhip-sys", "src", "lib.rs")).read()
    for name in ("starkhip_verify_batch", "starkhip_last_verify_timings", "starkhip_verify_batch_replay"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
    assert "verifier (GPU)" in hdr
    assert "pub fn verify_batch" in rs
