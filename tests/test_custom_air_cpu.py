"""User-defined AIRs on the CPU: the program validator (starkhip_air_check_program), the registry (starkhip_air_register), the
Python builder, and oracle proofs of seeded random AIRs checked by the product's verifiers under a registered id."""
import threading

import numpy as np
import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from air_blob import parse_blob
from random_air import random_air
from starky_bls12_381_amd.air_builder import AirBuilder, REF_NEXT, REF_COMPL

BUILTIN = [S.AIR_FP12_MUL, S.AIR_PAIRING_PRECOMP, S.AIR_MILLER_LOOP, S.AIR_FINAL_EXP, S.AIR_ECC_AGGREGATE, S.AIR_TEST_FIBONACCI]


def fib_program():
    """The Fibonacci toy AIR of csrc/air_fibonacci.cpp, written with the Python builder."""
    b = AirBuilder(4, 3, 3)
    one = AirBuilder.one()
    b.first_row(b.L(0) - b.PI(0))
    b.first_row(b.L(1) - b.PI(1))
    b.last_row(b.L(1) - b.PI(2))
    b.transition(b.N(0) - b.L(1))
    b.transition(b.N(1) - b.L(0) - b.L(1))
    b.constraint(b.L(2) - b.L(0) * b.L(1))
    b.constraint(b.L(3) * (one - b.L(3)))
    b.constraint(b.L(3) * (b.L(2) - b.L(0) * b.L(1)) * AirBuilder.C(5))
    b.transition((one - b.L(3)) * (b.N(3) - 1))
    b.transition(b.L(3) * b.N(3))
    b.transition((one - b.L(3)) * (b.L(2) * AirBuilder.C(1 << 32) - b.L(0) * b.L(1) * AirBuilder.C(1 << 32)))
    return b.finish()


def test_builder_reproduces_the_fibonacci_program():
    assert np.array_equal(fib_program(), S.air_program(S.AIR_TEST_FIBONACCI))


@pytest.mark.parametrize("air", BUILTIN)
def test_builtin_program_registers_with_the_same_shape(air):
    blob = S.air_program(air)
    assert S.air_check_program(blob) is None
    i = S.register_air(blob, name="copy", default_rows=S.air_default_rows(air))
    assert i >= S.AIR_CUSTOM_BASE
    assert (S.air_columns(i), S.air_public_inputs(i), S.air_constraint_degree(i), S.air_num_constraints(i), S.air_default_rows(i)) == \
        (S.air_columns(air), S.air_public_inputs(air), S.air_constraint_degree(air), S.air_num_constraints(air), S.air_default_rows(air))
    assert np.array_equal(S.air_program(i), blob)
    assert S.register_air(blob) == i
    assert S.StarkConfig.for_air(i).rate_bits == S.StarkConfig.for_air(air).rate_bits
    if air in (S.AIR_TEST_FIBONACCI, S.AIR_ECC_AGGREGATE):  # the tiled plan of the registered copy replays to the plain fold
        assert S.quotient_plan_check(i, 4, 7) == S.quotient_plan_check(air, 4, 7)


def test_unregistered_ids_are_bad_air():
    for air in (S.AIR_CUSTOM_BASE + S.AIR_CUSTOM_CAPACITY - 1, S.AIR_CUSTOM_BASE + S.AIR_CUSTOM_CAPACITY, 5, 99, -1):
        with pytest.raises(S.StarkhipError) as e:
            S.air_columns(air)
        assert e.value.code == S.ERR_BAD_AIR
        with pytest.raises(S.StarkhipError):
            S.StarkConfig.for_air(air)


def test_register_argument_checks():
    blob = fib_program()
    with pytest.raises(S.StarkhipError) as e:
        S.register_air(blob, default_rows=3)
    assert e.value.code == S.ERR_BAD_SHAPE
    with pytest.raises(S.StarkhipError) as e:
        S.register_air(blob[:-1])
    assert e.value.code == S.ERR_BAD_AIR


def test_custom_config_rate_bits_cover_the_degree():
    for degree, rate in ((2, 1), (3, 1), (4, 2), (5, 2), (6, 3), (8, 3)):
        b = AirBuilder(2, 0, degree)
        b.constraint(b.L(0) - b.L(1))
        cfg = S.StarkConfig.for_air(S.register_air(b.finish()))
        assert cfg.rate_bits == rate, degree
        std = S.StarkConfig.standard_fast_config()
        assert [getattr(cfg, f) for f, _ in cfg._fields_ if f != "rate_bits"] == [getattr(std, f) for f, _ in std._fields_ if f != "rate_bits"]


def test_custom_placement_costs_are_estimates_between_the_builtins():
    blob, _, _ = random_air(11, 40, 4, 64)
    i = S.register_air(blob)
    cost, vcost = S.lib.starkhip_air_cost(i), S.lib.starkhip_air_verify_cost(i)
    assert 1.0 < cost < S.lib.starkhip_air_cost(S.AIR_FINAL_EXP) and 0.0 < vcost < S.lib.starkhip_air_verify_cost(S.AIR_MILLER_LOOP)
    fe = S.register_air(S.air_program(S.AIR_FINAL_EXP), default_rows=8192)  # the formula lands near the measured figures
    assert abs(S.lib.starkhip_air_cost(fe) - S.lib.starkhip_air_cost(S.AIR_FINAL_EXP)) < 3
    assert abs(S.lib.starkhip_air_verify_cost(fe) - S.lib.starkhip_air_verify_cost(S.AIR_FINAL_EXP)) < 3


# ---------------------------------------------------------------------------------------------------------- malformed programs
def _code_of(blob):
    p = parse_blob(blob)
    return p, 8 + len(p["consts"])


def _set_code(blob, i, w):
    """blob with code word i replaced by w"""
    b = blob.copy()
    _, base = _code_of(b)
    q, half = base + i // 2, i & 1
    b[q] = np.uint64((int(b[q]) & ~(0xFFFFFFFF << (32 * half))) | (w << (32 * half)))
    return b


def _find(code, pred):
    return next(i for i, w in enumerate(code) if pred(i, w))


def _malformed():
    blob = fib_program()
    p, base = _code_of(blob)
    code = p["code"]
    n_consts = len(p["consts"])
    out = {}
    # positions in the Fibonacci program: the first group word, a term word with a factor, a gate word
    g0 = 0
    t0 = 1 + ((code[0] >> 8) & 255)          # first term of group 0: L(0) (- PI 0)
    cell0 = t0 + 1                           # its cell factor
    group_offs = [int(x) & 0xFFFFFFFF for x in blob[-p["n_groups"]:]]
    gate_group = next(i for i in group_offs if (code[i] >> 8) & 255 >= 1)
    out["column out of range"] = _set_code(blob, cell0, 4)
    out["column out of range, next row"] = _set_code(blob, cell0, 1000 | REF_NEXT)
    out["unknown cellref flag"] = _set_code(blob, cell0, 1 | (1 << 29))
    out["REF_COMPL on a term factor"] = _set_code(blob, cell0, 0 | REF_COMPL)
    pi_term = _find(code, lambda i, w: i > 0 and w != 0 and (w >> 2) & 7 in (3, 4) and w & 32)
    out["PI index out of range"] = _set_code(blob, pi_term, (code[pi_term] & 63) | (3 << 6))
    const_term = _find(code, lambda i, w: i > 0 and (w >> 2) & 7 == 2 and (w & 3) >= 1)
    out["const index out of range"] = _set_code(blob, const_term, (code[const_term] & 63) | (n_consts << 6))
    out["coefficient kind 5"] = _set_code(blob, t0, (code[t0] & ~(7 << 2)) | (5 << 2))
    b = blob.copy()
    b[8] = np.uint64(S.P)
    out["non-canonical const"] = b
    out["m = 0"] = _set_code(blob, g0, code[g0] & 0xFFFF)
    out["five gates"] = _set_code(blob, gate_group, (code[gate_group] & ~(255 << 8)) | (5 << 8))
    b = blob.copy()
    b[3] = 2
    out["understated degree"] = b
    b = blob.copy()
    b[3] = 9
    out["degree above the limit"] = b
    out["missing END"] = _set_code(blob, len(code) - 1, code[0])
    b = np.concatenate([blob[:base + (len(code) + 1) // 2], [np.uint64(0)], blob[base + (len(code) + 1) // 2:]])
    b[6] = len(code) + 2
    out["trailing words"] = b
    b = blob.copy()
    b[-1] = np.uint64(int(b[-1]) + 1)
    out["wrong group table offset"] = b
    b = blob.copy()
    b[-1] = np.uint64(int(b[-1]) + (1 << 32))
    out["wrong group table k0"] = b
    b = blob.copy()
    b[4] = int(b[4]) + 1
    out["wrong constraint count"] = b
    b = blob.copy()
    b[0] = np.uint64(0x1234)
    out["bad magic"] = b
    out["truncated"] = blob[:-1]
    out["header only"] = blob[:8]
    b = blob.copy()
    b[1] = 0
    out["no columns"] = b
    b = blob.copy()
    b[2] = 1 << 20
    out["too many public inputs"] = b
    b = blob.copy()
    b[1] = 1 << 24
    out["too many columns"] = b
    b = blob.copy()
    b[6] = 1 << 40
    out["code size overflow"] = b
    return out


@pytest.mark.parametrize("case", sorted(_malformed()))
def test_malformed_program_is_refused_with_a_reason(case):
    blob = _malformed()[case]
    why = S.air_check_program(blob)
    assert why, case
    with pytest.raises(S.StarkhipError) as e:
        S.register_air(blob)
    assert e.value.code == S.ERR_BAD_AIR


def _refs_in_bounds(blob):
    p = parse_blob(blob)
    code, C, npi, nk = p["code"], p["n_cols"], p["n_pis"], len(p["consts"])
    i = 0
    while code[i] != 0:
        ng, m = (code[i] >> 8) & 255, code[i] >> 16
        assert 1 <= m <= 255 and ng <= 4
        for g in code[i + 1:i + 1 + ng]:
            assert g & 0xFFFFFF < C and g & ~(0xFFFFFF | REF_NEXT | REF_COMPL) == 0
        i += 1 + ng
        for _ in range(m):
            while True:
                tw = code[i]
                nf, ck, idx = tw & 3, (tw >> 2) & 7, tw >> 6
                assert ck <= 4 and (ck != 2 or idx < nk) and (ck not in (3, 4) or idx < npi)
                for f in code[i + 1:i + 1 + nf]:
                    assert f & 0xFFFFFF < C and f & ~(0xFFFFFF | REF_NEXT) == 0
                i += 1 + nf
                if tw & 32:
                    break
    assert i == len(code) - 1
    assert all(c < S.P for c in p["consts"])


def test_fuzzed_programs_are_refused_or_safe():
    """Single-word mutations of valid programs: each is refused, or accepted with every reference in bounds -- and then registered,
    its tiled plan built and replayed against the plain fold (a sample of them, the registry is finite)."""
    rng = np.random.default_rng(0xF022)
    bases = [fib_program()] + [random_air(s, c, d, 8)[0] for s, c, d in ((21, 9, 3), (22, 70, 5), (23, 20, 4))]
    accepted = refused = planned = 0
    for it in range(3000):
        base = bases[it % len(bases)]
        b = base.copy()
        pos = int(rng.integers(0, b.size))
        r = rng.random()
        if r < 0.3:
            b[pos] = np.uint64(int(b[pos]) ^ (1 << int(rng.integers(0, 64))))
        elif r < 0.6:
            b[pos] = np.uint64(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)))
        elif r < 0.8:
            b[pos] = np.uint64(int(b[pos]) + int(rng.integers(-3, 4)) & 0xFFFFFFFFFFFFFFFF)
        else:
            half = int(rng.integers(0, 2))
            b[pos] = np.uint64((int(b[pos]) & ~(0xFFFFFFFF << (32 * half))) | (int(rng.integers(0, 1 << 32)) << (32 * half)))
        why = S.air_check_program(b)
        if why:
            refused += 1
            continue
        accepted += 1
        _refs_in_bounds(b)
        if planned < 150 and not np.array_equal(b, base):
            i = S.register_air(b)
            assert S.quotient_plan_check(i, 1 + planned % 4, 3 + planned)["chunks"] >= 1
            planned += 1
    assert refused > 1000 and accepted > 100


# ---------------------------------------------------------------------------------------------------------- random AIRs, proven
CPU_CASES = [(31, 1, 2, 8), (32, 9, 3, 16), (33, 66, 5, 16), (34, 130, 4, 32)]


@pytest.mark.parametrize("seed,cols,degree,rows", CPU_CASES)
def test_random_air_oracle_proof_verifies_after_registration(seed, cols, degree, rows):
    blob, trace, pis = random_air(seed, cols, degree, rows)
    assert S.air_check_program(blob) is None
    assert O.check_trace(blob, trace, pis)[0] == 0
    cfg = S.StarkConfig.standard_fast_config()
    while (1 << cfg.rate_bits) + 1 < degree:
        cfg.rate_bits += 1
    proof = O.prove(blob, cfg, trace.T.copy(), pis)
    # ids are handed out in order: the next one is the first without an AIR, and it is BAD_AIR until the registration
    nxt = next(i for i in range(S.AIR_CUSTOM_BASE, S.AIR_CUSTOM_BASE + S.AIR_CUSTOM_CAPACITY) if S.lib.starkhip_air_columns(i) < 0)
    with pytest.raises(S.StarkhipError) as e:
        S.verify_stark_proof(nxt, cfg, proof)
    assert e.value.code == S.ERR_BAD_AIR
    assert S.verify_batch_replay([(nxt, cfg, proof)]) == [S.ERR_BAD_AIR]
    air = S.register_air(blob, name=f"random{seed}")
    assert air == nxt
    assert S.StarkConfig.for_air(air).rate_bits == cfg.rate_bits
    S.verify_stark_proof(air, cfg, proof)
    assert S.verify_batch_replay([(air, cfg, proof)]) == [0]
    L = S.proof_layout(proof)
    assert L.n_columns == cols and L.n_public_inputs == len(pis)
    for pos in (int(L.off_trace_cap) + 1, int(L.off_local_values) + 2 * (cols - 1), int(L.off_public_inputs)):
        bad = proof.copy()
        bad[pos] = np.uint64((int(bad[pos]) + 1) % S.P)
        with pytest.raises(S.StarkhipError):
            S.verify_stark_proof(air, cfg, bad)
        assert S.verify_batch_replay([(air, cfg, bad)]) != [0]


def test_registration_is_consistent_under_threads():
    blobs = [random_air(100 + s, 3 + s % 5, 2 + s % 4, 8)[0] for s in range(24)]
    known = {S.register_air(blobs[0]): blobs[0]}
    errors = []
    ids = {}

    def register(k):
        try:
            for j in range(k, len(blobs), 4):
                ids[j] = S.register_air(blobs[j])
                assert S.register_air(blobs[j]) == ids[j]
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)

    def query():
        try:
            for _ in range(300):
                for i, b in list(known.items()):
                    assert np.array_equal(S.air_program(i), b)
                for i in range(S.AIR_CUSTOM_BASE, S.AIR_CUSTOM_BASE + 400):
                    c = S.lib.starkhip_air_columns(i)
                    if c >= 0:
                        assert S.air_num_constraints(i) >= 1 and parse_blob(S.air_program(i))["n_cols"] == c
        except Exception as e:  # pragma: no cover
            errors.append(e)

    ts = [threading.Thread(target=register, args=(k,)) for k in range(4)] + [threading.Thread(target=query) for _ in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert len(set(ids.values())) == len(blobs)
    for j, b in enumerate(blobs):
        assert np.array_equal(S.air_program(ids[j]), b)
