"""The device verifier inside a proof pool on the MI355X: "verify_proofs" checks every proof before wait returns it (the proofs
byte-identical to an unverified pool's), submit_verify gives exactly starkhip_verify's code for any proof -- on an idle pool and beside
a batch of signatures being proved --, the verifier allocates nothing per batch, and a two-slot handle spreads a verify batch over
both of its pools."""
import ctypes as C
import threading

import pytest

import oracle_lib as O
import starky_bls12_381_amd as S
from starky_bls12_381_amd.api import lib, PoolVerifyStats
from test_gpu_verify_device import _batch_with_tampered, _bump, _cpu_code, _sweep

pytestmark = pytest.mark.gpu


def _sigs(batch, seed):
    from bls_util import native_vectors
    from starky_bls12_381_amd import signature as G
    return G.synthetic_signatures(batch, native_vectors()["bls_signature"], seed=seed)


def _prove_signatures(pool, batch, sigs):
    from starky_bls12_381_amd import signature as G
    _, results, _, _, _ = G.one_step(None, batch, pool, G.plan_batch(batch, 1)[0], sigs)
    return [(air, cfg, proof) for _, (air, proof, cfg) in sorted(results.items())]


def _every_air(pool):
    """one proof of every AIR through submit_witness: one signature's six jobs, ECCAgg and the toy AIR"""
    from test_ecc_aggregate_cpu import pack, reference_vector
    out = _prove_signatures(pool, 1, _sigs(1, 0x7E57))
    pts, bits, _ = reference_vector()
    arr, b = pack(pts, bits)
    tickets = [(S.AIR_ECC_AGGREGATE, pool.submit_witness(S.AIR_ECC_AGGREGATE, arr, b)),
               (S.AIR_TEST_FIBONACCI, pool.submit_witness(S.AIR_TEST_FIBONACCI, 3, 5))]
    for air, t in tickets:
        proof, _ = pool.wait(t)
        out.append((air, S.StarkConfig.for_air(air), proof))
    return out


@pytest.fixture(scope="module")
def signature_batch():
    """48 proofs of eight signatures from a pool with "verify_proofs" on: [(air, cfg, proof)]"""
    pool = S.ProofPool(0, big_contexts=4, small_contexts=12, stream_priority=1, warm_up=1, verify_proofs=True)
    try:
        out = _prove_signatures(pool, 8, _sigs(8, 0x8516))
        st = pool.verify_stats()
    finally:
        pool.close()
    assert len(out) == 48
    assert st["proofs_checked"] == 48 and st["rejected"] == 0 and st["device_batches"] >= 1 and st["arena_bytes"] == 1024 << 20
    return out


def test_verify_proofs_pool_proves_every_air_byte_identically_and_counts_them():
    plain = S.ProofPool(0, big_contexts=2, small_contexts=6)
    try:
        want = _every_air(plain)
    finally:
        plain.close()
    checked = S.ProofPool(0, big_contexts=2, small_contexts=6, verify_proofs=True)
    try:
        got = _every_air(checked)  # every wait returned OK (ProofPool.wait raises otherwise)
        st = checked.verify_stats()
    finally:
        checked.close()
    assert {a for a, _, _ in got} == {S.AIR_TEST_FIBONACCI, S.AIR_FP12_MUL, S.AIR_ECC_AGGREGATE, S.AIR_FINAL_EXP, S.AIR_MILLER_LOOP,
                                      S.AIR_PAIRING_PRECOMP}
    assert len(got) == len(want) == 8
    for (a, _, p), (b, _, q) in zip(got, want):
        assert a == b and p.size == q.size and (p == q).all()
    assert st["proofs_checked"] == 8 and st["rejected"] == 0 and st["verify_jobs"] == 0


def _sweep_items(prover, signature_batch):
    from bls_util import random_fp12
    air = S.AIR_FP12_MUL
    t, pis = S.trace_fp12_mul(random_fp12(0x5EED3000), random_fp12(0x5EED3001))
    cfg = S.StarkConfig.for_air(air)
    fp12 = (air, cfg, prover.prove(air, cfg, t, pis))
    fexp = next(it for it in signature_batch if it[0] == S.AIR_FINAL_EXP)
    cfg_t = S.StarkConfig.standard_fast_config()
    t, pis = S.trace_fibonacci(3, 5, 256)
    toy = O.prove(S.air_program(S.AIR_TEST_FIBONACCI), cfg_t, S.trace_rows_to_poly_values(t), pis)  # an oracle proof
    items = []
    for it in (fp12, fexp):
        items += _sweep(*it) + [it]
        items.append((S.AIR_MILLER_LOOP, S.StarkConfig.for_air(S.AIR_MILLER_LOOP), it[2]))  # the wrong AIR
    items += [(S.AIR_TEST_FIBONACCI, cfg_t, toy), (S.AIR_TEST_FIBONACCI, cfg_t, _bump(toy, toy.size - 3))]
    return items


def test_submit_verify_tamper_sweep_on_an_idle_and_a_busy_pool(prover, signature_batch):
    items = _sweep_items(prover, signature_batch)
    want = [_cpu_code(*it) for it in items]
    assert want.count(0) == 3 and S.ERR_VERIFY in want and S.ERR_BAD_SHAPE in want
    pool = S.ProofPool(0, big_contexts=2, small_contexts=6)
    try:
        assert pool.verify_batch(items) == want  # idle
        proved = {}
        th = threading.Thread(target=lambda: proved.setdefault("out", _prove_signatures(pool, 2, _sigs(2, 0xB5))))
        th.start()
        try:
            tickets = [pool.submit_verify(a, p, c) for a, c, p in items]  # beside the proving signatures
            got = [pool.wait(t) for t in tickets]
        finally:
            th.join()
        assert got == want
        assert len(proved["out"]) == 12
        st = pool.verify_stats()
        assert st["verify_jobs"] == 2 * len(items) and st["rejected"] == 2 * (len(items) - 3)
    finally:
        pool.close()


def test_the_verifier_allocates_nothing_per_batch(signature_batch):
    pool = S.ProofPool(0, big_contexts=1, small_contexts=2, verify_arena_mb=512)
    try:
        assert pool.verify_batch(signature_batch[:12]) == [0] * 12
        r1, s1 = pool.reservation()["device_bytes"], pool.verify_stats()
        assert pool.verify_batch(signature_batch[12:30]) == [0] * 18
        r2, s2 = pool.reservation()["device_bytes"], pool.verify_stats()
        assert r1 == r2
        assert s1["arena_bytes"] == s2["arena_bytes"] == 512 << 20 and s2["device_batches"] > s1["device_batches"]
        with pytest.raises(S.StarkhipError):
            pool.set_option("verify_arena_mb", 256)  # the arena exists
    finally:
        pool.close()


def test_two_slot_handle_verify_batch_on_one_card(signature_batch):
    items = _batch_with_tampered(signature_batch)
    want = [_cpu_code(*it) for it in items]
    assert want.count(0) == 48 and want.count(S.ERR_VERIFY) == 6
    pool = S.ProofPool(big_contexts=1, small_contexts=2, devices=[0, 0])
    try:
        assert pool.verify_batch(items) == want
        per_slot = []
        for h in pool._pools():
            st = PoolVerifyStats()
            assert lib.starkhip_pool_verify_stats(h, C.byref(st)) == 0
            per_slot.append(int(st.verify_jobs))
        assert sum(per_slot) == len(items) and min(per_slot) > 0
    finally:
        pool.close()
