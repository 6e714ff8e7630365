"""The pool option "check_traces": a proving ticket submitted while it is on has its trace checked against the AIR by its context,
whichever submit it came through; wait returns ERR_TRACE with the check blob ("check_trace_list" entries at most) for a violating
trace and the lone prover's bytes for a satisfying one, with and without "verify_proofs"; the counters add up; a two-slot handle
passes the option to both of its pools.  1 big and 2 small contexts, no warm-up."""
import numpy as np
import pytest

import starky_bls12_381_amd as S

pytestmark = pytest.mark.gpu
TOY = S.AIR_TEST_FIBONACCI
CAP = 4


def _writes(trace):
    r, c = np.nonzero(trace)
    return np.stack([r.astype(np.uint64), c.astype(np.uint64), trace[r, c]], axis=1)


def _violating():
    """(64 rows with the product column changed on every row; 16 rows, all cells below 2^32, with one cell changed), public inputs"""
    t64, pis64 = S.trace_fibonacci(0, 1, 64)
    bad64 = t64.copy()
    bad64[:, 2] = (bad64[:, 2] + np.uint64(1)) % np.uint64(S.P)
    t16, pis16 = S.trace_fibonacci(0, 1, 16)
    bad16 = t16.copy()
    bad16[9, 0] += np.uint64(1)
    assert int(bad16.max()) < 1 << 32
    return (bad64, pis64), (bad16, pis16)


def _wait_refused(pool, ticket, want_blob):
    with pytest.raises(S.TraceViolation) as e:
        pool.wait(ticket)
    assert e.value.code == S.ERR_TRACE
    assert np.array_equal(e.value.blob, want_blob)
    assert len(e.value.report.list) <= CAP
    return e.value


@pytest.mark.parametrize("verify", [False, True])
def test_pool_checks_every_form_of_job(prover, verify):
    cfg = S.StarkConfig.standard_fast_config()
    (bad64, pis64), (bad16, pis16) = _violating()
    blob64, blob16 = S.check_blob_replay(TOY, bad64, pis64, cap=CAP), S.check_blob_replay(TOY, bad16, pis16, cap=CAP)
    assert int(blob64[3]) > CAP and int(blob64[6]) == CAP and 0 < int(blob16[6]) <= CAP
    good, good_pis = S.trace_fibonacci(3, 5)
    want = prover.prove(TOY, S.StarkConfig.for_air(TOY), good, good_pis)
    pool = S.ProofPool(0, big_contexts=1, small_contexts=2, verify_proofs=verify)
    try:
        pool.set_option("check_traces", 1)
        pool.set_option("check_trace_list", CAP)
        for name, value in (("check_traces", 2), ("check_traces", -1), ("check_trace_list", S.CHECK_LIST_MAX + 1), ("check_trace_list", -1)):
            with pytest.raises(S.StarkhipError) as e:
                pool.set_option(name, value)
            assert e.value.code == S.ERR_BAD_SHAPE
        t_good = pool.submit_witness(TOY, 3, 5)
        t_dense = pool.submit(TOY, cfg, bad64, pis64)
        t_cols = pool.submit(TOY, cfg, bad64.T.copy(), pis64, layout=1)
        t_rec = pool.submit(TOY, cfg, S.trace_from_writes(16, 4, _writes(bad16)), pis16)
        t_table = pool.submit_columns(TOY, cfg, [bad64[:, c].copy() for c in range(4)], pis64)
        proof, _ = pool.wait(t_good)
        assert np.array_equal(proof, want)
        err = _wait_refused(pool, t_dense, blob64)
        assert err.report.violations == prover.check_trace(TOY, bad64, pis64)[0]
        assert tuple(int(x) for x in err.report.list[0]) == prover.check_trace(TOY, bad64, pis64)[1]
        _wait_refused(pool, t_cols, blob64)
        _wait_refused(pool, t_rec, blob16)
        _wait_refused(pool, t_table, blob64)
        assert pool.check_stats() == {"checked": 5, "rejected": 4}
        st = pool.verify_stats()
        assert st["proofs_checked"] == (1 if verify else 0) and st["rejected"] == 0  # a refused trace never reaches the verifier
        # the pool still proves
        proof, _ = pool.wait(pool.submit_witness(TOY, 3, 5))
        assert np.array_equal(proof, want)
        assert pool.check_stats() == {"checked": 6, "rejected": 4}
        # option off: read at submit; a violating trace is proven like any other and nothing is counted
        pool.set_option("check_traces", 0)
        ticket = pool.submit(TOY, cfg, bad64, pis64)
        try:
            bad_proof, _ = pool.wait(ticket)
            assert not verify
            with pytest.raises(S.StarkhipError) as e:
                S.verify_stark_proof(TOY, cfg, bad_proof)
            assert e.value.code == S.ERR_VERIFY
        except S.StarkhipError as e:
            assert verify and e.code == S.ERR_VERIFY and not isinstance(e, S.TraceViolation)
        assert pool.check_stats() == {"checked": 6, "rejected": 4}
    finally:
        pool.close()


def test_two_slot_handle_passes_the_option_to_both_pools():
    cfg = S.StarkConfig.standard_fast_config()
    (bad64, pis64), _ = _violating()
    blob = S.check_blob_replay(TOY, bad64, pis64, cap=CAP)
    pool = S.ProofPool(big_contexts=1, small_contexts=2, devices=[0, 0])
    try:
        pool.set_option("check_traces", 1)
        pool.set_option("check_trace_list", CAP)
        tickets = [pool.submit(TOY, cfg, bad64, pis64, slot=s) for s in (0, 1)]
        good = [pool.submit_witness(TOY, 3, 5, slot=s) for s in (0, 1)]
        assert [pool.slot_of(t) for t in tickets] == [0, 1]
        for t in tickets:
            _wait_refused(pool, t, blob)
        proofs = [pool.wait(t)[0] for t in good]
        assert np.array_equal(proofs[0], proofs[1])
        assert pool.check_stats(per_pool=True) == [{"checked": 2, "rejected": 1}] * 2
        assert pool.check_stats() == {"checked": 4, "rejected": 2}
    finally:
        pool.close()
