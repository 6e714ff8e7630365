"""A pool of eight big contexts keeps to its stream budget (csrc/scheduler.h): the commitments of a lane-form group go out as ONE grid
on a long-launch stream, the proofs are the ones made alone, and the pool says how many hardware queues the process really has."""
import os

import numpy as np
import pytest

import starky_bls12_381_amd as S

pytestmark = pytest.mark.gpu


def test_eight_big_contexts_one_grid_per_group_same_proofs_and_the_queues_in_effect():
    from test_ecc_aggregate_cpu import pack, reference_vector
    env_queues = os.environ.get("GPU_MAX_HW_QUEUES")   # as the process was started: the library's own setenv does not show here
    air = S.AIR_ECC_AGGREGATE                          # 8192 rows at blow-up 4: the FinalExp class of commitments, a fraction of its columns
    cfg = S.StarkConfig.for_air(air)
    pts, bits, _ = reference_vector()
    trace, pis = S.trace_ecc_aggregate(*pack(pts, bits))
    pool = S.ProofPool(0, big_contexts=8, small_contexts=1, generator_threads=1)
    try:
        alone, info = pool.wait(pool.submit(air, cfg, trace, pis))
        assert (info["leaf_hash_form"], info["leaf_hash_group"]) == ("pair", 1)   # nobody to share a group with
        S.verify_stark_proof(air, cfg, alone)
        before = pool.stats()
        got = [pool.wait(t) for t in [pool.submit(air, cfg, trace, pis) for _ in range(8)]]
        after = pool.stats()
        host = pool.host_info()[0]
    finally:
        pool.close()
    for proof, _ in got:
        assert np.array_equal(proof, alone)
    # the groups as the tickets report them: a member of a group of g is 1 / g of a launch; a commitment that went out alone is one
    forms = [(i["leaf_hash_form"], i["leaf_hash_group"]) for _, i in got]
    assert all(f in (("lane", 2), ("lane", 3), ("lane", 4), ("pair", 1)) for f in forms), forms
    twelfths = sum(12 // g for _, g in forms)
    assert twelfths % 12 == 0, forms
    assert max(g for _, g in forms) >= 2, forms            # eight submitted together: groups did form
    assert after["big_commit_grids"] - before["big_commit_grids"] == twelfths // 12, forms   # launches = groups, not commitments
    assert after["big_commit_launches"] - before["big_commit_launches"] == 8
    assert before["big_commit_grids"] == 1
    # the queues in effect: the environment's value when there was one before HIP came up, else the library's 16 -- or HIP's 4 when
    # this process had used HIP before its first pool
    want = int(env_queues) if env_queues else (4 if S.api.hw_queues_late() else 16)
    assert S.api.hw_queues_in_effect() == want and host["hw_queues"] == want
    assert host["stream_budget"] == 10                     # eight big contexts, a small one, a merged window
