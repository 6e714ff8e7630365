"""LogUp lookups over Column combinations with per-column Filters on the GPU (COMPAT.md §2c): the general kernels of
csrc/kernels_logup.hip and csrc/kernels_logup_freq.hip against the Python reference of tests/logup_columns_ref.py, word for word, and
whole proofs through the product's CPU verifier, its device verifier and the Python mini-verifier.  The shapes are the smallest at
which the kernels can go wrong: 2 rows (the next row is the other row), 64 and 128 (a next-row read crosses a wave), 2048 (two spans
of the prefix sum), 2^14; degrees 2, 3 and 5 with m = 1 and m no multiple of degree - 1.  Every shape is at most 2^14 rows x 20 columns."""
import os
import subprocess
import sys

import numpy as np
import pytest

import logup_columns_ref as G
import logup_ref as R
import starky_bls12_381_amd as S
from logup_columns_util import columns_air, golden_case, load_golden, plain_in_general_section
from logup_util import cpu_code, logup_air, logup_config, logup_flips

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = G.P
_REF = {}


def _case(name, n_rows):
    """(air, blob, lookups, trace with some cells >= p, public inputs, the reference's polys, closing values), computed once"""
    if (name, n_rows) not in _REF:
        air, blob, case, lookups = columns_air(name)
        trace, pis = G.make_trace(case, n_rows, seed=5 * n_rows + len(name), noncanonical=True)
        assert (trace >= np.uint64(P)).any()
        polys, closing, zeros = G.polys_and_closing(lookups, case.degree, trace.tolist(), G.CHALLENGES)
        assert zeros == 0 and all(c == 0 for row in closing for c in row)  # the reference alone says the trace closes
        trace.setflags(write=False)
        _REF[(name, n_rows)] = (air, blob, lookups, trace, pis, np.array(polys, dtype=np.uint64), np.array(closing, dtype=np.uint64))
    return _REF[(name, n_rows)]


SHAPES = [("mixed", n) for n in (2, 64, 128, 2048, 1 << 14)] + [(name, n) for name in ("next_only", "wide16", "big_filter", "table_comb", "freq_comb") for n in (2, 128)]


@pytest.mark.parametrize("name,n_rows", SHAPES)
def test_polys_are_the_references(prover, name, n_rows):
    air, blob, lookups, trace, pis, ref_polys, ref_closing = _case(name, n_rows)
    assert S.air_logup_general(air) == 1 and ref_polys.shape[0] == S.air_logup_polys(air)
    for layout, t in ((0, trace), (1, np.ascontiguousarray(trace.T))):
        polys, closing, zeros = prover.logup_polys(air, t, G.CHALLENGES, layout=layout)
        assert np.array_equal(polys, ref_polys) and np.array_equal(closing, ref_closing) and zeros == 0, (layout,)
    reduced = trace % np.uint64(P)  # cells >= p give the words of the reduced trace
    assert np.array_equal(prover.logup_polys(air, reduced, G.CHALLENGES)[0], ref_polys)


def test_a_filter_of_ones_gives_the_unfiltered_polys(prover):
    air, blob, lookups, trace, pis, ref_polys, ref_closing = _case("ones", 128)
    bare = columns_air("ones_unfiltered")[0]
    assert bare != air
    for a in (air, bare):
        polys, closing, zeros = prover.logup_polys(a, trace, G.CHALLENGES)
        assert np.array_equal(polys, ref_polys) and np.array_equal(closing, ref_closing) and zeros == 0


def test_zero_denominators_count_filtered_off_cells_too(prover):
    air, blob, lookups, trace, pis, _, _ = _case("mixed", 128)
    # chi_0 = p - the constant Column 9, whose filter is 0 on every row: n zero denominators that change no helper; chi_1 = p - a table cell
    ch = [P - 9, (P - int(trace[3, 3]) % P) % P]
    ref_polys, ref_closing, ref_zeros = G.polys_and_closing(lookups, 3, trace.tolist(), ch)
    assert ref_zeros >= 129
    polys, closing, zeros = prover.logup_polys(air, trace, ch)
    assert zeros == ref_zeros and polys.tolist() == ref_polys and closing.tolist() == ref_closing
    assert S.logup_polys_replay(air, trace, ch)[2] == ref_zeros


class _forced_general:
    """STARKHIP_LOGUP_GENERAL=1: the general kernels on a program of plain lookups (read whenever a descriptor is built)"""

    def __enter__(self):
        os.environ["STARKHIP_LOGUP_GENERAL"] = "1"

    def __exit__(self, *a):
        del os.environ["STARKHIP_LOGUP_GENERAL"]


@pytest.mark.parametrize("degree,m", [(2, 2), (3, 3), (5, 5)])
def test_the_general_kernels_on_a_plain_program_give_the_plain_kernels_words(prover, degree, m):
    air, blob = logup_air(degree, m, 2)
    blob2 = plain_in_general_section(degree, m, 2)
    assert int.from_bytes(b"LOGUPS02", "little") in [int(x) for x in blob2] and len(blob2) > len(blob)
    air2 = S.register_air(blob2)
    assert air2 != air and S.air_logup_general(air) == 0 and S.air_logup_general(air2) == 0
    cfg = logup_config(degree, 3)
    for n in (2, 2048):
        trace, _ = R.make_trace(degree, m, 2, n, seed=n + m, noncanonical=True)
        want = prover.logup_polys(air, trace, G.CHALLENGES)
        assert (want[1] == 0).all() and want[2] == 0
        with _forced_general():
            got = prover.logup_polys(air, trace, G.CHALLENGES)
        for g in (got, prover.logup_polys(air2, trace, G.CHALLENGES)):
            assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]) and g[2] == 0
    trace, pis = R.make_trace(degree, m, 2, 256, seed=11)
    proof = prover.prove(air, cfg, trace, pis)
    with _forced_general():
        forced = prover.prove(air, cfg, trace, pis)
        forced2 = prover.prove(air2, cfg, trace, pis)
    assert forced.tobytes() == proof.tobytes() == forced2.tobytes() == prover.prove(air2, cfg, trace, pis).tobytes()
    assert int(proof[15]) == 0
    S.verify_stark_proof(air2, cfg, proof)  # nothing in a proof names the section


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import logup_columns_ref as G
import starky_bls12_381_amd as S
from logup_columns_util import columns_air
from logup_util import logup_config
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.array(a, order="C", copy=True).view(np.int64)).to("cuda:0")
pv = S.Prover(0)
for name, n in (("mixed", 128), ("table_comb", 4096)):
    air, blob, case, lookups = columns_air(name)
    trace, pis = G.make_trace(case, n, seed=n, noncanonical=True)
    want = S.logup_polys_replay(air, trace, G.CHALLENGES)
    assert (want[1] == 0).all() and want[2] == 0
    zeroed = trace.copy()
    fcols = [lk["freq"][1][0][0] for lk in lookups]
    zeroed[:, fcols] = 0
    for layout, t, z in ((0, dev(trace), dev(zeroed)), (1, dev(trace.T), dev(zeroed.T))):
        torch.cuda.synchronize()
        polys, closing, zeros = pv.logup_polys_device(air, t.data_ptr(), n, G.CHALLENGES, layout=layout)
        assert np.array_equal(polys, want[0]) and np.array_equal(closing, want[1]) and zeros == 0, (name, layout)
        rep = pv.logup_frequencies_device(air, z.data_ptr(), n, trace.shape[1], layout=layout)
        torch.cuda.synchronize()
        back = z.cpu().numpy().view(np.uint64)
        back = back.T if layout else back
        assert rep.failed == 0 and np.array_equal(back %% np.uint64(G.P), trace %% np.uint64(G.P)), (name, layout)
    cfg = logup_config(case.degree, 3)
    ref = pv.prove(air, cfg, trace, pis)
    S.verify_stark_proof(air, cfg, ref)
    for layout, t in ((0, dev(trace)), (1, dev(trace.T))):
        torch.cuda.synchronize()
        assert np.array_equal(pv.prove_device(air, cfg, t.data_ptr(), n, pis, layout=layout), ref), (name, layout)
pv.close()
print("device forms ok")
"""


def test_traces_in_device_memory():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "device forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ whole proofs
def _prove(prover, name, n_rows, hasher, nq):
    air, blob, lookups, trace, pis, _, _ = _case(name, n_rows)
    cfg = logup_config(G.CASES[name].degree, nq)
    prover.set_option("hasher", hasher)
    try:
        return air, blob, cfg, trace, pis, prover.prove(air, cfg, trace, pis)
    finally:
        prover.set_option("hasher", S.HASHER_POSEIDON)


@pytest.mark.parametrize("hasher", [S.HASHER_POSEIDON, S.HASHER_KECCAK])
@pytest.mark.parametrize("name,n_rows", [("mixed", 32), ("mixed", 1 << 14), ("next_only", 64), ("wide16", 64), ("big_filter", 128), ("table_comb", 64), ("freq_comb", 32)])
def test_prove_and_verify(prover, name, n_rows, hasher):
    nq = 3 if n_rows <= 256 else 84  # the Python verifier hashes every opened leaf and path: few rounds keep it within seconds
    air, blob, cfg, trace, pis, proof = _prove(prover, name, n_rows, hasher, nq)
    assert S.proof_hasher(proof) == hasher and int(proof[13]) == 0 and int(proof[14]) == S.air_logup_polys(air) > 0 and int(proof[15]) == 0
    S.verify_stark_proof(air, cfg, proof)
    assert prover.verify_batch([(air, cfg, proof)]) == [0]
    if n_rows <= 256:
        G.verify_or_raise(blob, cfg, proof, hasher)
    assert np.array_equal(proof, _prove(prover, name, n_rows, hasher, nq)[5])  # two runs, the same bytes
    if n_rows <= 256:  # the interpreter behind the same LogUp kernel: the same bytes
        prover.set_option("quotient_impl", 1)
        try:
            other = _prove(prover, name, n_rows, hasher, nq)[5]
        finally:
            prover.set_option("quotient_impl", 0)
        assert np.array_equal(proof, other)


def test_every_upload_form_gives_the_same_proof(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, "mixed", 256, S.HASHER_POSEIDON, 3)
    cm = np.ascontiguousarray(trace.T)
    assert np.array_equal(prover.prove(air, cfg, cm, pis, layout=1), proof)
    assert np.array_equal(prover.prove_columns(air, cfg, [cm[c].copy() for c in range(cm.shape[0])], pis), proof)
    assert np.array_equal(prover.prove(air, cfg, trace % np.uint64(P), pis), proof)  # the trace has cells >= p
    prover.set_option("check_trace", 1)  # the check covers the AIR's own constraints only, and the proof is the same
    try:
        assert np.array_equal(prover.prove(air, cfg, trace, pis), proof)
    finally:
        prover.set_option("check_trace", 0)


def test_a_pools_and_a_multi_device_handles_proofs_are_the_contexts(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, "big_filter", 256, S.HASHER_POSEIDON, 3)
    pool = S.ProofPool(0, big_contexts=1, small_contexts=2, verify_proofs=True)  # the pool's own device verifier checks each before wait returns
    try:
        for t in [pool.submit(air, cfg, trace, pis) for _ in range(3)]:
            assert np.array_equal(pool.wait(t)[0], proof)
        bad = logup_flips(proof)["aux_leaf"]
        assert pool.wait(pool.submit_verify(air, bad, config=cfg)) == S.ERR_VERIFY
        assert pool.wait(pool.submit_verify(air, proof, config=cfg)) == 0
    finally:
        pool.close()
    pool = S.ProofPool(big_contexts=1, small_contexts=2, devices=[0, 0])  # two pools of one handle, both on this device
    try:
        for t in [pool.submit(air, cfg, trace, pis) for _ in range(4)]:
            assert np.array_equal(pool.wait(t)[0], proof)
    finally:
        pool.close()


def test_verify_batch_gives_the_cpu_verifiers_codes(prover):
    items = []
    for name, n_rows, hasher in (("mixed", 32, 0), ("mixed", 32, 1), ("table_comb", 64, 1)):
        air, blob, cfg, trace, pis, proof = _prove(prover, name, n_rows, hasher, 3)
        items.append((air, cfg, proof))
        items += [(air, cfg, bad) for bad in logup_flips(proof).values()]
        C = int(proof[1])
        t = proof.copy()  # the next-row opening of a trace column: mixed reads column 5 on the next row only
        off = int(S.proof_layout(proof).off_next_values) + 2 * 5
        t[off] = (int(t[off]) + 1) % P
        items.append((air, cfg, t))
        assert C > 5
    want = [cpu_code(*it) for it in items]
    assert want.count(0) == 3 and want.count(S.ERR_VERIFY) == 18
    assert prover.verify_batch(items) == want
    assert S.verify_batch_replay(items) == want


def _mixed_rows(trace):
    """(a row whose selector, column 7, is on, one where it is off)"""
    sel = trace[:, 7] % np.uint64(P)
    return int(np.nonzero(sel == 1)[0][3]), int(np.nonzero(sel == 0)[0][3])


def test_what_does_not_close_is_refused_and_the_context_goes_on(prover):
    air, blob, cfg, trace, pis, proof = _prove(prover, "mixed", 256, S.HASHER_POSEIDON, 3)
    on, off = _mixed_rows(trace)
    outside = 1 << 20  # the table's values are below 2^16
    wrong_freq, on_cell, off_cell = trace.copy(), trace.copy(), trace.copy()
    wrong_freq[100, 10] = (int(wrong_freq[100, 10]) + 1) % P  # a frequencies cell: no constraint of the AIR itself reads it
    on_cell[on, 6] = outside
    off_cell[off, 6] = outside
    for bad in (wrong_freq, on_cell):
        with pytest.raises(S.StarkhipError) as e:
            prover.prove(air, cfg, bad, pis)
        assert e.value.code == S.ERR_QUOTIENT_NOT_DIVISIBLE
        assert np.array_equal(prover.prove(air, cfg, trace, pis), proof)
    other = prover.prove(air, cfg, off_cell, pis)  # a filtered-off cell is looked up nowhere
    assert not np.array_equal(other, proof)
    S.verify_stark_proof(air, cfg, other)
    G.verify_or_raise(blob, cfg, other, S.HASHER_POSEIDON)


# ------------------------------------------------------------------------------------------------ the frequencies fill
def _freq_cols(lookups):
    return [lk["freq"][1][0][0] for lk in lookups]


@pytest.mark.parametrize("name,n_rows", [("mixed", 2), ("mixed", 2048), ("next_only", 128), ("wide16", 128), ("big_filter", 128), ("table_comb", 2), ("table_comb", 128),
                                         ("ones", 64)])
def test_the_fill_is_the_references(prover, name, n_rows):
    air, blob, lookups, trace, pis, _, _ = _case(name, n_rows)
    assert S.air_logup_fillable(air) == 1
    want = G.frequencies(lookups, trace.tolist())
    for layout in (0, 1):
        t = trace.copy()
        t[:, _freq_cols(lookups)] = 77
        arg = np.ascontiguousarray(t.T) if layout else t
        rep = prover.logup_frequencies(air, arg, layout=layout)
        assert rep.failed == 0 and rep.missing_cells == 0
        got = arg.T if layout else arg
        for f, w in zip(_freq_cols(lookups), want):
            assert got[:, f].tolist() == w, (layout, f)
        replay = trace.copy()
        replay[:, _freq_cols(lookups)] = 77
        S.logup_frequencies_replay(air, replay)
        assert np.array_equal(got, replay)


def test_a_filter_that_is_neither_0_nor_1_is_flagged_on_its_row(prover):
    air, blob, lookups, trace, pis, _, _ = _case("mixed", 128)
    on, off = _mixed_rows(trace)
    bad = trace.copy()
    bad[:, 10] = 77
    bad[off, 7] = 2
    bad[on, 6] = 1 << 20  # and a filter-on cell outside the table
    t = bad.copy()
    rep = prover.logup_frequencies(air, t)
    assert (rep.failed, rep.missing_cells, rep.missing_rows) == (1, 2, 2) and rep.list.tolist() == sorted([[0, on], [0, off]])
    assert np.array_equal(t, bad)  # nothing is written for a lookup that fails
    r = bad.copy()
    rep2 = S.logup_frequencies_replay(air, r)
    assert rep2.list.tolist() == rep.list.tolist() and rep2.per_column.tolist() == rep.per_column.tolist() == [0, 2, 0] and np.array_equal(r, bad)


def test_fill_inside_prove_and_the_blob_of_a_bad_trace(prover):
    filler = S.Prover(0)
    filler.set_option("fill_frequencies", 1)
    try:
        for name, n in (("mixed", 64), ("table_comb", 2048)):
            air, blob, cfg, trace, pis, want = _prove(prover, name, n, S.HASHER_POSEIDON, 3)
            lookups = _case(name, n)[2]
            zeroed = trace.copy()
            zeroed[:, _freq_cols(lookups)] = 0
            before = zeroed.copy()
            for form, proof in (("rows", filler.prove(air, cfg, zeroed, pis)), ("columns", filler.prove(air, cfg, np.ascontiguousarray(zeroed.T), pis, layout=1)),
                                ("column table", filler.prove_columns(air, cfg, [zeroed[:, c].copy() for c in range(zeroed.shape[1])], pis))):
                assert proof.tobytes() == want.tobytes(), (name, form)
            assert np.array_equal(zeroed, before)
        air, blob, cfg, trace, pis, want = _prove(prover, "mixed", 64, S.HASHER_POSEIDON, 3)
        on, off = _mixed_rows(trace)
        bad = trace.copy()
        bad[on, 6] = 1 << 20
        bad[off, 7] = 2
        with pytest.raises(S.TraceViolation) as e:
            filler.prove(air, cfg, bad, pis)
        assert e.value.code == S.ERR_TRACE and e.value.blob.tobytes() == S.logup_blob_replay(air, bad).tobytes()
        assert e.value.logup_report.list.tolist() == sorted([[0, on], [0, off]])
        assert filler.prove(air, cfg, trace, pis).tobytes() == want.tobytes()  # the context is as usable as before
        pool = S.ProofPool(0, big_contexts=1, small_contexts=1, verify_proofs=True)
        try:
            pool.set_option("fill_frequencies", 1)
            zeroed = trace.copy()
            zeroed[:, 10] = 0
            tickets = [pool.submit(air, cfg, zeroed, pis), pool.submit(air, cfg, bad, pis)]
            assert pool.wait(tickets[0])[0].tobytes() == want.tobytes()
            with pytest.raises(S.TraceViolation) as e:
                pool.wait(tickets[1])
            assert e.value.blob.tobytes() == S.logup_blob_replay(air, bad).tobytes()
        finally:
            pool.close()
        # frequencies that are a combination: nothing can fill them
        air, blob, cfg, trace, pis, want = _prove(prover, "freq_comb", 32, S.HASHER_POSEIDON, 3)
        assert S.air_logup_fillable(air) == 0
        with pytest.raises(S.StarkhipError) as e:
            filler.prove(air, cfg, trace, pis)
        assert e.value.code == S.ERR_BAD_AIR
        with pytest.raises(S.StarkhipError) as e:
            filler.logup_frequencies(air, trace.copy())
        assert e.value.code == S.ERR_BAD_SHAPE
    finally:
        filler.close()


def test_golden_proofs_are_regenerated():
    air, blob, cfg, trace, pis = golden_case()
    committed = load_golden()
    p = S.Prover(0)
    try:
        for hasher in (S.HASHER_POSEIDON, S.HASHER_KECCAK):
            p.set_option("hasher", hasher)
            assert np.array_equal(p.prove(air, cfg, trace, pis), committed[hasher]), hasher
    finally:
        p.close()
