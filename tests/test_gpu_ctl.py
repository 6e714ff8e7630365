"""Cross-table lookups on the GPU (COMPAT.md §2d): the kernels of csrc/kernels_ctl.hip against the Python reference of tests/ctl_ref.py,
word for word, and whole system proofs through the product's CPU system verifier and the Python mini-verifier.  The row counts are the
smallest at which the kernels can go wrong: 2 rows (the next row is the other row), one span of the running sums' scan, two spans and
sixteen; the systems are proved with unequal row counts 2 and 2, 64 and 16, 2^14 and 32 (one table on the long transform)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ctl_ref as X
import starky_bls12_381_amd as S
from ctl_util import configs, cpu_code, ctl_system, golden_case, golden_two_case, load_golden
from logup_columns_util import golden_case as logup_golden_case, load_golden as logup_load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = X.P
SPAN = S.CTL_SPAN_ROWS
CASES = sorted(X.CASES)
_REF = {}


def _rows(name, big, small):
    return (big,) + (small,) * (len(X.CASES[name].tables) - 1)


def _polys_case(name, n):
    """(system, case, traces with some cells >= p, the reference's (polys, sums) per table), computed once and left unchanged"""
    if (name, n) not in _REF:
        system, _, _, case = ctl_system(name)
        traces = [t.copy() for t, _ in X.make_traces(case, _rows(name, n, min(n, 16)), seed=n + len(name))]
        want = []
        for t, trace in enumerate(traces):
            trace[::3, 3:] += np.uint64(P)  # every cell behind column 2 is small
            polys, sums, zeros = X.polys_and_sums(X.table_endpoints(case.ctls, t), trace.tolist(), X.CHALLENGES)
            assert zeros == 0
            want.append((np.array(polys, dtype=np.uint64), sums))
            trace.setflags(write=False)
        assert X.first_unbalanced(case.ctls, [s for _, s in want]) == -1  # the reference alone says the traces balance
        _REF[(name, n)] = (system, case, traces, want)
    return _REF[(name, n)]


@pytest.mark.parametrize("n", [2, SPAN, 2 * SPAN, 16 * SPAN])
@pytest.mark.parametrize("name", ["range", "xor", "next_row"])
def test_polys_byte_for_byte(prover, name, n):
    system, case, traces, want = _polys_case(name, n)
    for t, trace in enumerate(traces):
        for layout, arg in ((0, trace), (1, np.ascontiguousarray(trace.T))):
            polys, sums, zeros = S.ctl_polys(prover, system, t, arg, X.CHALLENGES, layout=layout)
            assert polys.tobytes() == want[t][0].tobytes() and sums.tolist() == want[t][1] and zeros == 0, (t, layout)


@pytest.mark.parametrize("n", [2, 2 * SPAN])
def test_zero_denominators_are_counted_exactly(prover, n):
    system, case, traces, _ = _polys_case("range", n)
    trace = traces[0]
    row = n - 1
    value = int(trace[row, 3]) % P
    chal = list(X.CHALLENGES)
    chal[3] = (P - value) % P  # gamma_1 = -value: every row holding it has a zero denominator under the second challenge pair
    hits = int(((trace[:, 3] % np.uint64(P)) == np.uint64(value)).sum())
    want = X.polys_and_sums(X.table_endpoints(case.ctls, 0), trace.tolist(), chal)
    polys, sums, zeros = S.ctl_polys(prover, system, 0, trace, chal)
    assert zeros == want[2] == hits >= 1 and int(polys[2, row]) == 0
    assert polys.tobytes() == np.array(want[0], dtype=np.uint64).tobytes() and sums.tolist() == want[1]


# ------------------------------------------------------------------------------------------------ whole systems
@pytest.fixture(scope="module")
def provers():
    made = {}

    def get(name):
        if name not in made:
            made[name] = S.SystemProver(ctl_system(name)[0], 0)
        return made[name]
    yield get
    for p in made.values():
        p.close()


def _prove(provers, name, rows, hasher, seed=1):
    system, airs, blobs, case = ctl_system(name)
    traces = X.make_traces(case, rows, seed=seed)
    cfgs = configs(case, rows=rows)
    sp = provers(name)
    sp.set_option("hasher", hasher)
    return system, blobs, case, cfgs, traces, sp, sp.prove(cfgs, [t for t, _ in traces], [p for _, p in traces])


@pytest.mark.parametrize("hasher", [S.HASHER_POSEIDON, S.HASHER_KECCAK])
@pytest.mark.parametrize("big,small", [(2, 2), (64, 16), (1 << 14, 32)])
@pytest.mark.parametrize("name", CASES)
def test_prove_and_verify(provers, name, big, small, hasher):
    system, blobs, case, cfgs, traces, sp, proof = _prove(provers, name, _rows(name, big, small), hasher)
    tables = S.system_proof_tables(proof)
    assert [int(t[15]) for t in tables] == [4 * len(X.table_endpoints(case.ctls, t)) for t in range(len(tables))]
    assert all(S.proof_hasher(t) == hasher for t in tables)
    S.verify_system_proof(system, cfgs, proof)
    X.verify_system_or_raise(blobs, case.ctls, cfgs, proof, hasher)
    again = sp.prove(cfgs, [t for t, _ in traces], [p for _, p in traces])
    assert again.tobytes() == proof.tobytes()


def test_balanced_shift_of_two_looking_sums_is_rejected(provers):
    system, blobs, case, cfgs, _, _, proof = _prove(provers, "two_lookers", (64, 16, 16), S.HASHER_POSEIDON)
    tables = [t.copy() for t in S.system_proof_tables(proof)]
    for t, delta in ((0, 9), (1, P - 9)):  # + delta on one looking sum and - delta on the other, under both challenges: the CTL balances
        at = int(S.proof_layout(tables[t]).off_ctl_sums)
        for i in range(2):
            tables[t][at + i] = (int(tables[t][at + i]) + delta) % P
    bad = S.system_proof_join(tables)
    sums_of = [[int(x) for x in t[int(S.proof_layout(t).off_ctl_sums):]] for t in tables]
    assert X.first_unbalanced(case.ctls, sums_of) == -1
    assert cpu_code(system, cfgs, bad) == S.ERR_VERIFY and not X.verify_system(blobs, case.ctls, cfgs, bad, S.HASHER_POSEIDON)


DEVICE_CHILD = r"""
import os, sys, faulthandler
faulthandler.dump_traceback_later(120, exit=True)
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np, torch   # torch first: its HIP runtime has to be the process's first
import ctl_ref as X
import starky_bls12_381_amd as S
from ctl_util import configs, ctl_system
torch.cuda.set_device(0)
dev = lambda a: torch.from_numpy(np.array(a, order="C", copy=True).view(np.int64)).to("cuda:0")
system, airs, blobs, case = ctl_system("xor")
cfgs = configs(case)
traces = X.make_traces(case, (64, 16), seed=2)
sp = S.SystemProver(system, 0)
ts, pis = [t for t, _ in traces], [p for _, p in traces]
ref = sp.prove(cfgs, ts, pis)
S.verify_system_proof(system, cfgs, ref)
cols = sp.prove(cfgs, [np.ascontiguousarray(t.T) for t in ts], pis, layouts=[1, 1])
mixed = sp.prove(cfgs, [ts[0], np.ascontiguousarray(ts[1].T)], pis, layouts=[0, 1])
assert cols.tobytes() == ref.tobytes() == mixed.tobytes()
for layout in (0, 1):
    d = [dev(t.T if layout else t) for t in ts]
    torch.cuda.synchronize()
    got = sp.prove(cfgs, [None, None], pis, layouts=[layout, layout], device_ptrs=[(d[0].data_ptr(), 64), (d[1].data_ptr(), 16)])
    assert got.tobytes() == ref.tobytes(), layout
    half = sp.prove(cfgs, [ts[0], None], pis, layouts=[0, layout], device_ptrs=[None, (d[1].data_ptr(), 16)])
    assert half.tobytes() == ref.tobytes(), layout
sp.close()
print("trace forms ok")
"""


def test_proof_bytes_do_not_depend_on_the_trace_form():
    # in a child process: a torch tensor needs torch's HIP runtime, which has to come up before the library's
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "trace forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_refusals_name_the_ctl_and_leave_the_handle_usable(provers):
    system, blobs, case, cfgs, traces, sp, good = _prove(provers, "chain", (64, 16, 16), S.HASHER_POSEIDON)
    ts, pis = [t.copy() for t, _ in traces], [p for _, p in traces]
    missing = [t.copy() for t in ts]
    row = int(np.nonzero(missing[0][:, 4] == 1)[0][0])
    missing[0][row, 3] = 99999  # a looking value of CTL 0 that table 1 does not hold
    wrong = [t.copy() for t in ts]
    wrong[2][5, 4] += np.uint64(1)  # a multiplicity of CTL 1's looked table one too high
    for bad, ctl in ((missing, 0), (wrong, 1)):
        with pytest.raises(S.SystemRefused) as e:
            sp.prove(cfgs, bad, pis)
        assert e.value.code == S.ERR_QUOTIENT_NOT_DIVISIBLE and e.value.ctl == ctl
        assert sp.prove(cfgs, ts, pis).tobytes() == good.tobytes()  # the same handle then proves the good system


def test_a_table_without_endpoints_and_plain_prove_keeps_its_bytes(prover):
    # a system whose third table carries no endpoint
    _, airs, blobs, case = ctl_system("range")
    from ctl_util import system_blob
    system = S.register_system(system_blob(airs + [airs[0]], case.ctls))
    assert [S.system_table_endpoints(system, t) for t in range(3)] == [1, 1, 0]
    traces = X.make_traces(case, (64, 16), seed=6)
    extra = X.make_traces(case, (8, 16), seed=7)[0]
    cfgs = configs(case) + [configs(case)[0]]
    sp = S.SystemProver(system, 0)
    try:
        proof = sp.prove(cfgs, [t for t, _ in traces] + [extra[0]], [p for _, p in traces] + [extra[1]])
    finally:
        sp.close()
    assert [int(t[15]) for t in S.system_proof_tables(proof)] == [4, 4, 0]
    S.verify_system_proof(system, cfgs, proof)
    X.verify_system_or_raise(blobs + [blobs[0]], case.ctls, cfgs, proof, S.HASHER_POSEIDON)
    # the two halves of prove() back to back are what prove() was: a LogUp AIR's proof is the committed golden's, byte for byte
    air, _, cfg, trace, pis = logup_golden_case()
    committed = logup_load_golden()
    for hasher in (S.HASHER_POSEIDON, S.HASHER_KECCAK):
        prover.set_option("hasher", hasher)
        try:
            assert prover.prove(air, cfg, trace, pis).tobytes() == committed[hasher].tobytes(), hasher
        finally:
            prover.set_option("hasher", S.HASHER_POSEIDON)


@pytest.mark.parametrize("which", ["range", "two_lookers"])
def test_golden_proofs_are_regenerated(which):
    system, _, _, cfgs, traces = golden_case() if which == "range" else golden_two_case()
    committed = load_golden("proofs_hex" if which == "range" else "two_lookers_proofs_hex")
    sp = S.SystemProver(system, 0)
    try:
        for hasher in (S.HASHER_POSEIDON, S.HASHER_KECCAK):
            sp.set_option("hasher", hasher)
            assert np.array_equal(sp.prove(cfgs, [t for t, _ in traces], [p for _, p in traces]), committed[hasher]), hasher
    finally:
        sp.close()
