"""LogUp lookups over Column combinations with per-column Filters (COMPAT.md §2c) without a GPU: the "LOGUPS02" section through both
builders, validator and registry; the host replays of the auxiliary polynomials and of the frequencies fill and the constraint fold
over an extension frame against the Python reference of tests/logup_columns_ref.py; the golden proofs
(tests/golden/logup_columns_small.json, one per hasher) through the CPU verifier, the device verifier's replay and the Python
mini-verifier, intact and with one word changed."""
import os
import subprocess

import numpy as np
import pytest

import keccak_ref as K
import logup_columns_ref as G
import logup_ref as R
import starky_bls12_381_amd as S
from logup_columns_util import GOLDEN, columns_air, golden_case, load_golden, plain_in_general_section
from logup_util import cpu_code, logup_air, logup_flips
from starky_bls12_381_amd.air_builder import AirBuilder, Column, Filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = G.P
MAGIC2 = int.from_bytes(b"LOGUPS02", "little")


def _section(blob):
    w = [int(x) for x in blob]
    return 8 + w[5] + (w[6] + 1) // 2 + w[7]


def _builder(n_cols=6, degree=3):
    b = AirBuilder(n_cols, 0, degree)
    b.constraint(b.L(1) - b.L(0) * b.L(0))
    return b


# ------------------------------------------------------------------------------------------------ blob, builders, registry
def test_the_section_word_for_word():
    b = _builder()
    b.logup_columns([(Column([(0, 3)], [(1, P - 1)], 5), Filter(products=[(Column.single(2), Column.const(1))], sums=[4])), (1, None)], Column([(2, 1), (3, 1 << 16)]), 5)
    blob = b.finish()
    at = _section(blob)
    assert [int(x) for x in blob[at:]] == [
        MAGIC2, 1, 2,
        2, 0, 2, 1, 3, 1 << 16,                 # the table: lo + 2^16 hi
        1, 0, 5, 1,                             # the frequencies: plain column 5
        1 | (1 << 32), 5, 0, 3, 1, P - 1,       # 5 + 3 local[0] - next[1]
        1 | (1 << 32), 1, 0, 2, 1, 0, 1, 1, 0, 4, 1,  # its filter: local[2] * 1 + local[4]
        1, 0, 1, 1, 0]                          # plain column 1 under the empty filter
    assert S.air_check_program(blob) is None
    air = S.register_air(blob)
    assert np.array_equal(S.air_program(air), blob) and S.register_air(blob.copy()) == air
    assert (S.air_logups(air), S.air_logup_columns(air), S.air_logup_polys(air), S.air_logup_general(air)) == (1, 2, 4, 1)
    assert S.air_logup_general(S.AIR_TEST_FIBONACCI) == 0
    with pytest.raises(S.StarkhipError) as e:
        S.air_logup_general(999)
    assert e.value.code == S.ERR_BAD_AIR


def test_a_plain_program_keeps_its_first_section_and_both_kinds_go_into_the_second():
    air, blob = logup_air(3, 3, 2)
    assert int(blob[_section(blob)]) == R.AIR_LOGUP_MAGIC and MAGIC2 not in [int(x) for x in blob]  # logup() alone: the old bytes
    assert S.air_logup_general(air) == 0
    blob2 = plain_in_general_section(3, 3, 2)
    assert int(blob2[_section(blob2)]) == MAGIC2 and np.array_equal(blob2[:_section(blob2)], blob[:_section(blob)])
    air2 = S.register_air(blob2)
    assert air2 != air and S.air_logup_general(air2) == 0 and S.air_logup_polys(air2) == S.air_logup_polys(air)
    assert np.array_equal(S.air_program(air2), blob2) and np.array_equal(S.air_program(air), blob)
    assert G.split_program(blob2)[1] == G.split_program(blob)[1]
    b = _builder()  # a plain declaration after a general one, and before: both in the general section, in declaration order
    b.logup([0], 2, 3)
    b.logup_columns([(Column([(1, 2)]), None)], 2, 4)
    b.logup([1], 2, 5)
    mixed = b.finish()
    assert [int(x) for x in mixed].count(MAGIC2) == 1 and R.AIR_LOGUP_MAGIC not in [int(x) for x in mixed]
    lookups = G.split_program(mixed)[1]
    assert [lk["freq"] for lk in lookups] == [G.plain(3), G.plain(4), G.plain(5)] and lookups[1]["pairs"][0][0] == (0, [(1, 2)], [])
    assert S.air_check_program(mixed) is None and S.air_logup_general(S.register_air(mixed)) == 1


def _cpp_column(col):
    const, local, nxt = col
    terms = lambda ts: "{" + ", ".join("{%du, %dull}" % t for t in ts) + "}"  # noqa: E731
    return "AirBuilder::column_of(%dull, %s, %s)" % (const, terms(local), terms(nxt))


def _cpp_case(case):
    """the C++ AirBuilder calls that declare the case's lookups, from the reference's reading of the Python builder's words"""
    _, lookups = G.split_program(case.blob())
    is_plain = lambda c: c[0] == 0 and len(c[1]) == 1 and not c[2] and c[1][0][1] == 1  # noqa: E731
    plain = lambda lk: all(is_plain(v) and f == ([], []) for v, f in lk["pairs"]) and is_plain(lk["table"]) and is_plain(lk["freq"])  # noqa: E731
    out = []
    for lk in lookups:
        if plain(lk):
            out.append("b.logup({%s}, %d, %d);" % (", ".join(str(v[1][0][0]) for v, _ in lk["pairs"]), lk["table"][1][0][0], lk["freq"][1][0][0]))
            continue
        pairs = []
        for v, (products, sums) in lk["pairs"]:
            flt = "AirBuilder::filter_of({%s}, {%s})" % (", ".join("{%s, %s}" % (_cpp_column(a), _cpp_column(c)) for a, c in products), ", ".join(_cpp_column(c) for c in sums))
            pairs.append("{%s, %s}" % (_cpp_column(v), flt))
        out.append("b.logup_columns({%s}, %s, %s);" % (", ".join(pairs), _cpp_column(lk["table"]), _cpp_column(lk["freq"])))
    return "\n            ".join(out)


CPP_BUILDER = r"""
#include <stdio.h>
#include "air_ir.h"
using namespace starkhip;
static void own(AirBuilder& b, uint32_t degree) {
    b.constraint(b.L(1) - b.L(0) * b.L(0));
    if (degree == 2) b.constraint(b.L(2) - b.L(0) * b.L(1));
    else if (degree == 3) b.constraint(b.L(2) - b.L(0) * b.L(0) * b.L(0));
    else {
        b.constraint(b.L(2) - b.L(1) * b.L(1) * b.L(0));
        b.constraint(b.L(0) * b.L(1) * (b.L(2) - b.L(1) * b.L(1) * b.L(0)));
    }
    b.transition(b.N(0) - b.L(0) - 1);
    b.first_row(b.L(0) - b.PI(0));
}
int main() {
%s
    return 0;
}
"""
CPP_ONE = r"""
    {
        AirBuilder b(%d, 1, %d);
        own(b, %d);
        {
            %s
        }
        printf("%s");
        for (uint64_t w : b.finish().serialize()) printf(" %%llx", (unsigned long long)w);
        printf("\n");
    }
"""


def test_cpp_and_python_builders_emit_the_same_words(tmp_path):
    body = "".join(CPP_ONE % (c.n_cols, c.degree, c.degree, _cpp_case(c), name) for name, c in G.CASES.items())
    assert "b.logup(" in body and "b.logup_columns(" in body and "filter_of({{" in body
    src = tmp_path / "logup_columns_builder.cpp"
    src.write_text(CPP_BUILDER % body)
    exe = tmp_path / "logup_columns_builder"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "starky_bls12_381_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert len(lines) == len(G.CASES)
    for line in lines:
        f = line.split()
        assert [int(x, 16) for x in f[1:]] == [int(x) for x in G.CASES[f[0]].blob()], f[0]


def _refused(blob, needle):
    why = S.air_check_program(np.array(blob, dtype=np.uint64))
    assert why is not None and needle in why, why
    with pytest.raises(S.StarkhipError) as e:
        S.register_air(np.array(blob, dtype=np.uint64))
    assert e.value.code == S.ERR_BAD_AIR


def test_every_refusal_of_the_section():
    base = [int(x) for x in _builder().finish()]  # 6 columns, degree 3, no section
    col = lambda c: [1, 0, c, 1]  # noqa: E731  a plain COLUMN
    good = base + [MAGIC2, 1, 1] + col(2) + col(3) + col(0) + [0]
    assert S.air_check_program(np.array(good, dtype=np.uint64)) is None
    sec = lambda *w: base + [MAGIC2] + list(w)  # noqa: E731
    # a trace column >= n_cols: in the table, the frequencies, a value, a filter's product and its sum
    _refused(sec(1, 1, *col(6), *col(3), *col(0), 0), "table: column 6 out of range")
    _refused(sec(1, 1, *col(2), *col(1 << 32), *col(0), 0), "frequencies: column 4294967296 out of range")
    _refused(sec(1, 1, *col(2), *col(3), 1 << 32, 0, 7, 1, 0), "column 0: column 7 out of range")
    _refused(sec(1, 1, *col(2), *col(3), *col(0), 1, *col(1), *col(9)), "filter: column 9 out of range")
    _refused(sec(1, 1, *col(2), *col(3), *col(0), 1 << 32, *col(6)), "filter: column 6 out of range")
    # coefficients and constants
    _refused(sec(1, 1, *col(2), *col(3), 1, 0, 0, 0, 0), "coefficient is zero")
    _refused(sec(1, 1, *col(2), *col(3), 1, 0, 0, P, 0), "coefficient is not canonical")
    _refused(sec(1, 1, *col(2), *col(3), 1, P, 0, 1, 0), "constant is not canonical")
    # 16 terms fit (local and next together), 17 do not
    terms = [x for k in range(17) for x in (k % 6, k + 1)]
    assert S.air_check_program(np.array(sec(1, 1, *col(2), *col(3), 9 | (7 << 32), 0, *terms[:32], 0), dtype=np.uint64)) is None
    _refused(sec(1, 1, *col(2), *col(3), 9 | (8 << 32), 0, *terms, 0), "17 terms")
    # 4 products and 4 sums fit, 5 of either do not
    assert S.air_check_program(np.array(sec(1, 1, *col(2), *col(3), *col(0), 4 | (4 << 32), *(col(1) * 12)), dtype=np.uint64)) is None
    _refused(sec(1, 1, *col(2), *col(3), *col(0), 5 | (4 << 32), *(col(1) * 14)), "5 products")
    _refused(sec(1, 1, *col(2), *col(3), *col(0), 4 | (5 << 32), *(col(1) * 13)), "5 sums")
    # an empty lookup, no lookups, more than 64 lookups, more than 64 columns
    _refused(sec(1, 0, *col(2), *col(3)), "empty lookup")
    _refused(sec(0), "lookups")
    one = [1] + col(2) + col(3) + col(0) + [0]
    _refused(sec(65, *(one * 65)), "lookups")
    assert S.air_check_program(np.array(sec(1, 64, *col(2), *col(3), *((col(0) + [0]) * 64)), dtype=np.uint64)) is None
    _refused(sec(1, 65, *col(2), *col(3), *((col(0) + [0]) * 65)), "columns")
    # nA above 1024: at degree 2 a lookup of 64 columns has 65 polynomials per challenge -- seven are 910, eight 1040
    base2 = [int(x) for x in _builder(degree=2).finish()]
    big = [64] + col(2) + col(3) + (col(0) + [0]) * 64
    assert S.air_check_program(np.array(base2 + [MAGIC2, 7] + big * 7, dtype=np.uint64)) is None
    _refused(base2 + [MAGIC2, 8] + big * 8, "auxiliary polynomials")
    # degree 1
    b = AirBuilder(4, 0, 1)
    b.constraint(b.L(0) - b.L(1))
    _refused([int(x) for x in b.finish()] + [MAGIC2, 1] + one, "degree")
    # pairs beside it, in either order; a section of either version beside the other, in either order
    b = _builder()
    b.permutation_pair([(0, 1)])
    pairs = [int(x) for x in b.finish()]
    _refused(pairs + good[len(base):], "together")
    _refused(good + pairs[len(base):], "together")
    first = [R.AIR_LOGUP_MAGIC, 1, 1, 2 | (3 << 32), 0]
    assert S.air_check_program(np.array(base + first, dtype=np.uint64)) is None
    _refused(good + first, "both versions")
    _refused(base + first + good[len(base):], "both versions")
    # trailing words, a section cut short anywhere
    _refused(good + [0], "trailing")
    _refused(good[:len(base) + 1], "shorter")
    for cut in range(len(base) + 2, len(good)):
        _refused(good[:cut], "past the blob")
    # the Python builder refuses what it can see
    b = _builder()
    with pytest.raises(ValueError):
        b.logup_columns([(Column([(6, 1)]), None)], 2, 3)
    with pytest.raises(ValueError):
        b.logup_columns([(Column([(0, P)]), None)], 2, 3)


def test_fuzzed_sections_that_pass_are_in_bounds():
    """single-word mutations of a section: whatever the validator accepts the reference reads to its last word, within every limit"""
    blob = G.CASES["big_filter"].blob()
    at = _section(blob)
    rng = np.random.default_rng(20261021)
    interesting = [0, 1, 2, 3, 4, 5, 16, 17, 19, 20, 1 << 32, 4 << 32, 5 << 32, (1 << 32) | 1, P - 1, P, (1 << 64) - 1, MAGIC2, R.AIR_LOGUP_MAGIC]
    passed = 0
    for trial in range(1500):
        t = blob.copy()
        i = int(rng.integers(at + 1, len(t)))
        t[i] = interesting[int(rng.integers(len(interesting)))] if trial % 3 else int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 63))
        if S.air_check_program(t) is not None:
            continue
        passed += 1
        _, lookups = G.split_program(t)  # asserts the section's own length
        assert 1 <= len(lookups) <= 64 and G.n_polys(lookups, 5) <= 1024
        for lk in lookups:
            cols = [lk["table"], lk["freq"]] + [v for v, _ in lk["pairs"]] + [c for _, (pr, su) in lk["pairs"] for c in [x for ab in pr for x in ab] + su]
            assert 1 <= len(lk["pairs"]) <= 64 and all(len(pr) <= 4 and len(su) <= 4 for _, (pr, su) in lk["pairs"])
            for const, local, nxt in cols:
                assert const < P and len(local) + len(nxt) <= 16 and all(c < 20 and 0 < k < P for c, k in local + nxt)
    assert passed >= 20


# ------------------------------------------------------------------------------------------------ polynomials, frequencies, constraints
def test_the_trace_of_the_issue_closes_by_hand():
    """n = 8, degree 3, the three Columns of "mixed": the sums close and every helper and step constraint is 0 on every row, the wrap
    row included -- in this file's own integers, from the definitions"""
    air, blob, case, lookups = columns_air("mixed")
    trace, _ = G.make_trace(case, 8, seed=1)
    rows = trace.tolist()
    lk = lookups[0]
    (v0, f0), (v1, f1), (v2, f2) = lk["pairs"]
    assert v0[2] == [(5, P - 1)] and f0 == ([], []) and f1 == ([], [G.plain(7)]) and v2 == (9, [], []) and len(f2[0]) == 1
    assert all(G.filter_value(f2, rows[r], rows[(r + 1) % 8]) == 0 for r in range(8))
    assert G.frequencies(lookups, rows)[0] == [int(x) for x in trace[:, 10]] and sum(rows[r][10] for r in range(8)) == 8 + sum(rows[r][7] for r in range(8))
    polys, closing, zeros = G.polys_and_closing(lookups, 3, rows, G.CHALLENGES)
    assert closing == [[0], [0]] and zeros == 0
    for i, chi in enumerate(G.CHALLENGES):
        h0, h1, z = polys[3 * i:3 * i + 3]
        for r in range(8):
            row, nxt = rows[r], rows[(r + 1) % 8]
            x = [(chi + G.column_value(v, row, nxt)) % P for v, _ in lk["pairs"]]
            phi = [G.filter_value(f, row, nxt) for _, f in lk["pairs"]]
            assert (h0[r] * x[0] * x[1] - phi[0] * x[1] - phi[1] * x[0]) % P == 0 and (h1[r] * x[2] - phi[2]) % P == 0
            den = (chi + row[3]) % P
            assert ((z[(r + 1) % 8] - z[r]) * den - (h0[r] + h1[r]) * den + row[10]) % P == 0
        assert z[0] == 0


@pytest.mark.parametrize("n_rows", [2, 64])
@pytest.mark.parametrize("name", list(G.CASES))
def test_polys_replay_is_the_references(name, n_rows):
    air, blob, case, lookups = columns_air(name)
    trace, _ = G.make_trace(case, n_rows, seed=n_rows + len(name), noncanonical=True)
    assert (trace >= np.uint64(P)).any()
    ref_polys, ref_closing, ref_zeros = G.polys_and_closing(lookups, case.degree, trace.tolist(), G.CHALLENGES)
    assert all(c == 0 for row in ref_closing for c in row) and ref_zeros == 0  # the reference alone says the trace closes
    for layout, t in ((0, trace), (1, np.ascontiguousarray(trace.T))):
        polys, closing, zeros = S.logup_polys_replay(air, t, G.CHALLENGES, layout=layout)
        assert polys.tolist() == ref_polys and closing.tolist() == ref_closing and zeros == 0
    bad = trace.copy()
    f = lookups[-1]["freq"][1][0][0]
    bad[n_rows // 2, f] = (int(bad[n_rows // 2, f]) + 1) % P
    ref_polys, ref_closing, _ = G.polys_and_closing(lookups, case.degree, bad.tolist(), G.CHALLENGES)
    assert ref_closing[0][-1] != 0 and ref_closing[1][-1] != 0
    polys, closing, zeros = S.logup_polys_replay(air, bad, G.CHALLENGES)
    assert polys.tolist() == ref_polys and closing.tolist() == ref_closing and zeros == 0


def test_zero_denominators_count_filtered_off_cells_too():
    air, blob, case, lookups = columns_air("mixed")
    trace, _ = G.make_trace(case, 64, seed=5)
    ch = [P - 9, (P - int(trace[3, 3])) % P]  # the constant Column 9 is filtered off on every row; a table cell
    ref = G.polys_and_closing(lookups, 3, trace.tolist(), ch)
    got = S.logup_polys_replay(air, trace, ch)
    assert got[2] == ref[2] >= 65 and got[0].tolist() == ref[0] and got[1].tolist() == ref[1]
    assert all(h == 0 for h in ref[0][1])  # the batch of the constant Column alone: a helper of zeros


def _freq_cols(lookups):
    return [lk["freq"][1][0][0] for lk in lookups]


@pytest.mark.parametrize("n_rows", [2, 64])
@pytest.mark.parametrize("name", G.FILLABLE)
def test_frequencies_replay_is_the_references(name, n_rows):
    air, blob, case, lookups = columns_air(name)
    assert S.air_logup_fillable(air) == 1
    trace, _ = G.make_trace(case, n_rows, seed=n_rows + 1, noncanonical=True)
    want = G.frequencies(lookups, trace.tolist())
    for layout in (0, 1):
        t = trace.copy()
        t[:, _freq_cols(lookups)] = 77
        arg = np.ascontiguousarray(t.T) if layout else t
        rep = S.logup_frequencies_replay(air, arg, layout=layout)
        assert (rep.failed, rep.missing_cells, rep.missing_rows) == (0, 0, 0)
        got = arg.T if layout else arg
        for f, w in zip(_freq_cols(lookups), want):
            assert got[:, f].tolist() == w
        others = [c for c in range(t.shape[1]) if c not in _freq_cols(lookups)]
        assert np.array_equal(got[:, others], trace[:, others])
        assert S.logup_blob_replay(air, arg, layout=layout) is None


def test_the_fill_skips_flags_and_misses():
    air, blob, case, lookups = columns_air("mixed")
    trace, _ = G.make_trace(case, 64, seed=9)
    on, off = int(np.nonzero(trace[:, 7] == 1)[0][2]), int(np.nonzero(trace[:, 7] == 0)[0][2])
    skipped = trace.copy()
    skipped[off, 6] = 1 << 20  # outside the table, filtered off: not looked up
    skipped[:, 10] = 77
    assert S.logup_frequencies_replay(air, skipped).failed == 0 and np.array_equal(skipped[:, 10], trace[:, 10])
    bad = trace.copy()
    bad[:, 10] = 77
    bad[on, 6] = 1 << 20  # filtered on: missing
    bad[off, 7] = 2       # a filter that is neither 0 nor 1: flagged, whatever the cell holds
    assert G.frequencies(lookups, bad.tolist()) == [None]
    t = bad.copy()
    rep = S.logup_frequencies_replay(air, t)
    assert (rep.failed, rep.missing_cells, rep.missing_rows) == (1, 2, 2) and rep.per_column.tolist() == [0, 2, 0]
    assert rep.list.tolist() == sorted([[0, on], [0, off]]) and np.array_equal(t, bad)  # nothing is written
    blob_words = S.logup_blob_replay(air, bad)
    layout = S.logup_blob_layout(blob_words)
    assert (layout.failed, layout.missing_cells, layout.missing_rows) == (1, 2, 2) and layout.list.tolist() == rep.list.tolist()


def test_what_is_fillable():
    assert S.air_logup_fillable(columns_air("freq_comb")[0]) == 0  # frequencies that are a combination
    t, _ = G.make_trace(G.CASES["freq_comb"], 8, 1)
    with pytest.raises(S.StarkhipError) as e:
        S.logup_frequencies_replay(columns_air("freq_comb")[0], t)
    assert e.value.code == S.ERR_BAD_SHAPE
    for declare in (lambda b: b.logup_columns([(Column([(0, 1), (3, 1)]), None)], 2, 3),                   # a value reads the frequencies column
                    lambda b: b.logup_columns([(0, Filter(sums=[3]))], 2, 3),                                # a filter does
                    lambda b: b.logup_columns([(0, None)], Column([(2, 1)], [(3, 1)]), 3),                   # the table does, on the next row
                    lambda b: (b.logup_columns([(0, None)], 2, 3), b.logup_columns([(1, None)], 2, 3))):     # two lookups, one frequencies column
        b = _builder()
        declare(b)
        assert S.air_logup_fillable(S.register_air(b.finish())) == 0
    b = _builder()
    b.logup_columns([(Column([(0, 1)], [(0, 1)]), Filter(sums=[4]))], Column([(2, 1), (1, 2)]), 3)
    assert S.air_logup_fillable(S.register_air(b.finish())) == 1


@pytest.mark.parametrize("name", list(G.CASES))
def test_eval_frame_logup_is_the_references(name):
    air, blob, case, lookups = columns_air(name)
    base = G.split_program(blob)[0]
    na, cols, nl = S.air_logup_polys(air), S.air_columns(air), G.n_constraints(lookups, case.degree)
    rng = np.random.default_rng(len(name))
    for trial in range(2):
        ext = lambda k: rng.integers(0, P, size=(k, 2), dtype=np.uint64)  # noqa: E731
        local, nxt, aux, aux_next, masks, alphas = ext(cols), ext(cols), ext(na), ext(na), ext(4), ext(2)
        pis = rng.integers(0, P, 1, dtype=np.uint64)
        got = S.air_eval_frame_logup(air, local, nxt, pis, masks, alphas, aux, aux_next, G.CHALLENGES)
        tup = lambda a: [(int(x), int(y)) for x, y in a]  # noqa: E731
        mk = tup(masks)
        own = R.own_values_ext(base, tup(local), tup(nxt), pis, mk)
        lc = G.logup_constraints_ext(lookups, case.degree, tup(local), tup(nxt), tup(aux), tup(aux_next), G.CHALLENGES)
        assert len(lc) == nl
        assert tup(got) == [R.fold_full(own, lc, mk, a) for a in tup(alphas)]
    # a frame of words >= p gives the fold of the reduced frame
    big = local.copy()
    big[3, 0] = int(big[3, 0]) % (1 << 31) + P
    small = big.copy()
    small[3, 0] = int(big[3, 0]) - P
    assert np.array_equal(S.air_eval_frame_logup(air, big, nxt, pis, masks, alphas, aux, aux_next, G.CHALLENGES),
                          S.air_eval_frame_logup(air, small, nxt, pis, masks, alphas, aux, aux_next, G.CHALLENGES))


# ------------------------------------------------------------------------------------------------ the golden proofs
@pytest.fixture(scope="module")
def golden():
    air, blob, cfg, trace, pis = golden_case()
    return air, blob, cfg, load_golden()


def test_golden_file_is_small_and_has_both_hashers(golden):
    air, blob, cfg, proofs = golden
    assert os.path.getsize(GOLDEN) < 1 << 20 and sorted(proofs) == [S.HASHER_POSEIDON, S.HASHER_KECCAK]
    for hasher, proof in proofs.items():
        assert S.proof_hasher(proof) == hasher and (int(proof[13]), int(proof[14]), int(proof[15])) == (0, 6, 0)
        assert int(S.proof_layout(proof).degree_bits) == 5


def test_golden_proofs_are_accepted_by_all_three_verifiers(golden):
    air, blob, cfg, proofs = golden
    for hasher, proof in proofs.items():
        assert cpu_code(air, cfg, proof) == 0
        assert S.verify_batch_replay([(air, cfg, proof)]) == [0]
        G.verify_or_raise(blob, cfg, proof, hasher)
    assert S.verify_batch_replay([(air, cfg, proofs[0]), (air, cfg, proofs[1])]) == [0, 0]


def test_one_changed_word_is_rejected(golden):
    """any single word of the auxiliary openings (at zeta and at the next row's point), of the next-row opening of column 5 -- which
    only a next-row term reads -- and of the auxiliary cap"""
    air, blob, cfg, proofs = golden
    for hasher, proof in proofs.items():
        L = S.proof_layout(proof)
        ncap = 1 << cfg.cap_height
        places = list(range(int(L.off_permutation_zs), int(L.off_permutation_zs) + 4 * 6))         # aux and aux_next, 6 pairs each
        places += [int(L.off_next_values) + 2 * 5, int(L.off_next_values) + 2 * 5 + 1]
        places += list(range(int(L.off_permutation_zs_cap), int(L.off_permutation_zs_cap) + 4 * ncap))
        assert int(L.off_permutation_zs_next) == int(L.off_permutation_zs) + 12
        for at in places:
            t = proof.copy()
            t[at] = (int(t[at]) + 1) % P
            assert cpu_code(air, cfg, t) == S.ERR_VERIFY, (hasher, at)
            assert not G.verify(blob, cfg, t, hasher), (hasher, at)
        flips = logup_flips(proof)
        assert S.verify_batch_replay([(air, cfg, t) for t in flips.values()]) == [S.ERR_VERIFY] * 5
        for name, t in flips.items():
            with pytest.raises(K.Reject):
                G.verify_or_raise(blob, cfg, t, hasher)


def test_rust_mirror_has_the_new_name():
    with open(os.path.join(ROOT, "bindings", "rust", "starkhip-sys", "src", "lib.rs")) as f:
        assert "pub fn starkhip_air_logup_general(air: c_int) -> c_int;" in f.read()
