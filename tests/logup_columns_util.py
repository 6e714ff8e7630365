"""What the tests of LogUp lookups over Columns and Filters (CPU and GPU) and the golden's maker share: the cases of
logup_columns_ref registered once, plain lookups declared in either section, the golden case.  Test code."""
import json
import os

import numpy as np

import logup_columns_ref as G
import logup_ref as R
import starky_bls12_381_amd as S
from logup_util import logup_config
from starky_bls12_381_amd.air_builder import AirBuilder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logup_columns_small.json")
GOLDEN_CASE, GOLDEN_ROWS, GOLDEN_SEED = "mixed", 32, 7

_AIRS = {}


def columns_air(name):
    """(air id, blob, case, the reference's lookups) of logup_columns_ref.CASES[name], registered once per process"""
    if name not in _AIRS:
        case = G.CASES[name]
        blob = case.blob()
        _AIRS[name] = (S.register_air(blob, name="LogupColumns_" + name), blob, case, G.split_program(blob)[1])
    return _AIRS[name]


def plain_in_general_section(degree, m, n_lookups):
    """logup_ref.make_air(degree, m, n_lookups) with its plain lookups declared through logup_columns: the "LOGUPS02" blob"""
    b = AirBuilder(R.air_columns(m, n_lookups), 1, degree)
    G.own_constraints(b, degree)
    for l in range(n_lookups):
        cols, freq = R.lookup_columns(m, l)
        b.logup_columns([(c, None) for c in cols], R.TABLE_COL, freq)
    return b.finish()


def golden_case():
    """(air, blob, config, trace, public inputs) of the golden proofs: the case "mixed" (degree 3, a next-row term with coefficient
    p - 1, a selector filter, a constant Column under a product filter that is 0), 32 rows, 3 query rounds"""
    air, blob, case, _ = columns_air(GOLDEN_CASE)
    trace, pis = G.make_trace(case, GOLDEN_ROWS, GOLDEN_SEED)
    return air, blob, logup_config(case.degree, 3), trace, pis


def load_golden():
    """{hasher id: proof} of tests/golden/logup_columns_small.json (tests/make_logup_columns_golden.py wrote it on the GPU)"""
    with open(GOLDEN) as f:
        d = json.load(f)
    return {int(h): np.array([int(x, 16) for x in words], dtype=np.uint64) for h, words in d["proofs_hex"].items()}
