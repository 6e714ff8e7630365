"""What the cross-table-lookup tests (CPU and GPU) and the golden's maker share: the cases of ctl_ref registered once as systems, their
configs, the golden case.  Test code."""
import json
import os

import numpy as np

import ctl_ref as X
import starky_bls12_381_amd as S
from logup_util import logup_config
from starky_bls12_381_amd.air_builder import Column, Filter, SystemBuilder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctl_small.json")
GOLDEN_CASE, GOLDEN_ROWS, GOLDEN_SEED = "range", (32, 16), 7
GOLDEN_TWO_CASE, GOLDEN_TWO_ROWS = "two_lookers", (16, 8, 8)  # the second golden system: two looking sums to move against each other

_SYSTEMS = {}


def to_column(col):
    const, local, nxt = col
    return Column(local, nxt, const)


def to_filter(flt):
    products, sums = flt
    return Filter([(to_column(a), to_column(b)) for a, b in products], [to_column(c) for c in sums])


def to_endpoint(ep):
    return (ep[0], [to_column(c) for c in ep[1]], to_filter(ep[2]))


def system_blob(airs, ctls):
    sb = SystemBuilder(airs)
    for looked, looking in ctls:
        sb.ctl(to_endpoint(looked), [to_endpoint(e) for e in looking])
    return sb.finish()


def ctl_system(name):
    """(system id, [air ids], [program blobs], case) of ctl_ref.CASES[name], registered once per process"""
    if name not in _SYSTEMS:
        case = X.CASES[name]
        blobs = [t.blob() for t in case.tables]
        airs = [S.register_air(b, name="Ctl_%s_%d" % (name, i)) for i, b in enumerate(blobs)]
        _SYSTEMS[name] = (S.register_system(system_blob(airs, case.ctls)), airs, blobs, case)
    return _SYSTEMS[name]


def configs(case, num_query_rounds=3, rows=None):
    """one config per table: standard_fast with the smallest rate_bits the table's degree admits; with `rows`, the cap height every table
    shares lowered to what the shortest table's LDE has room for (2 rows at rate_bits 1: four leaves, cap height 2)"""
    cfgs = [logup_config(t.degree, num_query_rounds) for t in case.tables]
    if rows is not None:
        cap = min([cfgs[0].cap_height] + [int(n).bit_length() - 1 + c.rate_bits for n, c in zip(rows, cfgs)])
        for c in cfgs:
            c.cap_height = cap
    return cfgs


def golden_case():
    """(system, blobs, case, configs, [(trace, public inputs)]) of the golden proofs: "range" at 32 and 16 rows, 3 query rounds"""
    system, _, blobs, case = ctl_system(GOLDEN_CASE)
    return system, blobs, case, configs(case), X.make_traces(case, GOLDEN_ROWS, GOLDEN_SEED)


def golden_two_case():
    """the same of the second golden system: "two_lookers" at 16, 8 and 8 rows"""
    system, _, blobs, case = ctl_system(GOLDEN_TWO_CASE)
    return system, blobs, case, configs(case), X.make_traces(case, GOLDEN_TWO_ROWS, GOLDEN_SEED)


def load_golden(key="proofs_hex"):
    """{hasher id: system proof} of tests/golden/ctl_small.json (tests/make_ctl_golden.py wrote it on the GPU); key: "proofs_hex" (the case
    "range"), "other_proofs_hex" (the same looking trace beside another table trace) or "two_lookers_proofs_hex" (the case "two_lookers")"""
    with open(GOLDEN) as f:
        d = json.load(f)
    return {int(h): np.array([int(x, 16) for x in words], dtype=np.uint64) for h, words in d[key].items()}


def cpu_code(system, cfgs, proof):
    try:
        S.verify_system_proof(system, cfgs, proof)
        return 0
    except S.StarkhipError as e:
        return e.code
