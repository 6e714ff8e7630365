"""test_check_report_cpu.py's checks of starkhip_check_trace_report_replay on seed 1 of random_air.CASES: one column, 8 rows, one
first-row constraint.  Every one-column random AIR has that same program, and test_custom_air_cpu.py expects to be the first to register
it in a process, so this case lives in a file that is collected after that one."""
import pytest

import starky_bls12_381_amd as S
from check_report_util import case, check_caps, check_clean, check_corrupted
from random_air import CASES


@pytest.fixture(scope="module")
def air():
    assert CASES[0] == (1, 1, 2, 8)
    return S.register_air(case(0)[0])


def test_clean_trace_gives_an_all_zero_report(air):
    check_clean(air, 0)


def test_corrupted_trace_is_reported_as_the_oracle_sees_it(air):
    assert case(0)[4].violations == 1  # the first-row constraint, on row 0 only: rows 1 .. 7 are nonzero too and do not count
    check_corrupted(air, 0)


def test_cap_cuts_the_list_and_nothing_else(air):
    check_caps(air, 0)
