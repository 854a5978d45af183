"""The GEMM launch layer does what tests/golden/gemm_launch_trace.json recorded (tests/gemm_launch_trace.py: rows, inputs, what a record
holds): same kernel builds, launch counts and KernelTimer arguments, same note_kernel report, bit-identical outputs, on both matrix
paths.  The golden is regenerated only by a commit that means to change a launch or a kernel's arithmetic (NOTES.md)."""
import json

import pytest

import gemm_launch_trace as T

pytestmark = pytest.mark.gpu

ROWS = T.rows()


@pytest.fixture(scope="module")
def golden():
    T.setup_device()
    with open(T.GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_the_rows_of_the_helper(golden):
    assert list(golden) == [c.id for c in ROWS]


def test_the_three_blocks_per_cu_row_ran_that_build_when_the_golden_was_recorded(golden):
    """gg_launch_cfg takes the 768-slot gg_kernel build from 2 x 768 tiles on, on matrix path 0 only; its timer name is the plain build's"""
    rec = golden[T.O3_ROW]["fp32"]
    assert [l.split("|")[0] for l in rec["profile"]] == ["gg_kernel<2,2,2,128,rc>"] and rec["kernel"][1] >= 1536, rec


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_launches_and_output_bits_equal_the_recorded_trace(golden, case):
    got = T.record(case)
    diff = T.first_difference(got, golden[case.id])
    assert diff is None, (case.id,) + diff
