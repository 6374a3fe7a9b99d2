"""The metadata filter's program and output geometry (veritasfi_amd/csrc/vf_where.h), EXECUTED on the CPU: a host-compiled driver
(tests/where_driver.py, UBSan) runs the interpreter the kernel runs, the kernels' walk over tiles and the program checker.  No GPU.

What the device relies on: where_eval_row -- a stack in the bits of one word -- equals a recursive evaluation for every program shape of
up to 3 leaves on every row of a 12-row, 2-column table under all 4096 validity patterns; walking tiles of 64, 128 and 1024 rows at the
row counts around every word and tile boundary writes each bitmap word exactly once with zero tail bits, and the counts, their prefix
and the rank rule put every passing row's id where a plain loop puts it; where_validate names the first offending position of a
program that underflows, leaves values over, goes 33 deep, names column 16, or holds a set run that is not ascending."""
import pytest

import where_driver as drv


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("where_plan"))


@pytest.mark.parametrize("what", ["programs", "tiles", "validate"])
def test_where_plan(exe, what):
    run = drv.run(exe, what)
    print(run.stdout[-3000:])
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.stdout[-3000:], run.stderr[-3000:])
    assert " 0 failure(s)" in run.stdout
