"""The plan a subset search runs by (veritasfi_amd/csrc/vf_subset.h), decided and EXECUTED on the CPU: a host-compiled driver
(tests/subset_plan_driver.py, UBSan) runs the super-chunk / rank-chunk / merge-buffer scheme on integer arrays.  No GPU.

What the device relies on, for every n <= 12, every subset, every super-chunk and rank-chunk size and several k: the super-chunks tile
the list and fit the score workspace, the rank chunks tile each super-chunk, no part lands beyond the merge buffer, the folds end in
one list after the planned number of rounds, and that list mapped through the subset is the plain ranking of the listed rows (score
descending, ties to the lower id).  Random cases of up to 2^32 - 2 rows hold the arithmetic to 64 bits, the score workspace to 64 MB,
fan-in x k to the 16 384 keys of the merge kernel and the kernel's LDS to one query tile of one K-slice for every d <= 8192."""
import pytest

import subset_plan_driver as drv


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("subset_plan"))


@pytest.mark.parametrize("what", ["small", "large", "lists"])
def test_subset_plan(exe, what):
    run = drv.run(exe, what)
    print(run.stdout[-3000:])
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.stdout[-3000:], run.stderr[-3000:])
    assert " 0 failure(s)" in run.stdout
