"""The plan of a dense batch whose queries each bring their own row list (veritasfi_amd/csrc/vf_subset_multi.h), decided and EXECUTED on
the CPU: a host-compiled driver (tests/subset_multi_driver.py, UBSan) runs passes, permutation, tiles, size classes, the scan's grid
with its sentinel rule, the per-class ranking and the map on integer arrays.  No GPU.

What the device relies on, for every assignment of up to 5 queries to 3 lists of a 12-row index under shrunken blocking: the
permutation is a bijection; a tile holds queries of one list only and at most q_tile of them; the tile count is the sum over the lists
of ceil(queries of the list / q_tile); walking the scan's grid writes every score slot of every class row exactly once, real or
sentinel, so nothing the ranking reads is uninitialised; rank + map equal the brute-force answer per query; launches per pass and score
bytes stay within the stated bounds.  Random calls at the real constants hold the same invariants, the 16 MB and the refusals."""
import pytest

import subset_multi_driver as drv


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("subset_multi_plan"))


@pytest.mark.parametrize("what", ["small", "large"])
def test_subset_multi_plan(exe, what):
    run = drv.run(exe, what)
    print(run.stdout[-3000:])
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.stdout[-3000:], run.stderr[-3000:])
    assert " 0 failure(s)" in run.stdout
