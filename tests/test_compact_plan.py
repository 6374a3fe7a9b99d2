"""The plan a removal moves its rows by (veritasfi_amd/csrc/vf_compact.h), decided and EXECUTED on the CPU: a host-compiled driver
(tests/compact_plan_driver.py, UBSan) runs the gather / scatter scheme of k_compact_rows on integer arrays.  No GPU.

What the device relies on, for every n <= 12, every subset of removed rows and every chunk size: the result is the plain deletion;
the chunks are disjoint, ascending and tile the moved range; a chunk fits the staging buffer; no chunk reads a row below the previous
chunk's destination end (so launch order on one stream is the only synchronisation) or past the array; nothing below the first
removed row is touched.  Random cases of up to 2^32 - 2 rows hold the arithmetic to 64 bits."""
import pytest

import compact_plan_driver as drv


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("compact_plan"))


@pytest.mark.parametrize("what", ["small", "large", "units"])
def test_compact_plan(exe, what):
    run = drv.run(exe, what)
    print(run.stdout[-3000:])
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.stdout[-3000:], run.stderr[-3000:])
    assert " 0 failure(s)" in run.stdout
