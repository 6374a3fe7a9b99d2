"""The word arithmetic of a filtered BM25 search (veritasfi_amd/csrc/vf_bm25_filter.h), EXECUTED on the CPU: a host-compiled driver
(tests/bm25_filter_driver.py, UBSan) runs a filtered call the way the entry point and the kernels do and holds it to the plain
definition -- the allowed rows in canonical order, cut to k, then padding.  No GPU.

Every n <= 12 with every filter, every touched set and k in {1, 2, n}; seeded filters and touched sets at n in {31, 32, 33, 63, 64,
65, 32767, 32768, 32769, 65537}, where words and bitmap blocks end; and the bitmap check, which names the first bit at or past n."""
import pytest

import bm25_filter_driver as drv


@pytest.fixture(scope="module")
def outcome(tmp_path_factory):
    return drv.run(drv.build(tmp_path_factory.mktemp("bm25_filter_plan")))


def _clean(run):
    print(run.stdout[-3000:])
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.stdout[-3000:], run.stderr[-3000:])
    assert "bm25 filter plan: 0 failure(s)" in run.stdout


def test_every_filter_and_touched_set_of_up_to_12_rows_gives_the_plain_sort_then_padding(outcome):
    _clean(outcome)
    assert f"exhaustive: {drv.expected_exhaustive_cases()} cases" in outcome.stdout


def test_word_and_block_boundaries_give_the_plain_sort_then_padding(outcome):
    _clean(outcome)
    # 10 sizes x 4 filter densities x 4 touched densities x the k of {1, 2, 100, 4096, 4097, n} that fit
    fit = sum(sum(1 for k in (1, 2, 100, 4096, 4097, n) if k <= n) for n in (31, 32, 33, 63, 64, 65, 32767, 32768, 32769, 65537))
    assert f"random: {16 * fit} cases" in outcome.stdout


def test_the_bitmap_check_names_the_first_bit_at_or_past_n(outcome):
    _clean(outcome)
    past = sum((n + 31) // 32 * 32 - n for n in (1, 5, 31, 33, 63, 70001))
    assert f"check: {2 * past} cases" in outcome.stdout
