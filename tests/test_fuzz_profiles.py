"""tools/fuzz_search.py's draws, on the CPU.

The general draw (no profile) must consume the random stream exactly as it did before the profiles existed: the suite's fixed-seed fuzz
(tests/test_gpu_retrieval.py::test_fuzz_across_dispatch_boundaries_bit_exact) then keeps the very cases it has always run.
tests/golden/fuzz_draws_default.json.gz holds 500 draws for each of three seeds as draw_case returned them before it took a profile
(this project's own output, written as sorted compact JSON).  The profiles are held to what they are for."""
import gzip
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fuzz_draws_default.json.gz")


@pytest.fixture(scope="module")
def fz():
    spec = importlib.util.spec_from_file_location("fuzz_search", os.path.join(ROOT, "tools", "fuzz_search.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(autouse=True)
def _no_profile_in_the_environment(monkeypatch):
    monkeypatch.delenv("VF_FUZZ_SCAN2R", raising=False)
    monkeypatch.delenv("VF_FUZZ_WIDE_ROWS", raising=False)


def test_general_draw_consumes_the_stream_as_recorded(fz):
    with gzip.open(FIXTURE, "rb") as f:
        want = json.loads(f.read())
    assert sorted(want["seeds"]) == ["1", "20260404", "777"] and want["draws"] == 500
    for seed, cases in want["seeds"].items():
        rng = np.random.default_rng(int(seed))
        assert len(cases) == want["draws"]
        for i, w in enumerate(cases):
            got = json.loads(json.dumps(fz.draw_case(rng, want["max_work"])))
            assert got == w, (seed, i, got, w)
        # ... and the generator is where it was: the next draw of the recorded run would be the next draw of this one
    rng_a, rng_b = np.random.default_rng(5), np.random.default_rng(5)
    assert [fz.draw_case(rng_a, 1e10) for _ in range(50)] == [fz.draw_case(rng_b, 1e10, profile=None) for _ in range(50)]


def test_environment_variables_select_their_profiles(fz, monkeypatch):
    assert fz.env_profile() is None
    draws = lambda profile: [fz.draw_case(np.random.default_rng(3), 1e10, profile) for _ in range(1)][0]
    monkeypatch.setenv("VF_FUZZ_WIDE_ROWS", "1")
    assert fz.env_profile() == "wide_rows" and draws(None) == draws("wide_rows")
    monkeypatch.setenv("VF_FUZZ_SCAN2R", "1")                # (the first of the two wins, as before)
    assert fz.env_profile() == "scan2r" and draws(None) == draws("scan2r")
    with pytest.raises(AssertionError):
        fz.draw_case(np.random.default_rng(3), 1e10, "no-such-profile")


def test_int8_profile_draws_what_it_is_for(fz):
    rng = np.random.default_rng(11)
    cases = [fz.draw_case(rng, 4e9, "int8") for _ in range(400)]
    assert all(c["dtype"] == "int8" for c in cases)
    assert {c["d"] for c in cases} == {1, 7, 100, 128, 768, 1000, 1024, 1536, 2048, 2432}
    assert {c["opts"]["scan_image"] for c in cases} == {0, 1, 2} and {c["opts"]["image_mfma"] for c in cases} == {-1, 0, 1, 2}
    assert sum(c["k"] <= 128 for c in cases) > 200 and any(c["k"] > 128 for c in cases)
    assert any(c["data"] == "raw" for c in cases) and any(c["shards"] > 1 for c in cases)
    assert all(1 <= c["k"] <= 2048 and float(c["n"]) * c["nq"] * c["d"] <= 4e9 or c["n"] <= 17000 for c in cases)
    assert any(c["n"] <= 16384 for c in cases) and any(c["n"] > 16384 and c["nq"] >= 129 for c in cases)


def test_wide_rows_profile_draws_int8_on_both_sides_of_its_floor(fz):
    rng = np.random.default_rng(12)
    cases = [fz.draw_case(rng, 4e9, "wide_rows") for _ in range(300)]
    assert all(2433 <= c["d"] <= 4096 and c["opts"]["wide_rows"] == 2 for c in cases)
    assert {c["dtype"] for c in cases} == {"f16", "f32", "fp8", "int8"}
    n8 = {c["n"] for c in cases if c["dtype"] == "int8"}
    assert min(n8) < 32768 and 32768 in n8 and max(n8) > 32768, n8


def test_int8_data_kinds_are_int8_codes_and_their_float_values(fz):
    for data in ("normal", "zeros", "raw", "scaled"):
        codes, rows, q = fz.make_data(dict(dtype="int8", d=33, nq=3, n=300, k=5, data=data, seed=9))
        assert codes.dtype == np.int8 and codes.shape == (300, 33) and rows.dtype == np.float32 and q.shape == (3, 33)
        assert np.array_equal(rows, codes.astype(np.float32))
        if data == "raw":
            assert codes.min() == -128 and codes.max() == 127
        else:
            assert codes.min() >= -127
