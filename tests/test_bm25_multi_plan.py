"""A BM25 batch with a prepared filter per query (veritasfi_amd/csrc/vf_bm25_multi.h), EXECUTED on the CPU: a host-compiled driver
(tests/bm25_multi_driver.py, UBSan) replays a two-slot group of the 12-row index as the _m kernels run it -- each slot's scatter marks,
tail words and padding chosen by its own descriptor -- and holds every slot to vf_bm25_filter.h's one-filter replay of that slot alone.
Slot 0 runs through all 4096 filters; slot 1 holds a fixed other filter (corpus and subset form), no filter, and the empty filter.
numpy says once more, on its own, what slot 0 and slot 1 must hold.  Then the plan at n in {1, 31, 32768, 32769, 70001}, k in
{1, 4096, 4097, n} where they fit and nq in {1, slot_cap, slot_cap + 1}.  No GPU."""
import numpy as np
import pytest

import bm25_multi_driver as drv
from test_bm25_prepared_plan import _zipf
from veritasfi_amd import bm25 as B

N, VOCAB = 12, 16
FIXED = 0b101101100110            # slot 1's filter: rows 1, 2, 5, 6, 8, 9, 11
KS = [1, 5, 12]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("bm25_multi_plan"))


def _numpy_ranks(indptr, indices, query, mask, k):
    """touched rows ascending cut to k, then the allowed untouched rows ascending, then -1: ``mask`` None is the unfiltered query"""
    allowed = np.ones(N, bool) if mask is None else np.array([(mask >> r) & 1 for r in range(N)], bool)
    touched = np.zeros(N, bool)
    for c in query:
        touched[indices[indptr[c]:indptr[c + 1]]] = True
    touched &= allowed
    rows = np.concatenate([np.flatnonzero(touched), np.flatnonzero(allowed & ~touched)])[:k]
    return rows.tolist() + [-1] * (k - rows.size)


def test_a_two_slot_group_under_every_filter_is_two_one_filter_calls_and_the_plan_is_the_one_filter_plan(exe, tmp_path):
    off, toks = _zipf(N, VOCAB, 3, seed=3)
    indptr, indices, _ = B.bm25_index_arrays(off, toks, VOCAB)
    per = np.diff(indptr)
    assert indices.size == 31 and int((per == 0).sum()) == 1, per
    common = np.argsort(-per, kind="stable")
    queries = [[int(common[0]), int(common[2]), int(common[0])], [int(common[1]), int(common[5])]]
    touched0 = np.zeros(N, bool)
    for c in queries[0]:
        touched0[indices[indptr[c]:indptr[c + 1]]] = True
    assert 0 < int(touched0.sum()) < N, "slot 0's query leaves a tail and touches rows"
    plans = []
    for n in (1, 31, 32768, 32769, 70001):
        for k in sorted({1, 4096, 4097, n}):
            if k <= n:
                for cap in (64, 2):
                    plans += [(n, k, nq, cap) for nq in (1, cap, cap + 1)]
    out = drv.run(exe, drv.write_input(tmp_path / "in.txt", N, indptr, indices, queries, FIXED, KS, plans))
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "runtime error" not in out.stderr, (out.stdout[-3000:], out.stderr[-3000:])
    assert "multi: 0 failure(s)" in out.stdout
    rows, got_plans = drv.parse(out.stdout)
    assert len(rows) == 4096 * len(KS)
    for k in KS:
        want1 = _numpy_ranks(indptr, indices, queries[1], FIXED, k)
        for f in range(4096):
            s0, s1 = rows[(f, k)]
            assert s0 == _numpy_ranks(indptr, indices, queries[0], f, k), (f, k)
            assert s1 == want1, (f, k)
    assert len(got_plans) == len(plans)
    for n, k, nq, cap in plans:
        blocks = -(-(-(-n // 32)) // 1024)
        small = k <= 4096
        S = min(nq, cap) if small else 1
        assert got_plans[(n, k, nq, cap)] == (S, int(small), blocks, blocks if small else 0, -(-nq // S)), (n, k, nq, cap)
