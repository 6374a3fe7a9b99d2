"""The generators and references of tests/rank_cases.py, held to the C oracle and to their own contract on the CPU, before a
GPU is involved: oracle.merge_topk and the NumPy merge_reference are two independent statements of the same ranking and must
agree bit for bit on every case that tests/test_gpu_rank_kernels.py runs."""
import numpy as np
import pytest

import rank_cases as RC
from oracle import ref_numpy


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", RC.MERGE_KINDS)
@pytest.mark.parametrize("nparts,k,nq", RC.MERGE_SHAPES)
def test_merge_case_keeps_the_precondition_and_both_references_agree(oracle, nparts, k, nq, kind):
    ids, scores = RC.merge_case(nparts, k, nq, kind, seed=1)
    assert ids.shape == scores.shape == (nparts, nq, k) and ids.dtype == np.int64 and scores.dtype == np.float32
    assert not np.isnan(scores).any()
    RC.check_merge_precondition(ids, scores)
    want_i, want_s = RC.merge_reference(ids, scores, k)
    got_i, got_s = oracle.merge_topk(ids, scores, k)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(_bits(got_s), _bits(want_s))


def test_merge_kinds_hold_what_they_are_named_for():
    real = lambda ids: int((ids >= 0).sum())   # noqa: E731
    for nparts, k, nq in RC.MERGE_SHAPES:
        ids, sc = RC.merge_case(nparts, k, nq, "empty", 1)
        assert real(ids) == 0
        ids, sc = RC.merge_case(nparts, k, nq, "short", 1)
        for q in range(nq):
            assert real(ids[:, q]) < k and all(real(ids[g, q]) < k for g in range(nparts))
            if nparts >= 3:
                assert real(ids[nparts // 2, q]) == 0
        ids, sc = RC.merge_case(nparts, k, nq, "extremes", 1)
        live = ids[:, 0] >= 0
        assert 0 < int(live.sum()) < max(k, 2) and (sc[:, 0][live] == -RC.FLT_MAX).any()   # a real entry with the padding score
        ids, sc = RC.merge_case(nparts, k, nq, "ties", 1)
        assert set(np.unique(sc[ids >= 0]).tolist()) <= {-1.0, 0.0, 0.5}
    # over the whole table: parts that overflow k, signed zeros of both signs, both infinities
    ids, sc = RC.merge_case(8, 256, 2, "ties", 1)
    zeros = sc[(ids >= 0) & (sc == 0)]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    ids, sc = RC.merge_case(8, 256, 2, "distinct", 1)
    assert any(real(ids[g, q]) == 256 for g in range(8) for q in range(2)) and real(ids[:, 0]) > 256
    ids, sc = RC.merge_case(5, 100, 64, "extremes", 1)
    assert np.isposinf(sc).any() and np.isneginf(sc).any() and (sc[ids >= 0] == -RC.FLT_MAX).any()
    assert ids[ids >= 0].min() >= 5 << 32


@pytest.mark.parametrize("kind", RC.FUSE_KINDS)
@pytest.mark.parametrize("n", RC.FUSE_SIZES + (155,))
def test_fuse_and_rank_is_a_stable_descending_permutation(n, kind):
    a, b = RC.fuse_case(n, kind, seed=2)
    assert a.shape == b.shape == (n,) and a.dtype == b.dtype == np.float32
    s = RC.fuse_sums(a, b)
    assert not np.isnan(s).any()
    with np.errstate(over="ignore"):
        order = ref_numpy.fuse_and_rank(a, b)
    assert np.array_equal(np.sort(order), np.arange(n))
    hi, lo = s[order[:-1]], s[order[1:]]
    assert np.all((hi > lo) | ((hi == lo) & (order[:-1] < order[1:])))      # equal floats tie: -0.0 == +0.0
    if n >= 4:
        if kind == "all_equal":
            assert np.unique(s).size == 1 and np.array_equal(order, np.arange(n))
        if kind == "two_valued":
            assert np.unique(s).size == 2
        if kind == "zeros":
            assert not s.any() and np.signbit(s[1::2]).all() and not np.signbit(s[0::2]).any()
            assert np.array_equal(order, np.arange(n))
        if kind == "inf":
            assert np.isposinf(s[0::4]).all() and np.isposinf(s[1::4]).all() and np.isneginf(s[2::4]).all()


def test_tied_corpus_rows_repeat_bit_for_bit():
    rows, vec = RC.tied_corpus(1000, 3, 32, seed=3)
    assert rows.shape == (1000, 32) and rows.dtype == np.float32 and vec.shape == (3, 32)
    for i in (0, 1, 2, 500, 999):
        assert np.array_equal(rows[i].view(np.uint32), vec[i % 3].view(np.uint32))
    assert np.allclose(np.linalg.norm(vec.astype(np.float64), axis=1), 1.0, atol=1e-6)
    q = RC.tied_queries(vec, 3)
    assert q.shape == (3, 32) and np.array_equal(q[1], vec[1])


def test_a_negative_zero_score_exists_and_the_oracle_search_reports_plus_zero(oracle):
    rows, query, want = RC.negative_zero_case()
    raw = oracle.cosine(query, rows)[0]
    assert _bits(raw)[[0, 3]].tolist() == [0x80000000, 0x80000000] and _bits(raw)[2] == 0     # the dot product itself is -0.0
    ids, sc = oracle.search(rows, query, 4)
    assert np.array_equal(ids[0], want)
    assert sc[0, 0] == raw[1] > 0.7 and _bits(sc[0, 1:]).tolist() == [0, 0, 0]
