"""A prepared BM25 row filter PER QUERY of a batch on the GPU (``search_columns(..., subsets=[...])``; vf_bm25_search with
VF_BM25_PREPARED, phase VF_BM25_PREPARED_SEARCH and mode VF_BM25_PREPARED_PER_QUERY; the kernels k_bm25_accum_m, k_bm25_tail_count_m,
k_bm25_tail_write_m and k_bm25_pad_out_m of csrc/vf_sparse.hip).  The rule: row i of the batch is, ids equal and score BITS equal, what
the existing one-filter prepared call returns for query i ALONE with filter i on the same retriever -- the plain call where the entry is
None -- and, for a subset-mode entry, what a fresh retriever over the allowed documents alone returns, rows mapped back.

The worlds of tests/test_gpu_bm25_prepared.py: S, 12 rows over 16 columns; C, 32 768 + 40 rows over 4096 columns (two bitmap blocks); B,
5000 documents for k = 4500 (the k > 4096 arm, one query at a time).  Mixed groups (corpus mode, subset mode, no filter, a filter of no
row, of three rows, the same object twice, an empty query), 70 queries over two groups, tails and padding across the block boundary,
the sequence with unprepared calls between, staleness, the C ABI's refusals and the Python layer's."""
import numpy as np
import pytest

import veritasfi_amd as vf
from veritasfi_amd import _ffi
from veritasfi_amd import bm25 as B
from test_gpu_bm25_prepared import PAD_SCORE, SHAPES, U32P, World, _fresh_over_allowed, _masks, _queries, same

pytestmark = pytest.mark.gpu

U64P = _ffi.ctypes.POINTER(_ffi.ctypes.c_uint64)


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    out = {name: World(name, tmp_path_factory.mktemp("bm25_multi_" + name)) for name in SHAPES}
    yield out
    for w in out.values():
        w.close()


def _alone(r, queries, k, subsets):
    """the reference: one call per query, the one-filter prepared call or the plain one"""
    ids, sc = np.empty((len(queries), k), np.int64), np.empty((len(queries), k), np.float32)
    for i, (q, s) in enumerate(zip(queries, subsets)):
        one = r.search_columns([q], k) if s is None else r.search_columns([q], k, subset=s)
        ids[i], sc[i] = one[0][0], one[1][0]
    return ids, sc


def _check_padding(got, subsets, k):
    for i, s in enumerate(subsets):
        m = k if s is None else min(s.m, k)
        assert (got[0][i, :m] >= 0).all() and (got[0][i, m:] == -1).all() and (got[1][i, m:] == PAD_SCORE).all(), i


def test_s_a_mixed_group_is_each_query_alone_with_its_own_filter(worlds, tmp_path):
    w = worlds["S"]
    r, k = w.live, 5
    masks = _masks("S", w)
    big, three = masks["without_the_commonest_token"], masks["rows_0_5_11"]
    q = _queries(w, big, 3)
    assert q[0][0] == q[0][2] and q[2].size == 0 and int(big.sum()) >= k
    with r.prepare_subset(big) as big_c, r.prepare_subset(big, stats="subset") as big_s, r.prepare_subset(three) as three_c, \
            r.prepare_subset(three, stats="subset") as three_s, r.prepare_subset([], stats="subset") as none_s, r.prepare_subset([]) as none_c:
        batch = [(q[0], big_c, big), (q[0], big_s, big), (q[1], None, None), (q[0], none_s, None), (q[0], three_c, three), (q[1], three_s, three),
                 (q[0], big_c, big), (q[2], big_s, big), (q[2], None, None), (q[1], big_s, big), (q[1], none_c, None), (q[2], three_s, three)]
        queries, subsets = [b[0] for b in batch], [b[1] for b in batch]
        got = r.search_columns(queries, k, subsets=subsets)
        assert got[0].shape == (len(batch), k) and same(got, _alone(r, queries, k, subsets))
        _check_padding(got, subsets, k)
        assert (got[0][3] == -1).all() and (got[0][4, 3:] == -1).all() and (got[0][4, :3] >= 0).all() and (got[0][2] >= 0).all()
        for i, (qi, s, mask) in enumerate(batch):            # a subset-mode row is the fresh retriever's over the allowed documents alone
            if s is not None and s.stats == "subset" and mask is not None:
                want = _fresh_over_allowed(w, mask, tmp_path, [qi], k)
                assert np.array_equal(got[0][i], want[0][0]) and np.array_equal(got[1][i].view(np.uint32), want[1][0].view(np.uint32)), i
        for kk in (1, 3, 4, w.n):                            # k below, at and above the three-row filter; k = n
            assert same(r.search_columns(queries, kk, subsets=subsets), _alone(r, queries, kk, subsets)), kk
        assert same(r.search_columns(queries, k, subsets=[None] * len(queries)), r.search_columns(queries, k))      # all None: the plain call
        res = r.invoke_batch(["t0 t1 t0", "t1 t2", ""], 5, subsets=[three_s, None, none_c])
        assert [len(ids) for ids, _ in res] == [3, 5, 0] and [len(sc) for _, sc in res] == [3, 5, 0]
        assert res[0][0] == r.invoke("t0 t1 t0", 5, subset=three_s)[0] and res[1][0] == r.invoke("t1 t2", 5)[0]
    f = w.frozen                                             # corpus-mode filters on a handle that is not live
    with f.prepare_subset(big) as fb, f.prepare_subset(three) as ft:
        subsets = [fb, None, ft, fb]
        queries = [q[0], q[1], q[0], q[2]]
        assert same(f.search_columns(queries, k, subsets=subsets), _alone(f, queries, k, subsets))


def test_s_70_queries_are_two_groups_and_a_slot_serves_two_filters(worlds):
    w = worlds["S"]
    r, k = w.live, 5
    assert r.info()["slots"] == 64
    masks = _masks("S", w)
    queries = _queries(w, masks["without_the_commonest_token"], 70)
    with r.prepare_subset(masks["without_the_commonest_token"]) as a, r.prepare_subset(masks["rows_0_5_11"], stats="subset") as b, \
            r.prepare_subset(masks["all"], stats="subset") as c, r.prepare_subset(np.arange(w.n) % 2 == 1) as d:
        cycle = [a, b, None, c, d]
        subsets = [cycle[i % 5] for i in range(70)]
        assert subsets[0] is not subsets[64]                 # slot 0 serves query 0 and query 64 under different filters
        got = r.search_columns(queries, k, subsets=subsets)
        assert same(got, _alone(r, queries, k, subsets))
        _check_padding(got, subsets, k)
        same_filter = r.search_columns(queries, k, subsets=[b] * 70)      # every token equal: still this path, and the one-filter batch's result
        assert same(same_filter, r.search_columns(queries, k, subset=b))


def test_c_tails_and_padding_across_the_block_boundary(worlds):
    w = worlds["C"]
    r, k = w.live, 100
    masks = _masks("C", w)
    queries = _queries(w, masks["every_other"], 8)
    assert queries[2].size == 0
    with r.prepare_subset(masks["rows_32767_32768"]) as two_c, r.prepare_subset(masks["rows_32767_32768"], stats="subset") as two_s, \
            r.prepare_subset(masks["second_block"]) as blk_c, r.prepare_subset(masks["second_block"], stats="subset") as blk_s, \
            r.prepare_subset(masks["every_other"]) as eo, r.prepare_subset(masks["one_percent"], stats="subset") as pc:
        # query 2 is empty: under "second_block" all its rows are allowed untouched rows of block 1
        subsets = [two_c, blk_s, blk_c, eo, None, pc, two_s, None]
        got = r.search_columns(queries, k, subsets=subsets)
        assert same(got, _alone(r, queries, k, subsets))
        _check_padding(got, subsets, k)
        assert got[0][2].tolist() == list(range(32768, 32768 + 40)) + [-1] * 60 and (got[1][2, :40] == 0).all()
        assert sorted(got[0][0, :2].tolist()) == [32767, 32768] and sorted(got[0][6, :2].tolist()) == [32767, 32768]
    f = w.frozen
    with f.prepare_subset(masks["second_block"]) as blk, f.prepare_subset(masks["one_percent"]) as pc:
        subsets = [blk, None, blk, pc, None, pc, None, blk]
        assert same(f.search_columns(queries, k, subsets=subsets), _alone(f, queries, k, subsets))


def test_b_k_4500_the_deep_k_arm_one_query_at_a_time(worlds):
    w = worlds["B"]
    r, k = w.live, 4500
    rng = np.random.default_rng(4)
    few, many = np.sort(rng.choice(w.n, size=4400, replace=False)), np.sort(rng.choice(w.n, size=4600, replace=False))
    mask = np.zeros(w.n, bool)
    mask[few] = True
    queries = _queries(w, mask, 3)
    with r.prepare_subset(few, stats="subset") as few_s, r.prepare_subset(many) as many_c:
        subsets = [few_s, many_c, None]
        got = r.search_columns(queries, k, subsets=subsets)
        assert same(got, _alone(r, queries, k, subsets))
        _check_padding(got, subsets, k)
        assert (got[0][0, 4400:] == -1).all() and (got[0][1] >= 0).all() and (got[0][2] >= 0).all()


def test_unprepared_calls_between_do_not_disturb_it_and_an_update_makes_its_entries_stale(worlds):
    w = worlds["S"]
    k = 5
    with vf.BM25Retriever(w.dir, stemmer=None, load_corpus=False, live=True) as r:
        masks = _masks("S", w)
        other = np.arange(w.n) % 3 == 0
        queries = _queries(w, masks["rows_0_5_11"], 5)
        a, b = r.prepare_subset(masks["without_the_commonest_token"]), r.prepare_subset(masks["rows_0_5_11"], stats="subset")
        subsets = [a, b, None, b, a]
        first = r.search_columns(queries, k, subsets=subsets)
        assert same(first, _alone(r, queries, k, subsets))
        un_c = r.search_columns(queries, k, subset=other)                   # the handle's own bitmap now holds `other` ...
        un_s = r.search_columns(queries, k, subset=other, stats="subset")   # ... and a stage has left its copy there
        assert same(r.search_columns(queries, k, subsets=subsets), first)
        assert same(r.search_columns(queries, k, subset=other), un_c) and same(r.search_columns(queries, k, subset=other, stats="subset"), un_s)
        tokens = np.array([a._token, b._token], np.uint64)
        r.add_texts(["t3 t9 t9 t1"])
        assert a.stale and b.stale
        with pytest.raises(ValueError, match=r"subsets\[1\].*stale.*prepare_subset again"):
            r.search_columns(queries, k, subsets=[None, b, None, None, None])
        rc, ids, _ = _c_multi(r, tokens, [np.array([0], np.int32)] * 2, k)  # the retriever has released its stale filters: the library knows them no more
        assert rc == -1 and f"tokens[0] = {a._token}" in _ffi.last_error() and "unknown or released" in _ffi.last_error() and (ids == 7).all()
        grown = [np.append(m, False) for m in (masks["without_the_commonest_token"], masks["rows_0_5_11"])]
        with r.prepare_subset(grown[0]) as a2, r.prepare_subset(grown[1], stats="subset") as b2:
            subsets = [a2, b2, None, b2, a2]
            assert same(r.search_columns(queries, k, subsets=subsets), _alone(r, queries, k, subsets))


def _c_multi(r, tokens, queries, k, flags=0, null_tokens=False, mode=None):
    cols, off, terms = B.BM25Retriever._columns_args(queries)
    nq = len(cols)
    ids, sc = np.full((nq, k), 7, np.int64), np.full((nq, k), 7.0, np.float32)
    pq = _ffi.Bm25PreparedQuery()
    pq.q_offsets, pq.phase = off.ctypes.data_as(_ffi.p_i64), _ffi.VF_BM25_PREPARED_SEARCH
    pq.mode = _ffi.VF_BM25_PREPARED_PER_QUERY if mode is None else mode
    tokens = np.ascontiguousarray(tokens, np.uint64)
    if not null_tokens:
        pq.tokens = tokens.ctypes.data_as(U64P)
    rc = _ffi.lib().vf_bm25_search(r._h, _ffi.ctypes.cast(_ffi.ctypes.byref(pq), _ffi.p_i64), terms.ctypes.data_as(_ffi.p_i32), nq | _ffi.VF_BM25_PREPARED | flags,
                                   k, ids.ctypes.data_as(_ffi.p_i64), sc.ctypes.data_as(_ffi.p_f32))
    return rc, ids, sc


def test_the_c_abi_refuses_by_position_and_the_next_call_is_right(worlds):
    w = worlds["S"]
    n, V, k = w.n, w.vocab, 5
    assert _ffi.VF_BM25_PREPARED_PER_QUERY == 2 and _ffi.lib().vf_version() == 100
    mask = np.arange(n) % 2 == 0
    words, _ = B.filter_words(mask, n)
    queries = _queries(w, mask, 5)
    with vf.BM25Retriever(w.dir, stemmer=None, load_corpus=False, live=True) as r, r.prepare_subset(mask) as c, r.prepare_subset(mask, stats="subset") as s:
        subsets = [c, s, None, s, c]
        good = np.array([c._token, s._token, 0, s._token, c._token], np.uint64)
        want = _alone(r, queries, k, subsets)

        def next_call_is_right():
            rc, ids, sc = _c_multi(r, good, queries, k)
            assert rc == 0 and same((ids, sc), want)

        next_call_is_right()
        rc, ids, sc = _c_multi(r, good, queries, k, null_tokens=True)
        assert rc == -1 and "null tokens" in _ffi.last_error() and (ids == 7).all() and (sc == 7.0).all()
        next_call_is_right()
        bad = good.copy()
        bad[3] = 12345
        rc, ids, _ = _c_multi(r, bad, queries, k)
        assert rc == -1 and "tokens[3] = 12345" in _ffi.last_error() and "unknown or released" in _ffi.last_error() and (ids == 7).all()
        next_call_is_right()
        df = np.zeros(V, np.int64)                           # a subset-mode filter prepared through the ABI and never armed
        pq = _ffi.Bm25PreparedQuery()
        pq.allow, pq.n_docs, pq.phase, pq.mode = words.ctypes.data_as(U32P), n, _ffi.VF_BM25_PREPARED_PREPARE, _ffi.VF_BM25_PREPARED_SUBSET
        pq.vocab, pq.df = V, df.ctypes.data_as(_ffi.p_i64)
        assert _ffi.lib().vf_bm25_search(r._h, _ffi.ctypes.cast(_ffi.ctypes.byref(pq), _ffi.p_i64), None, _ffi.VF_BM25_PREPARED, 1, None, None) == 0
        unarmed = good.copy()
        unarmed[1] = pq.token
        rc, ids, _ = _c_multi(r, unarmed, queries, k)
        assert rc == -1 and f"tokens[1] = {pq.token}" in _ffi.last_error() and "never armed" in _ffi.last_error() and (ids == 7).all()
        next_call_is_right()
        rc, ids, _ = _c_multi(r, good, queries, k, flags=_ffi.VF_BM25_FILTER)
        assert rc == -1 and "goes alone" in _ffi.last_error() and (ids == 7).all()
        next_call_is_right()
        # a search whose mode is not VF_BM25_PREPARED_PER_QUERY reads `token` and never `tokens`, as before
        for mode in (_ffi.VF_BM25_PREPARED_CORPUS, _ffi.VF_BM25_PREPARED_SUBSET):
            rc, _, _ = _c_multi(r, good, queries, k, null_tokens=True, mode=mode)
            assert rc == -1 and "token 0 names no prepared filter" in _ffi.last_error()
        pq.phase = _ffi.VF_BM25_PREPARED_RELEASE
        assert _ffi.lib().vf_bm25_search(r._h, _ffi.ctypes.cast(_ffi.ctypes.byref(pq), _ffi.p_i64), None, _ffi.VF_BM25_PREPARED, 1, None, None) == 0
        rc, _, _ = _c_multi(r, unarmed, queries, k)
        assert rc == -1 and "tokens[1]" in _ffi.last_error() and "unknown or released" in _ffi.last_error()
        next_call_is_right()
        # a filter the library still knows, made before the handle's last update: refused by its generation, with the one-token call's message
        pq.phase, pq.mode = _ffi.VF_BM25_PREPARED_PREPARE, _ffi.VF_BM25_PREPARED_CORPUS
        assert _ffi.lib().vf_bm25_search(r._h, _ffi.ctypes.cast(_ffi.ctypes.byref(pq), _ffi.p_i64), None, _ffi.VF_BM25_PREPARED, 1, None, None) == 0
        r.add_token_ids(np.array([0, 4]), np.array([3, 9, 9, 1]), remove_ids=[5])      # n_docs stays: only the generation tells
        rc, ids, _ = _c_multi(r, np.array([0, pq.token], np.uint64), queries[:2], k)
        assert rc == -1 and f"tokens[1] = {pq.token}" in _ffi.last_error() and f"generation {pq.generation}" in _ffi.last_error() \
            and "prepare the filter again" in _ffi.last_error() and (ids == 7).all()
        with r.prepare_subset(mask) as c2:
            rc, ids, sc = _c_multi(r, np.array([0, c2._token], np.uint64), queries[:2], k)
            assert rc == 0 and same((ids, sc), _alone(r, queries[:2], k, [None, c2]))


def test_refusals_of_the_python_layer(worlds):
    w = worlds["S"]
    r = w.live
    mask = np.arange(w.n) % 2 == 0
    q = _queries(w, mask, 3)
    with r.prepare_subset(mask) as c, w.frozen.prepare_subset(mask) as foreign:
        with pytest.raises(ValueError, match="subset= and subsets="):
            r.search_columns(q, 3, subset=mask, subsets=[c, None, c])
        with pytest.raises(ValueError, match="stats="):
            r.search_columns(q, 3, stats="corpus", subsets=[c, None, c])
        with pytest.raises(ValueError, match="2 entries for 3 queries"):
            r.search_columns(q, 3, subsets=[c, None])
        with pytest.raises(ValueError, match=r"subsets\[2\].*another BM25Retriever"):
            r.invoke_batch(["t1", "t2", "t3"], 3, subsets=[c, None, foreign])
        with pytest.raises(TypeError, match=r"subsets\[1\]"):
            r.search_columns(q, 3, subsets=[c, mask, None])
        with pytest.raises(ValueError, match="k=13"):
            r.search_columns(q, w.n + 1, subsets=[c, None, c])
        assert same(r.search_columns(q, 3, subsets=[c, None, c]), _alone(r, q, 3, [c, None, c]))
    assert c.closed
    with pytest.raises(ValueError, match=r"subsets\[2\].*closed.*prepare_subset again"):
        r.search_columns(q, 3, subsets=[None, None, c])
    assert same(r.search_columns(q, 3, subsets=[None, None, None]), r.search_columns(q, 3))
