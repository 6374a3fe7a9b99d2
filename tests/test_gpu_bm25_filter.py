"""A BM25 search restricted to a set of rows on the GPU (``BM25Retriever(...).search_columns(..., subset=)``: vf_bm25_search with
VF_BM25_FILTER, the k_bm25_*_f kernels of csrc/vf_sparse.hip) against numpy: ids and score BITS equal.

The reference is the numpy scorer over ALL rows (fp32 from 0, np.add.at of each query token's postings in query order: whole-corpus
statistics), restricted to the allowed rows, ``lexsort((rows, -score))`` -- score descending, ties to the lower row, the untouched
rows at score 0 in ascending order -- cut to k and padded with (-1, -FLT_MAX).

The index: 70 001 documents over 2000 tokens, mean length 8 -- three bitmap blocks of 32 768 rows, the last partial, and a last
bitmap word of 17 bits (70 001 = 2187 * 32 + 17)."""
import threading

import numpy as np
import pytest

import veritasfi_amd as vf
from veritasfi_amd import _ffi
from veritasfi_amd import bm25 as B
from test_ensemble_where import Emb, Store, SubsetCosineRetriever, _passes, _world

pytestmark = pytest.mark.gpu

N, VOCAB = 70001, 2000
PAD_SCORE = -np.finfo(np.float32).max
RARE = np.array([1999, 1998], np.int32)      # two rare tokens: fewer than 100 rows touched


def zipf_tokens(n_docs, vocab, mean_len, seed, a=1.25):
    rng = np.random.default_rng(seed)
    lens = rng.poisson(mean_len, size=n_docs)
    off = np.zeros(n_docs + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, (rng.zipf(a, size=int(off[-1])) - 1) % vocab


class Ref:
    """The numpy scorer over an index's arrays; the scores of a query are computed once and shared."""

    def __init__(self, indptr, indices, data, n):
        self.indptr, self.indices, self.data, self.n, self._sc = indptr, indices, data, n, {}

    def scores(self, cols):
        key = tuple(int(c) for c in cols)
        if key not in self._sc:
            sc = np.zeros(self.n, np.float32)
            for c in key:
                seg = slice(self.indptr[c], self.indptr[c + 1])
                np.add.at(sc, self.indices[seg], self.data[seg])
            sc.flags.writeable = False
            self._sc[key] = sc
        return self._sc[key]

    def topk(self, cols, mask, k):
        sc, rows = self.scores(cols), np.flatnonzero(mask)
        o = rows[np.lexsort((rows, -sc[rows]))][:k]
        ids, out = np.full(k, -1, np.int64), np.full(k, PAD_SCORE, np.float32)
        ids[:o.size], out[:o.size] = o, sc[o]
        return ids, out

    def check(self, cols, mask, k, ids, scores):
        want_ids, want_sc = self.topk(cols, mask, k)
        assert np.array_equal(np.asarray(ids, np.int64), want_ids)
        assert np.array_equal(np.asarray(scores, np.float32).view(np.uint32), want_sc.view(np.uint32))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("bm25_filter")
    off, toks = zipf_tokens(N, VOCAB, 8, seed=17)
    B.build_bm25_index_from_ids(off, toks, VOCAB, str(d))
    ix = B.load_bm25_index(str(d), load_corpus=False)
    assert ix.num_docs == N
    with vf.BM25Retriever(str(d), stemmer=None, load_corpus=False) as r:
        yield Ref(ix.indptr, ix.indices, ix.data, N), r


def _queries():
    rng = np.random.default_rng(5)
    return [rng.integers(0, VOCAB, size=6).astype(np.int32), np.array([3, 700, 3], np.int32), RARE]


def _mask(name, ref):
    rng = np.random.default_rng(23)
    m = np.zeros(N, bool)
    touched = ref.scores(_queries()[0]) > 0
    if name == "half":
        m = rng.random(N) < 0.5
    elif name == "one_percent":
        m = rng.random(N) < 0.01
    elif name == "row_0":
        m[0] = True
    elif name == "row_last":
        m[N - 1] = True
    elif name == "all":
        m[:] = True
    elif name == "touched":
        m = touched.copy()
    elif name == "untouched":
        m = ~touched
    return m


# every depth against the 50 % filter; each other filter at k = 1 and k = 100 at least ("m" = as many rows as the filter allows)
CASES = [("half", k) for k in (1, 100, 4096, 4097, "m")] + \
        [(f, k) for f in ("one_percent", "row_0", "row_last", "all", "touched", "untouched") for k in (1, 100)] + \
        [("one_percent", "m"), ("touched", "m"), ("untouched", 4097)]


@pytest.mark.parametrize("name, k", CASES, ids=[f"{f}-{k}" for f, k in CASES])
def test_ids_and_score_bits_match_numpy(world, name, k):
    ref, r = world
    mask = _mask(name, ref)
    k = int(mask.sum()) if k == "m" else k
    queries = _queries()
    assert 0 < int((ref.scores(RARE) > 0).sum()) < 100
    ids, scores = r.search_columns(queries, k, subset=mask)
    assert ids.shape == (len(queries), k) and scores.shape == ids.shape
    for i, cols in enumerate(queries):
        ref.check(cols, mask, k, ids[i], scores[i])
    ids2, scores2 = r.search_columns(queries, k, subset=np.flatnonzero(mask)[::-1])     # the same set as ids, unsorted
    assert np.array_equal(ids2, ids) and np.array_equal(scores2.view(np.uint32), scores.view(np.uint32))


def test_the_tail_comes_from_every_bitmap_block(world):
    ref, r = world
    touched = ref.scores(RARE) > 0
    assert 0 < int(touched.sum()) < 100
    dense = np.arange(N) >= 40000                                  # only rows >= 40 000: nothing of block 0 may be returned
    sparse = np.zeros(N, bool)                                     # ... and thinned, so that 100 rows reach from block 1 into block 2
    sparse[40000:65536:1000] = True
    sparse[65536::7] = True
    for mask in (dense, sparse):
        ids, scores = r.search_columns([RARE], 100, subset=mask)
        ref.check(RARE, mask, 100, ids[0], scores[0])
        tail = ids[0][scores[0] == 0.0]
        assert tail.size > 0 and tail.min() >= 40000 and np.all(np.diff(tail) > 0)
    assert (tail < 65536).any() and (tail >= 65536).any(), "the sparse filter's tail spans blocks 1 and 2"
    got_ids, got_sc = r.invoke_batch([""], 100, subset=sparse)[0]  # no token at all: the whole result is tail
    assert got_ids == np.flatnonzero(sparse)[:100].tolist() and not got_sc.any()


def test_fewer_rows_than_k_are_padded_on_both_paths(world):
    ref, r = world
    rng = np.random.default_rng(3)
    queries = _queries()
    for m, k in ((37, 100), (37, 4096), (100, 5000), (4500, 4600), (1, N)):
        mask = np.zeros(N, bool)
        mask[rng.choice(N, size=m, replace=False)] = True
        ids, scores = r.search_columns(queries, k, subset=mask)
        for i, cols in enumerate(queries):
            ref.check(cols, mask, k, ids[i], scores[i])
            assert (ids[i][m:] == -1).all() and (scores[i][m:] == PAD_SCORE).all() and (ids[i][:m] >= 0).all()
    for k in (1, 100, 5000):                                       # nothing allowed: all padding
        ids, scores = r.search_columns(queries, k, subset=[])
        assert (ids == -1).all() and (scores == PAD_SCORE).all()
    got_ids, got_sc = r.invoke_batch([""], 100, subset=[5, 70000, 9])[0]     # invoke trims to min(k, m)
    assert got_ids == [5, 9, 70000] and got_sc.tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("k", [100, 5000])
def test_a_filter_of_all_ones_is_the_unfiltered_call(world, k):
    _, r = world
    queries = _queries()
    want_ids, want_sc = r.search_columns(queries, k)
    ids, sc = r.search_columns(queries, k, subset=np.ones(N, bool))
    assert np.array_equal(ids, want_ids) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))


def test_the_scratch_is_clean_after_a_filtered_call(world):
    ref, r = world
    queries = _queries()
    rng = np.random.default_rng(9)
    for k in (100, 4097):
        before = r.search_columns(queries, k)
        for density in (0.5, 0.001):
            r.search_columns(queries, k, subset=rng.random(N) < density)
        after = r.search_columns(queries, k)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        for i, cols in enumerate(queries):
            ref.check(cols, np.ones(N, bool), k, after[0][i], after[1][i])


def test_a_batch_under_one_filter_equals_one_at_a_time_and_threads_interleave(world):
    ref, r = world
    rng = np.random.default_rng(11)
    queries = [rng.integers(0, VOCAB, size=int(rng.integers(0, 10))).astype(np.int32) for _ in range(70)]   # more than one group of 64 slots
    assert r.info()["slots"] < 70
    mask = rng.random(N) < 0.02
    ids, sc = r.search_columns(queries, 100, subset=mask)
    for i in range(0, 70, 9):
        one_ids, one_sc = r.search_columns([queries[i]], 100, subset=mask)
        assert np.array_equal(one_ids[0], ids[i]) and np.array_equal(one_sc[0].view(np.uint32), sc[i].view(np.uint32))
    for i in range(70):
        ref.check(queries[i], mask, 100, ids[i], sc[i])
    plain_ids, plain_sc = r.search_columns(queries[:8], 100)
    errors = []

    def work(filtered):
        try:
            for _ in range(6):
                if filtered:
                    got = r.search_columns(queries[:8], 100, subset=mask)
                    ok = np.array_equal(got[0], ids[:8]) and np.array_equal(got[1].view(np.uint32), sc[:8].view(np.uint32))
                else:
                    got = r.search_columns(queries[:8], 100)
                    ok = np.array_equal(got[0], plain_ids) and np.array_equal(got[1].view(np.uint32), plain_sc.view(np.uint32))
                if not ok:
                    errors.append(filtered)
        except Exception as e:      # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(f,)) for f in (True, False)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def _c_search(r, queries_off, terms, nq, k, allow_ptr, n_docs):
    ids, sc = np.zeros((max(nq, 1), k), np.int64), np.zeros((max(nq, 1), k), np.float32)
    fq = _ffi.Bm25FilterQuery(queries_off.ctypes.data_as(_ffi.p_i64), allow_ptr, n_docs)
    rc = _ffi.lib().vf_bm25_search(r._h, _ffi.ctypes.cast(_ffi.ctypes.byref(fq), _ffi.p_i64), terms.ctypes.data_as(_ffi.p_i32),
                                   nq | _ffi.VF_BM25_FILTER, k, ids.ctypes.data_as(_ffi.p_i64), sc.ctypes.data_as(_ffi.p_f32))
    return rc, ids, sc


def test_a_null_bitmap_and_a_bit_past_the_end_are_refused(world):
    ref, r = world
    u32p = _ffi.ctypes.POINTER(_ffi.ctypes.c_uint32)
    off, terms = np.array([0, 2], np.int64), RARE
    rc, _, _ = _c_search(r, off, terms, 1, 10, u32p(), N)
    assert rc == -1 and "null allow" in _ffi.last_error()
    words, _ = B.filter_words(np.ones(N, bool), N)
    assert words.size == 2188 and words[-1] == (1 << 17) - 1      # the last word holds rows 69 984 .. 70 000
    words[-1] |= np.uint32(0b11 << 18)                            # rows 70 002 and 70 003 do not exist
    rc, _, _ = _c_search(r, off, terms, 1, 10, words.ctypes.data_as(u32p), N)
    assert rc == -1 and "row 70002" in _ffi.last_error()
    rc, _, _ = _c_search(r, off, terms, 1, 10, words.ctypes.data_as(u32p), N - 1)
    assert rc == -1 and "70000 documents" in _ffi.last_error()
    words[-1] = (1 << 17) - 1
    rc, ids, sc = _c_search(r, off, terms, 1, 10, words.ctypes.data_as(u32p), N)     # the handle is unharmed
    assert rc == 0
    ref.check(RARE, np.ones(N, bool), 10, ids[0], sc[0])


def test_a_live_retriever_refuses_a_stale_filter_and_serves_a_new_one(tmp_path):
    n0, vocab = 33000, 500
    off, toks = zipf_tokens(n0, vocab, 6, seed=29)
    docs = np.split(toks, off[1:-1])
    B.build_bm25_index_from_ids(off, toks, vocab, str(tmp_path))
    rng = np.random.default_rng(31)
    queries = [np.array([7, 450, 7], np.int32), np.array([499, 498], np.int32)]
    u32p = _ffi.ctypes.POINTER(_ffi.ctypes.c_uint32)
    with vf.BM25Retriever(str(tmp_path), stemmer=None, load_corpus=False, live=True) as r:
        old_mask = rng.random(n0) < 0.1
        old_words, _ = B.filter_words(old_mask, n0)
        r.search_columns(queries, 100, subset=old_mask)
        add = [rng.integers(0, vocab, size=5) for _ in range(40)]
        gone = [0, 5, 17, 20000, 32999, 32998, 31]
        aoff = np.concatenate([[0], np.cumsum([a.size for a in add])])
        r.add_token_ids(aoff, np.concatenate(add))
        r.remove(gone)
        n1 = n0 + 40 - len(gone)
        assert r.num_docs == n1
        with pytest.raises(ValueError, match="one entry per row"):
            r.search_columns(queries, 100, subset=old_mask)                       # a mask of the old length
        qoff, terms = np.array([0, 3], np.int64), queries[0]
        rc, _, _ = _c_search(r, qoff, terms, 1, 10, old_words.ctypes.data_as(u32p), n0)   # the C call with the old count
        assert rc == -1 and "may have changed" in _ffi.last_error()
        kept = [d for i, d in enumerate(docs) if i not in set(gone)] + add
        koff = np.concatenate([[0], np.cumsum([d.size for d in kept])]).astype(np.int64)
        indptr, indices, data = B.bm25_index_arrays(koff, np.concatenate(kept), vocab)
        ref = Ref(indptr, indices, data, n1)
        for density, k in ((0.1, 100), (0.001, 100), (0.3, 4097)):
            mask = rng.random(n1) < density
            mask[n1 - 1] = True
            ids, sc = r.search_columns(queries, k, subset=mask)
            for i, cols in enumerate(queries):
                ref.check(cols, mask, k, ids[i], sc[i])
        ids, sc = r.search_columns(queries, 100)                                  # and the handle is unharmed
        for i, cols in enumerate(queries):
            ref.check(cols, np.ones(n1, bool), 100, ids[i], sc[i])


class _HidesTheFilter:
    """The retriever as the ensemble saw it before it could filter: ``invoke(query, k)`` alone."""
    exact_prefix = True

    def __init__(self, r):
        self.r, self.asked = r, []

    def invoke(self, query, k):
        self.asked.append(k)
        return self.r.invoke(query, k)


@pytest.mark.parametrize("min_score", [None, "median"])
def test_the_ensemble_returns_what_the_full_ranking_filtered_on_the_host_returned(tmp_path, min_score):
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, _, _, _, _ = _world(6)
    n, vocab = len(metas), 40
    off, toks = zipf_tokens(n, vocab, 6, seed=37)
    B.build_bm25_index_from_ids(off, toks, vocab, str(tmp_path))
    rng = np.random.default_rng(41)
    texts = ["t3 t17 t3", "t39 t38", "t0 t1 t2 t25"]
    emb = Emb({t: (base[a] + 0.05 * rng.standard_normal(base.shape[1]).astype(np.float32)).tolist() for t, a in zip(texts, (3, 100, 199))})
    ts = Store(titles, [None] * len(titles), t_emb.tolist())
    with vf.BM25Retriever(str(tmp_path), stemmer=None, load_corpus=False) as r:
        if min_score == "median":                                 # a threshold that cuts the ranking of a query somewhere in the middle
            sc = r.invoke(texts[1], n)[1]
            r.min_score = float(np.median(sc[sc > 0]))
        hidden = _HidesTheFilter(r)
        new, old = (EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=bm, retriever_cls=SubsetCosineRetriever,
                                      faiss_ts_k=2, bm25_k=9) for bm in (r, hidden))
        emitted = 0
        for where in ({"company": "zeekr"}, {"company": ["zeekr", "lotus"], "year": 2023}):
            keep = [i for i, md in enumerate(metas) if _passes(md, where)]
            assert 0 < len(keep) < n
            for t in texts:
                hidden.asked.clear()
                got, want = new.invoke(t, [], where=where), old.invoke(t, [], where=where)
                assert hidden.asked == [n], "the wrapped retriever took the parent commit's path: the full ranking"
                assert got == want
                emitted += sum(1 for c in got if c["retriever"] == "BM25")
        assert emitted > 0
