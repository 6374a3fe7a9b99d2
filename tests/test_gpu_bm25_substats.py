"""A filtered BM25 search scored by the SUBSET's own statistics on the GPU (``BM25Retriever(dir, live=True).search_columns(...,
subset=, stats="subset")``: vf_bm25_search with VF_BM25_FILTER | VF_BM25_SUBSTATS, the kernels k_bm25_sub_len, k_bm25_sub_df and
k_bm25_accum_s of csrc/vf_sparse.hip) against the host: ids equal and score BITS equal, everywhere.

The expectation: ``bm25_index_arrays`` over the allowed documents ALONE (ascending rows, the same vocabulary size), its postings
scored by numpy (fp32 from 0, np.add.at per query token in query order), the canonical ranking (score descending, ties to the lower
row, untouched rows at 0 ascending), cut to k, padded with (-1, -FLT_MAX), its row i mapped back to the i-th allowed row -- and, for
the small cases, a plain ``BM25Retriever`` over ``build_bm25_index_from_ids`` of those documents.

Indexes: Zipf token ids over 64 tokens, mean length 4, every 23rd document empty.  A: 300 documents.  B: 5000 (k > 4096).  C: 32 768 + 40
(a second bitmap block)."""
import numpy as np
import pytest

import veritasfi_amd as vf
from veritasfi_amd import _ffi
from veritasfi_amd import bm25 as B
from test_ensemble_where import Emb, Store, SubsetCosineRetriever, _passes, _world
from test_gpu_bm25_filter import PAD_SCORE, Ref, _HidesTheFilter

pytestmark = pytest.mark.gpu

VOCAB = 64
SIZES = {"A": 300, "B": 5000, "C": 32768 + 40}
U32P = _ffi.ctypes.POINTER(_ffi.ctypes.c_uint32)
F64P = _ffi.ctypes.POINTER(_ffi.ctypes.c_double)


def make_docs(n, seed, vocab=VOCAB, mean_len=4):
    rng = np.random.default_rng(seed)
    lens = rng.poisson(mean_len, size=n)
    lens[11::23] = 0
    toks = (rng.zipf(1.25, size=int(lens.sum())) - 1) % vocab
    return np.split(toks, np.cumsum(lens)[:-1])


def flat(docs):
    off = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([d.size for d in docs], out=off[1:])
    return off, (np.concatenate(docs) if len(docs) else np.zeros(0, np.int64))


class SubsetRef:
    """The index of the allowed documents alone, and its numpy ranking with rows mapped back."""

    def __init__(self, docs, rows, vocab=VOCAB):
        self.rows = np.asarray(rows, np.int64)
        off, toks = flat([docs[r] for r in self.rows])
        self.off, self.toks, self.vocab = off, toks, vocab
        if self.rows.size:
            indptr, indices, data = B.bm25_index_arrays(off, toks, vocab)
            self.ref = Ref(indptr, indices, data, self.rows.size)

    def topk(self, cols, k):
        if not self.rows.size:
            return np.full(k, -1, np.int64), np.full(k, PAD_SCORE, np.float32)
        ids, sc = self.ref.topk(cols, np.ones(self.rows.size, bool), k)
        return np.where(ids >= 0, self.rows[np.maximum(ids, 0)], -1), sc

    def check(self, cols, k, ids, scores):
        want_ids, want_sc = self.topk(cols, k)
        assert np.array_equal(np.asarray(ids, np.int64), want_ids)
        assert np.array_equal(np.asarray(scores, np.float32).view(np.uint32), want_sc.view(np.uint32))


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    out, open_ = {}, []
    for name, n in SIZES.items():
        d = tmp_path_factory.mktemp("bm25_substats_" + name)
        docs = make_docs(n, seed=40 + len(out))
        off, toks = flat(docs)
        B.build_bm25_index_from_ids(off, toks, VOCAB, str(d))
        r = vf.BM25Retriever(str(d), stemmer=None, load_corpus=False, live=True)
        open_.append(r)
        out[name] = (docs, r, str(d))
    yield out
    for r in open_:
        r.close()


QUERIES = [np.array([0, 5, 17, 40, 2], np.int32), np.array([3, 9, 3], np.int32), np.zeros(0, np.int32), np.array([63, 58], np.int32)]


def _has(docs, token):
    """bool [n]: the documents that hold the token"""
    off, toks = flat(docs)
    out = np.zeros(len(docs), bool)
    out[np.repeat(np.arange(len(docs)), np.diff(off))[toks == token]] = True
    return out


def _filter_a(name, docs):
    n = len(docs)
    m = np.zeros(n, bool)
    if name == "one_row":
        m[137] = True
    elif name == "rows_31_32_33":
        m[[31, 32, 33]] = True
    elif name == "every_other":
        m[::2] = True
    elif name == "run":
        m[100:181] = True
    elif name == "all":
        m[:] = True
    elif name == "token_17_has_no_allowed_posting":
        m = ~_has(docs, 17)
    elif name == "empty_documents":
        m = np.array([d.size == 0 for d in docs])
    return m


FILTERS_A = ("one_row", "rows_31_32_33", "every_other", "run", "all", "token_17_has_no_allowed_posting", "empty_documents")
_refs = {}


def _ref_a(name, docs):
    if name not in _refs:
        _refs[name] = SubsetRef(docs, np.flatnonzero(_filter_a(name, docs)))
    return _refs[name]


@pytest.mark.parametrize("k", [10, "m"])
@pytest.mark.parametrize("name", FILTERS_A)
def test_a_ids_and_score_bits_are_those_of_the_subsets_own_index(worlds, tmp_path, name, k):
    docs, r, _ = worlds["A"]
    mask, ref = _filter_a(name, docs), _ref_a(name, docs)
    m = int(mask.sum())
    assert m > 0
    k = m if k == "m" else k
    if name == "token_17_has_no_allowed_posting":
        assert _has(docs, 17).any() and m > 10
    if name == "empty_documents":
        assert ref.toks.size == 0
    ids, sc = r.search_columns(QUERIES, k, subset=mask, stats="subset")
    assert ids.shape == (len(QUERIES), k)
    for i, cols in enumerate(QUERIES):
        ref.check(cols, k, ids[i], sc[i])
        assert (ids[i][:min(k, m)] >= 0).all() and (ids[i][m:] == -1).all() and (sc[i][m:] == PAD_SCORE).all()
    if name == "empty_documents":
        assert not sc[:, :min(k, m)].any()
    # ... and a plain retriever over a directory built from those documents alone, rows mapped back
    B.build_bm25_index_from_ids(ref.off, ref.toks, VOCAB, str(tmp_path))
    with vf.BM25Retriever(str(tmp_path), stemmer=None, load_corpus=False) as small:
        kk = min(k, m)
        s_ids, s_sc = small.search_columns(QUERIES, kk)
        assert np.array_equal(ref.rows[s_ids], ids[:, :kk]) and np.array_equal(s_sc.view(np.uint32), sc[:, :kk].view(np.uint32))
    got = r.invoke_batch(["t3 t9 t3", ""], k, subset=np.flatnonzero(mask), stats="subset")   # invoke trims the padding
    assert [len(g[0]) for g in got] == [min(k, m)] * 2 and got[0][0] == ids[1][:min(k, m)].tolist()


def test_the_mode_differs_from_the_corpus_mode(worlds):
    docs, r, _ = worlds["A"]
    mask = _filter_a("every_other", docs)
    a = r.search_columns(QUERIES[:1], 10, subset=mask, stats="subset")
    b = r.search_columns(QUERIES[:1], 10, subset=mask)
    assert not np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "idf and avgdl of half the corpus are not the corpus's"


@pytest.mark.parametrize("name, k", [("A", 100), ("A", 300), ("C", 100), ("C", 5000)])
def test_all_rows_allowed_is_the_unfiltered_call(worlds, name, k):
    docs, r, _ = worlds[name]
    want_ids, want_sc = r.search_columns(QUERIES, k)
    ids, sc = r.search_columns(QUERIES, k, subset=np.ones(len(docs), bool), stats="subset")
    assert np.array_equal(ids, want_ids) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))


@pytest.mark.parametrize("m", [4500, 5000])
def test_b_beyond_4096_ranks_and_its_padding(worlds, m):
    docs, r, _ = worlds["B"]
    rows = np.sort(np.random.default_rng(m).choice(len(docs), size=m, replace=False))
    ref = SubsetRef(docs, rows)
    for k in (5000, 4096):      # the global sort and the LDS sort, both padded when m = 4500 ... or not
        ids, sc = r.search_columns(QUERIES, k, subset=rows, stats="subset")
        for i, cols in enumerate(QUERIES):
            ref.check(cols, k, ids[i], sc[i])
            assert (ids[i][m:] == -1).all() and (ids[i][:min(k, m)] >= 0).all()


@pytest.mark.parametrize("which", ["second_block", "rows_32767_32768", "last_rows_of_block_0_and_first_of_block_1"])
def test_c_the_second_bitmap_block(worlds, which):
    docs, r, _ = worlds["C"]
    n = len(docs)
    rows = {"second_block": np.arange(32768, n), "rows_32767_32768": np.array([32767, 32768]),
            "last_rows_of_block_0_and_first_of_block_1": np.arange(32700, 32800)}[which]
    ref = SubsetRef(docs, rows)
    m, total, df = r.subset_statistics(rows, QUERIES)
    assert (m, total) == (rows.size, sum(docs[i].size for i in rows))
    for k in (10, 40, 100):
        ids, sc = r.search_columns(QUERIES, k, subset=rows, stats="subset")
        for i, cols in enumerate(QUERIES):
            ref.check(cols, k, ids[i], sc[i])
    tail = r.search_columns([QUERIES[2]], 40, subset=rows, stats="subset")[0][0]      # no token: the tail alone, from block 1 too
    assert tail[:min(40, m)].tolist() == rows[:40].tolist()


@pytest.mark.parametrize("name", ["A", "C"])
def test_subset_statistics_returns_numpys_counts(worlds, name):
    docs, r, _ = worlds[name]
    n = len(docs)
    rng = np.random.default_rng(7)
    queries = QUERIES + [rng.integers(0, VOCAB, size=12).astype(np.int32)]
    has = {int(c): _has(docs, int(c)) for q in queries for c in q}
    dl = np.array([d.size for d in docs])
    masks = [rng.random(n) < 0.5, rng.random(n) < 0.01, np.ones(n, bool), np.arange(n) >= n - 40, np.arange(n) == 31]
    for mask in masks:
        m, total, df = r.subset_statistics(mask, queries)
        assert (m, total) == (int(mask.sum()), int(dl[mask].sum()))
        assert len(df) == len(queries)
        for q, d in zip(queries, df):
            assert d.dtype == np.int64 and d.tolist() == [int((has[int(c)] & mask).sum()) for c in q]
    assert r.subset_statistics([], queries)[:2] == (0, 0)
    assert r.subset_statistics(masks[0], [])[2] == []


def test_a_batch_of_70_under_one_filter_equals_one_at_a_time(worlds):
    docs, r, _ = worlds["A"]
    rng = np.random.default_rng(11)
    queries = [rng.integers(0, VOCAB, size=int(rng.integers(0, 8))).astype(np.int32) for _ in range(70)]
    assert r.info()["slots"] < 70
    mask = _filter_a("every_other", docs)
    ref = _ref_a("every_other", docs)
    ids, sc = r.search_columns(queries, 20, subset=mask, stats="subset")
    for i in range(70):
        ref.check(queries[i], 20, ids[i], sc[i])
    for i in range(0, 70, 9):
        one_ids, one_sc = r.search_columns([queries[i]], 20, subset=mask, stats="subset")
        assert np.array_equal(one_ids[0], ids[i]) and np.array_equal(one_sc[0].view(np.uint32), sc[i].view(np.uint32))


def _own_live(worlds, tmp_path):
    docs, _, _ = worlds["A"]
    off, toks = flat(docs)
    B.build_bm25_index_from_ids(off, toks, VOCAB, str(tmp_path))
    return docs, vf.BM25Retriever(str(tmp_path), stemmer=None, load_corpus=False, live=True)


def test_after_live_updates_the_subset_is_that_of_the_new_corpus(worlds, tmp_path):
    docs, r = _own_live(worlds, tmp_path)
    rng = np.random.default_rng(13)
    with r:
        gone = rng.choice(len(docs), size=20, replace=False)
        add = make_docs(30, seed=99)
        aoff, atoks = flat(add)
        r.add_token_ids(aoff, atoks, remove_ids=gone)
        kept = [d for i, d in enumerate(docs) if i not in set(gone.tolist())] + add
        assert r.num_docs == len(kept) == 310
        for mask in (rng.random(310) < 0.4, np.arange(310) >= 270, np.ones(310, bool)):
            ref = SubsetRef(kept, np.flatnonzero(mask))
            for k in (10, int(mask.sum())):
                ids, sc = r.search_columns(QUERIES, k, subset=mask, stats="subset")
                for i, cols in enumerate(QUERIES):
                    ref.check(cols, k, ids[i], sc[i])


def _c_call(r, phase, off, terms, words, n_docs, k, df=None, idf=None, generation=0, avgdl=1.0, k1=1.5, b=0.75):
    nq = off.size - 1
    ids, sc = np.full((nq, k), 7, np.int64), np.full((nq, k), 7.0, np.float32)
    sq = _ffi.Bm25SubstatsQuery(off.ctypes.data_as(_ffi.p_i64), words.ctypes.data_as(U32P), n_docs)
    sq.phase, sq.generation, sq.avgdl, sq.k1, sq.b = phase, generation, avgdl, k1, b
    if df is not None:
        sq.df = df.ctypes.data_as(_ffi.p_i64)
    if idf is not None:
        sq.idf = idf.ctypes.data_as(F64P)
    rc = _ffi.lib().vf_bm25_search(r._h, _ffi.ctypes.cast(_ffi.ctypes.byref(sq), _ffi.p_i64), terms.ctypes.data_as(_ffi.p_i32),
                                   nq | _ffi.VF_BM25_FILTER | _ffi.VF_BM25_SUBSTATS, k, ids.ctypes.data_as(_ffi.p_i64), sc.ctypes.data_as(_ffi.p_f32))
    return rc, sq, ids, sc


def _idf(sq, df):
    d = df.astype(np.float64)
    return np.ascontiguousarray(np.log(1.0 + (sq.m - d + 0.5) / (d + 0.5)))


def test_a_stale_generation_is_refused_and_changes_nothing(worlds, tmp_path):
    docs, r = _own_live(worlds, tmp_path)
    with r:
        n = len(docs)
        mask = _filter_a("every_other", docs)
        words, _ = B.filter_words(mask, n)
        off, terms = np.array([0, 3], np.int64), QUERIES[1]
        df = np.zeros(3, np.int64)
        rc, sq, _, _ = _c_call(r, _ffi.VF_BM25_SUBSTATS_STAGE, off, terms, words, n, 10, df=df)
        assert rc == 0 and sq.m == int(mask.sum()) and sq.generation >= 1
        gen, idf, avgdl = sq.generation, _idf(sq, df), sq.total_len / sq.m
        r.add_token_ids(np.array([0, 4]), np.array([3, 9, 9, 1]), remove_ids=[5])      # one leaves, one arrives: n_docs stays
        assert r.num_docs == n
        rc, _, ids, sc = _c_call(r, _ffi.VF_BM25_SUBSTATS_SEARCH, off, terms, words, n, 10, idf=idf, generation=gen, avgdl=avgdl)
        assert rc == -1 and "generation" in _ffi.last_error() and "stage again" in _ffi.last_error()
        assert (ids == 7).all() and (sc == 7.0).all(), "a refused call leaves the outputs untouched"
        # staged again, the request is served: the new corpus's subset
        rc, sq, _, _ = _c_call(r, _ffi.VF_BM25_SUBSTATS_STAGE, off, terms, words, n, 10, df=df)
        assert rc == 0 and sq.generation == gen + 1
        rc, _, ids, sc = _c_call(r, _ffi.VF_BM25_SUBSTATS_SEARCH, off, terms, words, n, 10, idf=_idf(sq, df), generation=sq.generation,
                                 avgdl=sq.total_len / sq.m)
        assert rc == 0
        kept = [d for i, d in enumerate(docs) if i != 5] + [np.array([3, 9, 9, 1])]
        SubsetRef(kept, np.flatnonzero(mask)).check(terms, 10, ids[0], sc[0])


def test_other_refusals(worlds, tmp_path):
    docs, r, d = worlds["A"]
    n = len(docs)
    mask = _filter_a("every_other", docs)
    words, _ = B.filter_words(mask, n)
    off, terms = np.array([0, 3], np.int64), QUERIES[1]
    df = np.zeros(3, np.int64)
    with vf.BM25Retriever(d, stemmer=None, load_corpus=False) as frozen:             # not live: no tf, no lengths
        with pytest.raises(ValueError, match="live=True"):
            frozen.search_columns(QUERIES, 10, subset=mask, stats="subset")
        with pytest.raises(ValueError, match="live=True"):
            frozen.subset_statistics(mask, QUERIES)
        rc, _, ids, _ = _c_call(frozen, _ffi.VF_BM25_SUBSTATS_STAGE, off, terms, words, n, 10, df=df)
        assert rc == -4 and "live handle" in _ffi.last_error() and (ids == 7).all()
        want = frozen.search_columns(QUERIES, 10, subset=mask)
    with pytest.raises(ValueError, match="needs subset="):
        r.search_columns(QUERIES, 10, stats="subset")
    with pytest.raises(ValueError, match="stats="):
        r.search_columns(QUERIES, 10, subset=mask, stats="company")
    with pytest.raises(ValueError, match="stats="):
        r.invoke("t3", 10, subset=mask, stats=None)
    rc, sq, _, _ = _c_call(r, _ffi.VF_BM25_SUBSTATS_STAGE, off, terms, words, n, 10, df=df)
    assert rc == 0
    idf = _idf(sq, df)
    ok = dict(idf=idf, generation=sq.generation, avgdl=sq.total_len / sq.m)
    for bad, word in ((dict(ok, idf=None), "null idf"), (dict(ok, avgdl=0.0), "avgdl"), (dict(ok, avgdl=float("nan")), "avgdl"),
                      (dict(ok, idf=np.array([1.0, -0.5, 1.0])), "idf[1]"), (dict(ok, idf=np.array([1.0, 1.0, np.inf])), "idf[2]"),
                      (dict(ok, b=1.5), "b in")):
        rc, _, ids, sc = _c_call(r, _ffi.VF_BM25_SUBSTATS_SEARCH, off, terms, words, n, 10, **bad)
        assert rc == -1 and word in _ffi.last_error(), (bad, _ffi.last_error())
        assert (ids == 7).all() and (sc == 7.0).all()
    rc, _, _, _ = _c_call(r, _ffi.VF_BM25_SUBSTATS_STAGE, off, terms, words, n, 10)            # a null df
    assert rc == -1 and "null df" in _ffi.last_error()
    rc, _, _, _ = _c_call(r, 3, off, terms, words, n, 10, df=df)
    assert rc == -1 and "phase" in _ffi.last_error()
    rc, _, ids, sc = _c_call(r, _ffi.VF_BM25_SUBSTATS_SEARCH, off, terms, words, n, 10, **ok)   # and the handle is unharmed
    assert rc == 0
    _ref_a("every_other", docs).check(terms, 10, ids[0], sc[0])
    got = r.search_columns(QUERIES, 10, subset=mask)                                           # the corpus mode is what it was
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_the_scratch_is_clean_after_a_call(worlds):
    docs, r, d = worlds["B"]
    rng = np.random.default_rng(9)
    with vf.BM25Retriever(d, stemmer=None, load_corpus=False, live=True) as fresh:
        for k in (100, 4097):
            for density in (0.5, 0.01):
                r.search_columns(QUERIES, k, subset=rng.random(len(docs)) < density, stats="subset")
            after, want = r.search_columns(QUERIES, k), fresh.search_columns(QUERIES, k)
            assert np.array_equal(after[0], want[0]) and np.array_equal(after[1].view(np.uint32), want[1].view(np.uint32))


def test_the_ensemble_under_subset_statistics_is_the_ensemble_of_the_passing_chunks(tmp_path):
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, _, _, _, _ = _world(6)
    n, vocab = len(metas), 40
    tok_docs = make_docs(n, seed=37, vocab=vocab, mean_len=6)
    off, toks = flat(tok_docs)
    full_dir, small_dir = tmp_path / "full", tmp_path / "small"
    B.build_bm25_index_from_ids(off, toks, vocab, str(full_dir))
    rng = np.random.default_rng(41)
    texts = ["t3 t17 t3", "t39 t38", "t0 t1 t2 t25"]
    emb = Emb({t: (base[a] + 0.05 * rng.standard_normal(base.shape[1]).astype(np.float32)).tolist() for t, a in zip(texts, (3, 100, 199))})
    ts = Store(titles, [None] * len(titles), t_emb.tolist())
    kw = dict(retriever_cls=SubsetCosineRetriever, faiss_ts_k=2, bm25_k=9)
    with vf.BM25Retriever(str(full_dir), stemmer=None, load_corpus=False, live=True) as r:
        full = EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=r, where_statistics="subset", **kw)
        default = EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=r, **kw)
        hidden = EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=_HidesTheFilter(r), **kw)
        emitted = differs = 0
        for where in ({"company": "zeekr"}, {"company": ["zeekr", "lotus"], "year": 2023}):
            keep = [i for i, md in enumerate(metas) if _passes(md, where)]
            assert 9 < len(keep) < n
            koff, ktoks = flat([tok_docs[i] for i in keep])
            B.build_bm25_index_from_ids(koff, ktoks, vocab, str(small_dir))
            with vf.BM25Retriever(str(small_dir), stemmer=None, load_corpus=False) as rs:
                small = EnsembleRetriever("unused", Store([docs[i] for i in keep], [metas[i] for i in keep], base[keep].tolist()), ts, 6, emb,
                                          bm25_retriever=rs, **kw)
                for t in texts:
                    got = full.invoke(t, [], where=where)
                    assert got == small.invoke(t, []), "chunk for chunk, score for score: no exception for the BM25 leg"
                    emitted += sum(1 for c in got if c["retriever"] == "BM25")
                    parent = hidden.invoke(t, [], where=where)
                    assert default.invoke(t, [], where=where) == parent, "the default is the parent's result"
                    differs += got != parent
        assert emitted > 0 and differs > 0
    with vf.BM25Retriever(str(full_dir), stemmer=None, load_corpus=False) as frozen:
        with pytest.raises(ValueError, match="subset_statistics"):
            EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=frozen, where_statistics="subset", **kw)
