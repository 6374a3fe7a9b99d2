"""Prepared BM25 row filters on the GPU (``BM25Retriever.prepare_subset`` -> ``BM25Subset``; vf_bm25_search with VF_BM25_PREPARED, the
kernels k_bm25_sub_df_all and k_bm25_accum_sc of csrc/vf_sparse.hip): a search with ``subset=<prepared>`` returns, ids equal and score
BITS equal, what the unprepared call with the same rows and mode returns -- and, in subset mode, what a fresh retriever over
``bm25_index_arrays`` of the allowed documents alone returns, rows mapped back.

Indexes: S, the 12-row Zipf index over 16 columns of tests/test_bm25_prepared_plan.py (31 postings); C, its 32 768 + 40 rows over
4096 columns (two bitmap blocks, empty columns, a column of eight default chunks); B, 5000 documents over 64 columns for k = 4500 (the
k > 4096 path).  ``BM25Subset.df`` against numpy for all V columns at chunk sizes 1, 3 and 2048; three filters alive at once among
unprepared calls (a filter aliased to the handle's own bitmap would show); staleness and release; the C ABI's refusals; the real
ensemble, dict against ``PreparedWhere``, before and after ``add_documents``."""
import gc

import numpy as np
import pytest

import veritasfi_amd as vf
from veritasfi_amd import _ffi
from veritasfi_amd import bm25 as B
from test_bm25_prepared_plan import _zipf

pytestmark = pytest.mark.gpu

PAD_SCORE = -np.finfo(np.float32).max
U32P = _ffi.ctypes.POINTER(_ffi.ctypes.c_uint32)
F64P = _ffi.ctypes.POINTER(_ffi.ctypes.c_double)
SHAPES = {"S": (12, 16, 3, 3), "C": (32768 + 40, 4096, 4, 5), "B": (5000, 64, 4, 9)}     # n, vocab, mean length, seed


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


class World:
    def __init__(self, name, d):
        self.n, self.vocab, mean_len, seed = SHAPES[name]
        self.off, self.toks = _zipf(self.n, self.vocab, mean_len, seed=seed)
        self.dir = str(d)
        B.build_bm25_index_from_ids(self.off, self.toks, self.vocab, self.dir)
        self.indptr, self.indices, _ = B.bm25_index_arrays(self.off, self.toks, self.vocab)
        self.dl = np.diff(self.off)
        self.live = vf.BM25Retriever(self.dir, stemmer=None, load_corpus=False, live=True)
        self.frozen = vf.BM25Retriever(self.dir, stemmer=None, load_corpus=False)

    def has(self, token):
        out = np.zeros(self.n, bool)
        out[self.indices[self.indptr[token]:self.indptr[token + 1]]] = True
        return out

    def numpy_df(self, mask):
        return np.array([int(mask[self.indices[self.indptr[c]:self.indptr[c + 1]]].sum()) for c in range(self.vocab)], np.int64)

    def close(self):
        self.live.close()
        self.frozen.close()


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    out = {name: World(name, tmp_path_factory.mktemp("bm25_prepared_" + name)) for name in SHAPES}
    yield out
    for w in out.values():
        w.close()


def _queries(w, mask, nq):
    """nq queries over the world's columns; among the first three a repeated token, a token with no allowed posting (when the filter
    leaves one) and an empty query."""
    rng = np.random.default_rng(nq)
    per = np.diff(w.indptr)
    common = np.argsort(-per)[:8].astype(np.int32)
    none_allowed = [int(c) for c in np.argsort(-per, kind="stable")[:256] if per[c] and not mask[w.indices[w.indptr[c]:w.indptr[c + 1]]].any()][:1]
    q = [np.array([common[0], common[1], common[0], common[2]], np.int32),
         np.array(([none_allowed[0]] if none_allowed else []) + [int(common[3])], np.int32),
         np.zeros(0, np.int32)]
    while len(q) < nq:
        q.append(rng.choice(np.concatenate([common, rng.integers(0, w.vocab, size=8).astype(np.int32)]), size=int(rng.integers(0, 7))).astype(np.int32))
    return q[:nq] if nq >= 3 else q[:1]


def _masks(name, w):
    n = w.n
    rng = np.random.default_rng(17)
    if name == "S":
        common = int(np.argmax(np.diff(w.indptr)))
        return {"without_the_commonest_token": ~w.has(common), "rows_0_5_11": np.isin(np.arange(n), [0, 5, 11]), "all": np.ones(n, bool)}
    return {"every_other": np.arange(n) % 2 == 0, "rows_32767_32768": np.isin(np.arange(n), [32767, 32768]), "one_percent": rng.random(n) < 0.01,
            "second_block": np.arange(n) >= 32768}


def _fresh_over_allowed(w, mask, tmp_path, queries, k):
    """ids and scores of a plain retriever over the allowed documents alone, its row i mapped back to the i-th allowed row, padded"""
    rows = np.flatnonzero(mask)
    off = np.zeros(rows.size + 1, np.int64)
    np.cumsum(w.dl[rows], out=off[1:])
    toks = np.concatenate([w.toks[w.off[r]:w.off[r + 1]] for r in rows]) if rows.size else np.zeros(0, np.int64)
    B.build_bm25_index_from_ids(off, toks, w.vocab, str(tmp_path))
    with vf.BM25Retriever(str(tmp_path), stemmer=None, load_corpus=False) as small:
        kk = min(k, rows.size)
        s_ids, s_sc = small.search_columns(queries, kk)
    ids, sc = np.full((len(queries), k), -1, np.int64), np.full((len(queries), k), PAD_SCORE, np.float32)
    ids[:, :kk], sc[:, :kk] = rows[s_ids], s_sc
    return ids, sc


@pytest.mark.parametrize("mode", ["corpus", "subset"])
@pytest.mark.parametrize("name, which", [("S", "without_the_commonest_token"), ("S", "rows_0_5_11"), ("S", "all"), ("C", "every_other"),
                                         ("C", "rows_32767_32768"), ("C", "one_percent"), ("C", "second_block")])
def test_a_prepared_search_is_the_unprepared_call_bit_for_bit(worlds, tmp_path, name, which, mode):
    w = worlds[name]
    mask = _masks(name, w)[which]
    m = int(mask.sum())
    r = w.live
    with r.prepare_subset(mask, stats=mode) as s:
        assert (s.m, s.stats, s.closed, s.stale) == (m, mode, False, False) and s.nbytes >= w.n // 8 and s.generation >= 1
        if mode == "subset":
            assert s.total_len == int(w.dl[mask].sum()) and s.df.dtype == np.int64 and np.array_equal(s.df, w.numpy_df(mask))
        # k < m, k = m and k > m (the padding); the last two while one LDS sort holds k: test_b_* has the global sort
        ks = sorted({max(1, min(m - 1, 10))} | ({m} if m <= 4096 else set()) | ({m + 3} if m + 3 <= min(w.n, 4096) else set()))
        for nq in (1, 3, 65):
            queries = _queries(w, mask, nq)
            assert nq == 1 or (queries[0][0] == queries[0][2] and queries[2].size == 0)
            for k in ks:
                got = r.search_columns(queries, k, subset=s)
                assert same(got, r.search_columns(queries, k, subset=mask, stats=mode)), (nq, k)
                assert same(got, r.search_columns(queries, k, subset=s, stats=mode))      # stats= beside it may be equal
                assert (got[0][:, :min(k, m)] >= 0).all() and (got[0][:, m:] == -1).all() and (got[1][:, m:] == PAD_SCORE).all()
                if mode == "subset" and nq == 3:
                    assert same(got, _fresh_over_allowed(w, mask, tmp_path, queries, k)), k
        one = r.invoke_batch(["t0 t1 t0", ""], ks[-1], subset=s)                        # invoke trims the padding
        two = r.invoke_batch(["t0 t1 t0", ""], ks[-1], subset=np.flatnonzero(mask), stats=mode)
        assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) and len(a[0]) == min(ks[-1], m) for a, b in zip(one, two))
        assert r.invoke("t1 t2", ks[0], subset=s)[0] == r.invoke("t1 t2", ks[0], subset=mask, stats=mode)[0]
    if mode == "corpus":                                                                # ... and on a handle that is not live
        f = w.frozen
        with f.prepare_subset(mask) as s:
            queries = _queries(w, mask, 3)
            for k in ks:
                assert same(f.search_columns(queries, k, subset=s), f.search_columns(queries, k, subset=mask))
        with pytest.raises(ValueError, match="live=True"):
            f.prepare_subset(mask, stats="subset")
        assert f.info()["prepared"] == 0


@pytest.mark.parametrize("mode", ["corpus", "subset"])
@pytest.mark.parametrize("m", [4600, 4400])
def test_b_k_4500_the_global_sort_and_its_padding(worlds, tmp_path, m, mode):
    w = worlds["B"]
    rows = np.sort(np.random.default_rng(m).choice(w.n, size=m, replace=False))
    mask = np.zeros(w.n, bool)
    mask[rows] = True
    queries = _queries(w, mask, 3)
    with w.live.prepare_subset(rows, stats=mode) as s:
        got = w.live.search_columns(queries, 4500, subset=s)
        assert same(got, w.live.search_columns(queries, 4500, subset=rows, stats=mode))
        assert (got[0][:, :min(4500, m)] >= 0).all() and (got[0][:, m:] == -1).all()
        if mode == "subset":
            assert same(got, _fresh_over_allowed(w, mask, tmp_path, queries, 4500))


@pytest.mark.parametrize("chunk", [1, 3, 2048])
def test_df_of_every_column_is_numpys_on_the_12_row_index(worlds, chunk):
    w = worlds["S"]
    rng = np.random.default_rng(chunk)
    filters = [0, (1 << w.n) - 1] + rng.choice(1 << w.n, size=256, replace=False).tolist()
    with vf.BM25Retriever(w.dir, stemmer=None, load_corpus=False, live=True, live_chunk=chunk) as r:
        for f in filters:
            mask = np.array([(f >> i) & 1 for i in range(w.n)], bool)
            with r.prepare_subset(mask, stats="subset") as s:
                assert s.df.shape == (w.vocab,) and np.array_equal(s.df, w.numpy_df(mask)), f
                assert (s.m, s.total_len) == (int(mask.sum()), int(w.dl[mask].sum()))
        assert r.info()["prepared"] == 0


@pytest.mark.parametrize("chunk", [7, 2048])
def test_df_of_every_column_is_numpys_where_a_column_crosses_eight_chunks(worlds, chunk):
    w = worlds["C"]
    assert int(np.diff(w.indptr).max()) > 7 * 2048
    rng = np.random.default_rng(23)
    with vf.BM25Retriever(w.dir, stemmer=None, load_corpus=False, live=True, live_chunk=chunk) as r:
        for mask in (np.arange(w.n) % 2 == 0, rng.random(w.n) < 0.3, np.ones(w.n, bool), np.arange(w.n) == 32768):
            with r.prepare_subset(mask, stats="subset") as s:
                assert np.array_equal(s.df, w.numpy_df(mask)) and s.total_len == int(w.dl[mask].sum())


def test_three_filters_alive_at_once_among_unprepared_calls_each_return_their_own(worlds):
    w = worlds["C"]
    r, n = w.live, w.n
    rng = np.random.default_rng(31)
    mask_a, mask_b, other = rng.random(n) < 0.5, rng.random(n) < 0.05, rng.random(n) < 0.2
    queries = _queries(w, mask_a, 3)
    k = 50
    want_a = r.search_columns(queries, k, subset=mask_a)
    want_b = r.search_columns(queries, k, subset=mask_b, stats="subset")
    want_other = r.search_columns(queries, k, subset=other)
    want_other_s = r.search_columns(queries, k, subset=other, stats="subset")
    want_all = r.search_columns(queries, k)
    assert not same(want_a, want_other) and not same(want_b, want_other_s)
    with r.prepare_subset(mask_a) as a, r.prepare_subset(mask_b, stats="subset") as b, r.prepare_subset([], stats="subset") as none:
        info = r.info()
        assert info["prepared"] == 3 and info["prepared_bytes"] == a.nbytes + b.nbytes + none.nbytes and b.nbytes >= a.nbytes + 8 * w.vocab
        assert (none.m, none.total_len) == (0, 0) and not none.df.any()
        for _ in range(2):
            assert same(r.search_columns(queries, k, subset=a), want_a)
            assert same(r.search_columns(queries, k, subset=other), want_other)           # the handle's own bitmap now holds `other`
            assert same(r.search_columns(queries, k, subset=b), want_b)
            assert same(r.search_columns(queries, k, subset=a), want_a)
            assert same(r.search_columns(queries, k), want_all)
            assert same(r.search_columns(queries, k, subset=other, stats="subset"), want_other_s)
            got = r.search_columns(queries, k, subset=none)
            assert (got[0] == -1).all() and (got[1] == PAD_SCORE).all()
            assert same(r.search_columns(queries, k, subset=b), want_b)
        b.close()
        assert r.info()["prepared"] == 2 and same(r.search_columns(queries, k, subset=a), want_a)
    assert r.info()["prepared"] == 0 and r.info()["prepared_bytes"] == 0


def test_refusals_of_the_python_layer(worlds, tmp_path):
    w = worlds["S"]
    r = w.live
    mask = np.arange(w.n) % 2 == 0
    q = _queries(w, mask, 1)
    with r.prepare_subset(mask, stats="subset") as s, r.prepare_subset(mask) as c:
        with pytest.raises(ValueError, match="stats="):
            r.search_columns(q, 3, subset=s, stats="corpus")
        with pytest.raises(ValueError, match="stats="):
            r.invoke("t1", 3, subset=c, stats="subset")
        with pytest.raises(ValueError, match="another BM25Retriever"):
            w.frozen.search_columns(q, 3, subset=c)
        with pytest.raises(TypeError):
            r.prepare_subset(s)
        with pytest.raises(ValueError, match="outside|range|12"):
            r.prepare_subset([3, w.n])
    for closed in (s, c):
        assert closed.closed and closed.nbytes == 0
        with pytest.raises(ValueError, match="prepare_subset again"):
            r.search_columns(q, 3, subset=closed)
        closed.close()
    # collecting a BM25Subset after its retriever has closed does not touch the library
    own = vf.BM25Retriever(w.dir, stemmer=None, load_corpus=False, live=True)
    left = own.prepare_subset(mask, stats="subset")
    own.close()
    assert left.closed and left.nbytes == 0 and own.info()["prepared"] == 0
    left.close()
    del left
    gc.collect()
    with vf.BM25Retriever(w.dir, stemmer=None, load_corpus=False, live=True) as again:      # a collected one is released by the next call
        lost = again.prepare_subset(mask)
        assert again.info()["prepared"] == 1
        del lost
        gc.collect()
        assert again.info()["prepared"] == 0
        with again.prepare_subset(mask) as s2:
            assert same(again.search_columns(q, 3, subset=s2), again.search_columns(q, 3, subset=mask))


def test_a_stale_subset_is_refused_and_a_new_one_agrees(worlds):
    w = worlds["S"]
    mask = np.arange(w.n) % 3 != 0
    with vf.BM25Retriever(w.dir, stemmer=None, load_corpus=False, live=True) as r:
        q = _queries(w, mask, 3)
        old_c, old_s = r.prepare_subset(mask), r.prepare_subset(mask, stats="subset")
        assert r.info()["prepared"] == 2
        r.add_token_ids(np.array([0, 4]), np.array([3, 9, 9, 1]), remove_ids=[5])      # one leaves, one arrives: n_docs stays
        assert r.num_docs == w.n and r.info()["prepared"] == 0 and r.info()["prepared_bytes"] == 0
        for old in (old_c, old_s):
            assert old.stale and old.nbytes == 0
            with pytest.raises(ValueError, match="prepare_subset again"):
                r.search_columns(q, 5, subset=old)
            old.close()
            old.close()
        with r.prepare_subset(mask) as c, r.prepare_subset(mask, stats="subset") as s:
            assert s.generation == old_s.generation + 1 and r.info()["prepared"] == 2
            assert same(r.search_columns(q, 5, subset=c), r.search_columns(q, 5, subset=mask))
            assert same(r.search_columns(q, 5, subset=s), r.search_columns(q, 5, subset=mask, stats="subset"))
            r.remove([0])
            assert r.num_docs == w.n - 1 and c.stale and s.stale
            with pytest.raises(ValueError, match="prepare_subset again"):
                r.invoke("t1", 3, subset=s)
        assert r.info()["prepared"] == 0


def _c_call(r, phase, k=5, terms=None, off=None, **fields):
    nq = 0 if off is None else off.size - 1
    ids, sc = np.full((max(nq, 1), k), 7, np.int64), np.full((max(nq, 1), k), 7.0, np.float32)
    pq = _ffi.Bm25PreparedQuery()
    pq.phase = phase
    if off is not None:
        pq.q_offsets = off.ctypes.data_as(_ffi.p_i64)
    for key, v in fields.items():
        setattr(pq, key, v)
    rc = _ffi.lib().vf_bm25_search(r._h, _ffi.ctypes.cast(_ffi.ctypes.byref(pq), _ffi.p_i64), None if terms is None else terms.ctypes.data_as(_ffi.p_i32),
                                   nq | _ffi.VF_BM25_PREPARED, k, ids.ctypes.data_as(_ffi.p_i64), sc.ctypes.data_as(_ffi.p_f32))
    return rc, pq, ids, sc


def test_the_c_abi_refuses_what_the_header_says_it_refuses(worlds):
    w = worlds["S"]
    n, V = w.n, w.vocab
    mask = np.arange(n) % 2 == 0
    words, _ = B.filter_words(mask, n)
    off, terms = np.array([0, 2], np.int64), np.array([0, 1], np.int32)
    allow = words.ctypes.data_as(U32P)
    with vf.BM25Retriever(w.dir, stemmer=None, load_corpus=False, live=True) as r:
        P, A, S, R = _ffi.VF_BM25_PREPARED_PREPARE, _ffi.VF_BM25_PREPARED_ARM, _ffi.VF_BM25_PREPARED_SEARCH, _ffi.VF_BM25_PREPARED_RELEASE
        df = np.zeros(V, np.int64)
        for bad, word in ((dict(allow=None), "null allow"), (dict(n_docs=n + 1), "documents"), (dict(mode=2), "mode"), (dict(vocab=V - 1), "vocab"),
                          (dict(df=None), "df"), (dict(chunk=2049), "chunk")):
            fields = dict(dict(allow=allow, n_docs=n, mode=1, vocab=V, df=df.ctypes.data_as(_ffi.p_i64)), **bad)
            rc, pq, _, _ = _c_call(r, P, **fields)
            assert rc == -1 and word in _ffi.last_error() and pq.token == 0, (bad, _ffi.last_error())
        over = words.copy()
        over[0] |= np.uint32(1 << n)
        rc, _, _, _ = _c_call(r, P, allow=over.ctypes.data_as(U32P), n_docs=n, mode=0)
        assert rc == -1 and f"row {n}" in _ffi.last_error()
        rc, _, _, _ = _c_call(r, 9, token=1)
        assert rc == -1 and "phase" in _ffi.last_error()
        rc, _, ids, _ = _c_call(r, S, terms=terms, off=off, token=12345)
        assert rc == -1 and "unknown or released" in _ffi.last_error() and (ids == 7).all()
        rc, pq, _, _ = _c_call(r, P, allow=allow, n_docs=n, mode=1, vocab=V, df=df.ctypes.data_as(_ffi.p_i64), chunk=2)
        assert rc == 0 and pq.token != 0 and pq.m == int(mask.sum()) and np.array_equal(df, w.numpy_df(mask))
        token, gen, m, total = pq.token, pq.generation, pq.m, pq.total_len
        rc, _, ids, _ = _c_call(r, S, terms=terms, off=off, token=token)
        assert rc == -1 and "never armed" in _ffi.last_error() and (ids == 7).all()
        idf = np.log(1.0 + (m - df + 0.5) / (df + 0.5))
        ok = dict(token=token, vocab=V, idf=idf.ctypes.data_as(F64P), avgdl=total / m, k1=1.5, b=0.75)
        neg = idf.copy()
        neg[3] = -0.5
        for bad, word in ((dict(idf=neg.ctypes.data_as(F64P)), "idf[3]"), (dict(avgdl=0.0), "avgdl"), (dict(b=1.5), "b in"), (dict(idf=None), "idf"),
                          (dict(token=token + 99), "unknown or released")):
            rc, _, _, _ = _c_call(r, A, **dict(ok, **bad))
            assert rc == -1 and word in _ffi.last_error(), (bad, _ffi.last_error())
        rc, _, _, _ = _c_call(r, A, **ok)
        assert rc == 0
        rc, _, ids, sc = _c_call(r, S, terms=terms, off=off, token=token)
        assert rc == 0 and same((ids, sc), r.search_columns([terms], 5, subset=mask, stats="subset"))
        rc, cq, _, _ = _c_call(r, P, allow=allow, n_docs=n, mode=0)
        assert rc == 0 and cq.token not in (0, token) and cq.bytes > 0
        rc, _, _, _ = _c_call(r, A, **dict(ok, token=cq.token))
        assert rc == -1 and "corpus mode" in _ffi.last_error()
        r.add_token_ids(np.array([0, 4]), np.array([3, 9, 9, 1]), remove_ids=[5])      # n_docs stays: only the generation tells
        for tok in (token, cq.token):
            rc, _, ids, sc = _c_call(r, S, terms=terms, off=off, token=tok)
            assert rc == -1 and f"generation {gen}" in _ffi.last_error() and "prepare the filter again" in _ffi.last_error()
            assert (ids == 7).all() and (sc == 7.0).all(), "a refused call leaves the outputs untouched"
        rc, _, _, _ = _c_call(r, A, **ok)
        assert rc == -1 and "prepare the filter again" in _ffi.last_error()
        for tok in (token, cq.token):
            assert _c_call(r, R, token=tok)[0] == 0
            rc, _, _, _ = _c_call(r, R, token=tok)
            assert rc == -1 and "unknown or released" in _ffi.last_error()
        got = r.search_columns([terms], 5, subset=mask)                                  # and the handle is unharmed
        with r.prepare_subset(mask) as s:
            assert same(r.search_columns([terms], 5, subset=s), got)
    with vf.BM25Retriever(w.dir, stemmer=None, load_corpus=False) as frozen:
        rc, _, _, _ = _c_call(frozen, _ffi.VF_BM25_PREPARED_PREPARE, allow=allow, n_docs=n, mode=1, vocab=V, df=df.ctypes.data_as(_ffi.p_i64))
        assert rc == -4 and "live handle" in _ffi.last_error()


# ---- end to end: the real ensemble, a dict against a PreparedWhere -----------------------------------------------------------------
class _Store:
    def __init__(self, docs, metas, embs):
        self.docs, self.metas, self.embs = list(docs), list(metas), list(embs)

    def get(self, ids=None, include=()):
        if ids is None:
            return {"documents": list(self.docs), "metadatas": list(self.metas), "embeddings": list(self.embs)}
        by_id = {m["doc_id"]: i for i, m in enumerate(self.metas)}
        rows = [by_id[i] for i in ids]
        return {"documents": [self.docs[r] for r in rows], "metadatas": [self.metas[r] for r in rows]}


class _Emb:
    def __init__(self, d):
        self.d = d

    def embed_query(self, text):
        import zlib
        return np.random.default_rng(zlib.crc32(text.encode())).standard_normal(self.d).astype(np.float32).tolist()


@pytest.mark.parametrize("mode", ["corpus", "subset"])
def test_the_real_ensemble_a_dict_against_a_prepared_where_before_and_after_add_documents(tmp_path, mode):
    from veritasfi_amd.ensemble import EnsembleRetriever
    from veritasfi_amd.index import RowSubset
    rng = np.random.default_rng(2)
    vocab = [f"word{i}" for i in range(60)] + ["revenue", "margin", "guidance", "dividend"]
    n, extra, d = 300, 40, 32
    emb = _Emb(d)
    texts = [" ".join(rng.choice(vocab, size=int(rng.integers(3, 15)))) + f" uniq{i}" for i in range(n + extra)]
    metas = [{"doc_id": f"d{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": f"title {i // 40}", "company": ("zeekr", "lotus", "other")[(i // 3) % 3],
              **({"bundle_id": f"b{i // 6}"} if i % 6 < 2 else {})} for i in range(n + extra)]
    vecs = [emb.embed_query(t) for t in texts]
    ts = _Store([f"title {t}" for t in range(9)], [None] * 9, rng.standard_normal((9, d)).tolist())
    queries = ["revenue guidance word3", "dividend dividend margin", "uniq312 word7", "word7 word8 word9 word10"]
    where = {"company": ["zeekr", "other"]}
    assert metas[312]["company"] == "other" and metas[310]["company"] == "lotus"
    B.build_bm25_index(texts[:n], str(tmp_path / "live"), doc_ids=[m["doc_id"] for m in metas[:n]], stemmer=None)
    store = _Store(texts[:n], metas[:n], vecs[:n])
    with vf.BM25Retriever(str(tmp_path / "live"), stemmer=None, live=True) as bm:
        er = EnsembleRetriever("unused", store, ts, 5, emb, bm25_k=12, bm25_retriever=bm, prefetch_documents=True, where_statistics=mode)
        with er.prepare_where(where) as pw:
            assert isinstance(pw.dense, RowSubset) and isinstance(pw.bm25, B.BM25Subset) and pw.bm25.stats == mode and bm.info()["prepared"] == 1
            first = pw.bm25
            want = [er.invoke(q, [], where=where) for q in queries]
            assert [er.invoke(q, [], where=pw) for q in queries] == want
            assert any(c["retriever"] == "BM25" for out in want for c in out) and any(c["retriever"] == "FAISS" for out in want for c in out)
            store.docs += texts[n:]; store.metas += metas[n:]; store.embs += vecs[n:]      # the store is the caller's
            er.add_documents(texts[n:], metas[n:], embeddings=np.asarray(vecs[n:], np.float32))
            assert first.stale and bm.info()["prepared"] == 0
            got = [er.invoke(q, [], where=pw) for q in queries]
            assert pw.bm25 is not first and not pw.bm25.stale and bm.info()["prepared"] == 1 and pw.passing[-1] >= n
            assert got == [er.invoke(q, [], where=where) for q in queries]
            assert any(c["metadata"]["doc_id"] == "d312" for c in got[2]) and not any(c["metadata"]["doc_id"] == "d312" for c in want[2])
            assert not any(c["metadata"]["company"] == "lotus" for out in got for c in out)
        assert bm.info()["prepared"] == 0
