"""BM25Retriever on the GPU (vf_bm25_*, csrc/vf_sparse.hip) against the numpy scorer kept here: ids and score BITS equal.

The reference scorer is bm25s's numpy one -- fp32 scores from 0, np.add.at of each query token's postings in query order --
and the ranking contract is canonical: score descending, ties to the lower row, untouched rows (score 0) in ascending order."""
import threading
import zlib

import numpy as np
import pytest

import veritasfi_amd as vf
from veritasfi_amd import bm25 as B

pytestmark = pytest.mark.gpu


def ref_scores(ix, cols):
    sc = np.zeros(ix.num_docs, np.float32)
    for c in cols:
        seg = slice(ix.indptr[c], ix.indptr[c + 1])
        np.add.at(sc, ix.indices[seg], ix.data[seg])
    return sc


def ref_topk(sc, k):
    n = sc.size
    cand = np.arange(n) if k >= n else np.flatnonzero(sc >= np.partition(sc, n - k)[n - k])
    o = cand[np.lexsort((cand, -sc[cand]))][:k]
    return o, sc[o]


def check(ix, cols, k, ids, scores):
    want_ids, want_sc = ref_topk(ref_scores(ix, cols), k)
    assert np.array_equal(np.asarray(ids, np.int64), want_ids)
    assert np.array_equal(np.asarray(scores, np.float32).view(np.uint32), want_sc.view(np.uint32))


def zipf_index(path, n_docs, vocab, mean_len, seed, a=1.25):
    rng = np.random.default_rng(seed)
    lens = rng.poisson(mean_len, size=n_docs)
    off = np.zeros(n_docs + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    toks = (rng.zipf(a, size=int(off[-1])) - 1) % vocab
    B.build_bm25_index_from_ids(off, toks, vocab, str(path))
    return B.load_bm25_index(str(path), load_corpus=False)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("bm25_small")
    ix = zipf_index(d, 20000, 2000, 8, seed=7)
    with vf.BM25Retriever(str(d), stemmer=None) as r:
        yield ix, r


@pytest.mark.parametrize("k", [1, 100, 2048, 4097, "n"])
def test_ids_and_score_bits_match_numpy_at_every_depth(small, k):
    ix, r = small
    k = ix.num_docs if k == "n" else k
    rng = np.random.default_rng(k if isinstance(k, int) else 0)
    queries = [rng.integers(0, 2000, size=int(rng.integers(1, 9))).astype(np.int32) for _ in range(5)]
    queries.append(np.array([1999, 1998], np.int32))            # rare tokens: fewer touched rows than k (the zero tail)
    ids, scores = r.search_columns(queries, k)
    for i, cols in enumerate(queries):
        check(ix, cols, k, ids[i], scores[i])


def test_no_known_token_repeats_and_a_token_in_every_document(tmp_path):
    n = 3000
    rows = [[0, 1 + (i % 7)] + ([8] if i % 3 == 0 else []) for i in range(n)]   # token 0 is in every document
    off = np.concatenate([[0], np.cumsum([len(t) for t in rows])])
    B.build_bm25_index_from_ids(off, np.concatenate(rows), 9, str(tmp_path), vocab={f"w{i}": i for i in range(9)})
    ix = B.load_bm25_index(str(tmp_path))
    with vf.BM25Retriever(str(tmp_path), stemmer=None, stopwords=[]) as r:
        ids, scores = r.invoke("nothing here matches", 50)
        assert ids == list(range(50)) and not scores.any()
        for q in ("w8 w8 w3", "w0", "w0 w8 w0", "w3 W3 unknown w3"):
            cols = r.query_columns(q)
            for k in (10, 1000, n):
                got_ids, got_sc = r.invoke(q, k)
                check(ix, cols, k, got_ids, got_sc)
        assert r.query_columns("w3 W3 unknown w3").tolist() == [3, 3, 3]
        with pytest.raises(ValueError):
            r.invoke("w1", n + 1)
        from veritasfi_amd import _ffi   # the C ABI refuses k > n_docs itself
        off, ids_buf, sc_buf = np.array([0, 1], np.int64), np.zeros(n + 1, np.int64), np.zeros(n + 1, np.float32)
        rc = _ffi.lib().vf_bm25_search(r._h, off.ctypes.data_as(_ffi.p_i64), np.array([1], np.int32).ctypes.data_as(_ffi.p_i32),
                                       1, n + 1, ids_buf.ctypes.data_as(_ffi.p_i64), sc_buf.ctypes.data_as(_ffi.p_f32))
        assert rc == -1 and "k must" in _ffi.last_error()


def test_identical_documents_rank_by_row(tmp_path):
    n = 5000
    off = np.arange(0, 3 * n + 1, 3)
    toks = np.tile([0, 1, 2], n)
    toks[3 * 4000:3 * 4001] = [3, 3, 3]                       # one different document
    B.build_bm25_index_from_ids(off, toks, 4, str(tmp_path))
    ix = B.load_bm25_index(str(tmp_path))
    with vf.BM25Retriever(str(tmp_path), stemmer=None) as r:
        for k in (1, 7, 4096, 4097, n):
            ids, sc = r.search_columns([[0, 1]], k)
            check(ix, [0, 1], k, ids[0], sc[0])
        ids, _ = r.search_columns([[0]], 3)
        assert ids[0].tolist() == [0, 1, 2]


def test_batch_equals_one_at_a_time_threads_and_reruns(small):
    ix, r = small
    rng = np.random.default_rng(11)
    queries = [rng.integers(0, 2000, size=int(rng.integers(0, 12))).astype(np.int32) for _ in range(70)]   # > one group of 64
    ids, sc = r.search_columns(queries, 100)
    for i in range(0, 70, 9):
        one_ids, one_sc = r.search_columns([queries[i]], 100)
        assert np.array_equal(one_ids[0], ids[i]) and np.array_equal(one_sc[0].view(np.uint32), sc[i].view(np.uint32))
    for i in range(70):
        check(ix, queries[i], 100, ids[i], sc[i])
    again_ids, again_sc = r.search_columns(queries, 100)       # a second run: the same bits
    assert np.array_equal(again_ids, ids) and np.array_equal(again_sc.view(np.uint32), sc.view(np.uint32))
    results, errors = {}, []

    def worker(t):
        try:
            results[t] = r.search_columns(queries[t::2], 2048)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        for j, cols in enumerate(queries[t::2]):
            check(ix, cols, 2048, results[t][0][j], results[t][1][j])


def test_min_score_filters_ids_only(small):
    ix, r = small
    q = np.array([5, 17, 3], np.int32)
    ids, sc = r.search_columns([q], 50)
    r.min_score = float(sc[0][20])
    try:
        got_ids, got_sc = r._result(ids[0], sc[0])
    finally:
        r.min_score = None
    assert got_ids == [int(i) for i, s in zip(ids[0], sc[0]) if s >= sc[0][20]] and len(got_sc) == 50


def test_zipf_1m_documents_64_queries(tmp_path):
    ix = zipf_index(tmp_path, 1_000_000, 50_000, 12, seed=3)
    rng = np.random.default_rng(5)
    queries = [((rng.zipf(1.25, size=int(rng.integers(2, 11))) - 1) % 50_000).astype(np.int32) for _ in range(64)]
    with vf.BM25Retriever(str(tmp_path), stemmer=None) as r:
        assert r.info()["n_docs"] == 1_000_000
        for k in (100, 2048):
            ids, sc = r.search_columns(queries, k)
            for i, cols in enumerate(queries):
                check(ix, cols, k, ids[i], sc[i])


def test_10m_documents_few_queries(tmp_path):
    ix = zipf_index(tmp_path, 10_000_000, 100_000, 3, seed=9)
    queries = [np.array([0, 5, 40], np.int32), np.array([1, 1, 700, 3], np.int32), np.array([99_999], np.int32)]
    n = ix.num_docs
    with vf.BM25Retriever(str(tmp_path), stemmer=None) as r:
        ids, sc = r.search_columns(queries, 2048)
        for i, cols in enumerate(queries):
            check(ix, cols, 2048, ids[i], sc[i])
        # deep k (k > 4096: the global bitonic sort) at the sizes where its grid-stride loops take a second turn and the
        # zero tail's block prefix carries: one full ranking of query 0 on the CPU, two searches held to its prefixes
        want = ref_scores(ix, queries[0])
        assert np.count_nonzero(want) > 4_194_304 + 1000   # more selected keys than 8192 workgroups of pairs / 4096 of padding cover
        full_ids, full_sc = ref_topk(want, n)
        # k = 5M < touched: the select runs, 2^23 keys are sorted (16384 workgroups of pairs against a cap of 8192).
        # k = n: every touched key is taken, then the zero tail over all 306 bitmap blocks (> 256: k_bm25_tail_scan carries)
        assert (n + 32767) // 32768 > 256
        for k in (5_000_000, n):
            ids, sc = r.search_columns([queries[0]], k)
            assert np.array_equal(np.asarray(ids[0], np.int64), full_ids[:k]), k
            assert np.array_equal(np.asarray(sc[0], np.float32).view(np.uint32), full_sc[:k].view(np.uint32)), k
        del full_ids, full_sc, ids, sc
        # deep k with almost everything in the tail (17 touched documents), starting in bitmap block 0
        ids, sc = r.search_columns([queries[2]], 4097)
        check(ix, queries[2], 4097, ids[0], sc[0])


class _Store:
    def __init__(self, docs, metas, embs):
        self.docs, self.metas, self.embs = docs, metas, embs
        self.by_id = {m["doc_id"]: i for i, m in enumerate(metas)} if metas and metas[0] else {}

    def get(self, ids=None, include=()):
        if ids is None:
            return {"documents": self.docs, "metadatas": self.metas, "embeddings": self.embs}
        rows = [self.by_id[i] for i in ids]
        return {"documents": [self.docs[r] for r in rows], "metadatas": [self.metas[r] for r in rows]}


class _Emb:
    def __init__(self, d):
        self.d = d

    def embed_query(self, text):
        v = np.random.default_rng(zlib.crc32(text.encode())).standard_normal(self.d)
        return v.astype(np.float32).tolist()


class _NumpyBm25:
    """The upstream call shape: a full numpy ranking of all N rows per request (no exact_prefix)."""

    def __init__(self, path):
        self.ix = B.load_bm25_index(path)
        self.stem, self.stop = B.resolve_stemmer(None), B.STOPWORDS_EN
        self.min_score = None

    def invoke(self, query, k):
        cols = [self.ix.vocab[w] for w in B.tokenize(query, self.stem, self.stop) if w in self.ix.vocab]
        ids, sc = ref_topk(ref_scores(self.ix, cols), k)
        return [int(i) for i in ids], sc


def test_ensemble_with_the_device_leg_equals_the_numpy_full_ranking(tmp_path):
    from veritasfi_amd.ensemble import EnsembleRetriever
    rng = np.random.default_rng(2)
    words = [f"word{i}" for i in range(60)] + ["revenue", "margin", "guidance", "dividend"]
    n = 400
    texts = [" ".join(rng.choice(words, size=int(rng.integers(3, 15)))) for _ in range(n)]
    metas = [{"doc_id": f"d{i}", "prev_chunk_id": "" if i % 4 == 0 else f"d{i - 1}", "next_chunk_id": "" if i % 4 == 3 else f"d{i + 1}",
              "title_summary": f"title {i // 40}", **({"bundle_id": f"b{i // 6}"} if i % 6 < 2 else {})} for i in range(n)]
    B.build_bm25_index(texts, str(tmp_path), doc_ids=[m["doc_id"] for m in metas], stemmer=None)
    d = 32
    chroma = _Store(texts, metas, rng.standard_normal((n, d)).tolist())
    ts = _Store([f"title {t}" for t in range(10)], [None] * 10, rng.standard_normal((10, d)).tolist())
    emb = _Emb(d)
    queries = ["revenue guidance word3", "dividend dividend margin", "nothing known", "word7 word8 word9 word10"]
    with vf.BM25Retriever(str(tmp_path), stemmer=None) as dev:
        outs = []
        for bm in (dev, _NumpyBm25(str(tmp_path))):
            er = EnsembleRetriever("unused", chroma, ts, 5, emb, bm25_k=12, bm25_retriever=bm)
            outs.append([er.invoke(q, []) for q in queries])
    assert outs[0] == outs[1]
    assert any(c["retriever"] == "BM25" for out in outs[0] for c in out)
