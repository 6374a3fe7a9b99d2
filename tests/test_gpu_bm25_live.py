"""A live BM25 index on the GPU (BM25Retriever(live=True): vf_bm25_create with VF_BM25_LIVE, the k_bm25_live_* kernels of
csrc/vf_sparse.hip) against ``bm25_index_arrays`` run on the edited token lists.

After every update the handle's arrays -- downloaded through ``arrays()`` / ``save`` -- equal the fresh build's array for array, the
scores bit for bit, and searches return the ids and score bits the numpy scorer gives on that fresh build."""
import numpy as np
import pytest

import veritasfi_amd as vf
from veritasfi_amd import _ffi
from veritasfi_amd import bm25 as B

pytestmark = pytest.mark.gpu


class Ix:
    def __init__(self, indptr, indices, data, n):
        self.indptr, self.indices, self.data, self.num_docs = indptr, indices, data, n


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


class World:
    """The token lists the handle should hold, edited on the host beside it."""

    def __init__(self, docs, vocab):
        self.docs, self.vocab = [np.asarray(d, np.int64) for d in docs], vocab

    def flat(self, docs=None):
        docs = self.docs if docs is None else [np.asarray(d, np.int64) for d in docs]
        off = np.concatenate([[0], np.cumsum([d.size for d in docs])]).astype(np.int64)
        return off, (np.concatenate(docs) if docs else np.zeros(0, np.int64))

    def write(self, path):
        off, toks = self.flat()
        B.build_bm25_index_from_ids(off, toks, self.vocab, str(path))
        return str(path)

    def edit(self, remove=(), add=()):
        gone = set(int(i) for i in remove)
        self.docs = [d for i, d in enumerate(self.docs) if i not in gone] + [np.asarray(d, np.int64) for d in add]
        for d in add:
            self.vocab = max(self.vocab, int(max(d)) + 1 if len(d) else 0)

    def expect(self):
        off, toks = self.flat()
        return B.bm25_index_arrays(off, toks, self.vocab, return_tf=True)


def zipf_docs(n_docs, vocab, mean_len, seed, a=1.25):
    rng = np.random.default_rng(seed)
    lens = rng.poisson(mean_len, size=n_docs)
    toks = (rng.zipf(a, size=int(lens.sum())) - 1) % vocab
    return np.split(toks, np.cumsum(lens)[:-1])


def verify(r, w, queries=(), ks=()):
    """The handle's arrays equal the fresh build's, and searches on it rank as numpy does on that build."""
    indptr, indices, data, tf = w.expect()
    got = r.arrays()
    n = len(w.docs)
    assert r.num_docs == n and r.info()["n_docs"] == n and r.info()["vocab"] == w.vocab and r.info()["nnz"] == data.size
    assert np.array_equal(got[0], indptr) and np.array_equal(got[1], indices) and np.array_equal(got[3], tf)
    assert np.array_equal(got[2].view(np.uint32), data.view(np.uint32))
    ix = Ix(indptr, indices, data, n)
    for k in ks:
        k = n if k == "n" else min(k, n)
        ids, scores = r.search_columns(queries, k)
        for i, cols in enumerate(queries):
            check(ix, cols, k, ids[i], scores[i])
    return ix


def step(r, w, remove=(), add=()):
    off, toks = w.flat(add)
    n0 = len(w.docs)
    if len(add):
        first = r.add_token_ids(off, toks, remove_ids=remove)
        assert first == n0 - len(set(int(i) for i in remove))
    else:
        assert r.remove(remove) == len(set(int(i) for i in remove))
    w.edit(remove, add)


def test_add_remove_and_update_on_the_zipf_index(tmp_path):
    w = World(zipf_docs(20000, 2000, 8, seed=7), 2000)
    rng = np.random.default_rng(1)
    queries = [rng.integers(0, 2000, size=int(rng.integers(1, 9))).astype(np.int32) for _ in range(3)]
    queries.append(np.array([1999, 1998], np.int32))   # rare tokens: fewer touched rows than k (the zero tail)
    ks = (1, 100, 4097, "n")
    with vf.BM25Retriever(w.write(tmp_path), stemmer=None, live=True) as r:
        verify(r, w, queries, ks)                                                   # created live: scores computed on the device
        step(r, w, add=zipf_docs(100, 2000, 8, seed=8))
        verify(r, w, queries, ks)
        step(r, w, remove=rng.choice(len(w.docs), size=100, replace=False))
        verify(r, w, queries, ks)
        step(r, w, remove=[0])
        verify(r, w, queries, ks)
        step(r, w, remove=[len(w.docs) - 1])
        verify(r, w, queries, ks)
        step(r, w, remove=np.arange(5000, 6000))
        verify(r, w, queries, ks)
        step(r, w, remove=rng.choice(len(w.docs), size=100, replace=False), add=zipf_docs(100, 2000, 8, seed=9))
        verify(r, w, queries, ks)
        out = tmp_path / "saved"                                                    # save = what the builder writes, array for array
        r.save(str(out))
        off, toks = w.flat()
        B.build_bm25_index_from_ids(off, toks, w.vocab, str(tmp_path / "built"))
        for name in ("data", "indices", "indptr", "tf"):
            a, b = np.load(out / B.FILES[name]), np.load(tmp_path / "built" / B.FILES[name])
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if name == "data" else a, b.view(np.uint32) if name == "data" else b), name
    with vf.BM25Retriever(str(out), stemmer=None) as plain, vf.BM25Retriever(str(out), stemmer=None, live=True) as again:   # a restart
        a, b = plain.search_columns(queries, 100), again.search_columns(queries, 100)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _every_document_docs(n=3000):
    return [[0, 1 + (i % 7)] + ([8] if i % 3 == 0 else []) for i in range(n)]   # token 0 is in every document


@pytest.mark.parametrize("chunk", [0, 64])
def test_a_token_in_every_document_an_emptied_column_new_columns_and_repeats(tmp_path, chunk):
    docs = _every_document_docs()
    docs[5], docs[6] = [0, 9, 9], [9, 0]                     # column 9 lives in rows 5 and 6 only
    w = World(docs, 10)
    q = [np.array(c, np.int32) for c in ([0], [9], [8, 8, 3], [0, 8, 0], [9, 1])]
    with vf.BM25Retriever(w.write(tmp_path), stemmer=None, live=True, live_chunk=chunk) as r:   # chunk 64: column 0 spans 47 chunks
        verify(r, w, q, (10, 1000, "n"))
        step(r, w, remove=[5, 6])                            # column 9 is emptied and stays
        ix = verify(r, w, q, (10, 1000, "n"))
        assert ix.indptr[9] == ix.indptr[10] and w.vocab == 10
        ids, sc = r.search_columns([[9]], 7)
        assert ids[0].tolist() == list(range(7)) and not sc.any()
        step(r, w, add=[[0, 12, 12, 12, 12], [11, 3], [0] * 40, [9]])   # new columns 11 and 12 (10 stays empty), tf 4 and 40, column 9 again
        q += [np.array(c, np.int32) for c in ([12, 11], [10], [0, 12])]
        ix = verify(r, w, q, (10, 1000, "n"))
        assert w.vocab == 13 and ix.indptr[10] == ix.indptr[11] and "t12" in r.vocab
        step(r, w, remove=np.arange(0, 2990, 2), add=[[0, 1], [0, 1]])
        verify(r, w, q, (10, 1000, "n"))


def test_identical_documents_rank_by_row_after_renumbering(tmp_path):
    n = 5000
    docs = [[0, 1, 2] for _ in range(n)]
    docs[4000] = [3, 3, 3]
    w = World(docs, 4)
    with vf.BM25Retriever(w.write(tmp_path), stemmer=None, live=True) as r:
        step(r, w, remove=[0, 1, 17, 4000], add=[[0, 1, 2], [0, 1, 2]])
        verify(r, w, [np.array([0, 1], np.int32), np.array([3], np.int32)], (1, 7, 4096, 4097, "n"))
        ids, _ = r.search_columns([[0]], 3)
        assert ids[0].tolist() == [0, 1, 2]


def test_one_chunk_holds_hundreds_of_column_starts(tmp_path):
    rng = np.random.default_rng(4)
    vocab = 20000
    docs = [rng.choice(vocab, size=2, replace=False) for _ in range(300)]   # 600 postings over 20 000 columns: ~2000 starts per 64 postings
    w = World(docs, vocab)
    used = np.unique(np.concatenate(docs))
    q = [used[:5].astype(np.int32), used[-3:].astype(np.int32), np.array([int(used[7]), 19999, 0], np.int32)]
    with vf.BM25Retriever(w.write(tmp_path), stemmer=None, live=True, live_chunk=64) as r:
        verify(r, w, q, (5, "n"))
        step(r, w, remove=rng.choice(300, size=40, replace=False), add=[rng.choice(vocab + 50, size=3, replace=False) for _ in range(30)])
        verify(r, w, q, (5, "n"))
        step(r, w, remove=np.arange(1, 290))
        verify(r, w, q, (1, "n"))


def test_the_scratch_follows_the_document_count_across_a_bitmap_block(tmp_path):
    w = World(zipf_docs(32700, 500, 4, seed=12), 500)
    q = [np.array([3, 17, 250], np.int32), np.array([499, 498], np.int32)]
    with vf.BM25Retriever(w.write(tmp_path), stemmer=None, live=True) as r:
        verify(r, w, q, (100, 4097))
        step(r, w, add=zipf_docs(100, 500, 4, seed=13))      # 32 800: a second 32 768-row bitmap block
        verify(r, w, q, (100, 4097, "n"))
        step(r, w, remove=np.arange(32000, 32100))           # and back
        verify(r, w, q, (100, 4097, "n"))


def test_seeded_random_sequences_equal_a_fresh_build_after_every_step(tmp_path):
    rng = np.random.default_rng(2026)
    w = World(zipf_docs(5000, 800, 6, seed=21), 800)
    q = [rng.integers(0, 800, size=4).astype(np.int32) for _ in range(2)]
    with vf.BM25Retriever(w.write(tmp_path), stemmer=None, live=True, live_chunk=int(rng.integers(1, 2049))) as r:
        for it in range(30):
            kind = it % 3
            n = len(w.docs)
            remove = rng.choice(n, size=int(rng.integers(1, min(n - 1, 400))), replace=False) if kind != 0 else []
            if it % 7 == 3:
                remove = np.concatenate([remove, remove[:3]])                      # duplicates count once
            add = zipf_docs(int(rng.integers(1, 300)), 800 + 5 * (it % 4 == 0), 6, seed=100 + it) if kind != 1 else []
            step(r, w, remove=remove, add=add)
            verify(r, w, q, (50,) if it % 5 else (50, 4097))


def test_refusals_change_nothing(tmp_path):
    w = World(zipf_docs(2000, 300, 6, seed=31), 300)
    q = [np.array([1, 5, 200], np.int32), np.array([299], np.int32)]
    path = w.write(tmp_path / "ix")
    lib = _ffi.lib()

    def stage(h, remove=(), n_new=0, indptr=None, rows=(), tf=(), vocab=300):
        remove = np.asarray(remove, np.int64)
        indptr = np.zeros(vocab + 1, np.int64) if indptr is None else np.asarray(indptr, np.int64)
        rows, tf, counts = np.asarray(rows, np.int32), np.asarray(tf, np.int32), np.zeros(vocab, np.int64)
        d = _ffi.Bm25Delta()
        d.vocab, d.n_new, d.n_remove = vocab, n_new, remove.size
        d.indptr, d.rows, d.tf = indptr.ctypes.data_as(_ffi.p_i64), rows.ctypes.data_as(_ffi.p_i32), tf.ctypes.data_as(_ffi.p_i32)
        d.remove, d.counts = remove.ctypes.data_as(_ffi.p_i64), counts.ctypes.data_as(_ffi.p_i64)
        hh = _ffi.vp(h.value)
        rc = lib.vf_bm25_create(_ffi.ctypes.cast(_ffi.ctypes.byref(d), _ffi.p_i64), 0, None, None, 0, 0, _ffi.VF_BM25_LIVE, _ffi.ctypes.byref(hh), None)
        assert hh.value == h.value                      # the handle stays the handle, whatever the result
        return rc, _ffi.last_error()

    with vf.BM25Retriever(path, stemmer=None, live=True) as r:
        before = [r.search_columns(q, k) for k in (10, 2000)]

        def unchanged():
            verify(r, w)
            for (ids, sc), k in zip(before, (10, 2000)):
                got = r.search_columns(q, k)
                assert np.array_equal(got[0], ids) and np.array_equal(got[1].view(np.uint32), sc.view(np.uint32))

        assert r.remove([]) == 0 and r.add_token_ids([0], []) == 2000 and r.update([], []) == 2000   # nothing to do: no rewrite, nothing changes
        unchanged()
        with pytest.raises(ValueError, match=r"ids\[2\] = 2000"):
            r.remove([3, 4, 2000])
        rc, msg = stage(r._h, remove=[3, 4, 2000])      # the C ABI refuses it itself, naming the position
        assert rc == -1 and "remove[2] = 2000" in msg
        rc, msg = stage(r._h, remove=[-1])
        assert rc == -1 and "remove[0]" in msg
        unchanged()
        with pytest.raises(ValueError, match="no document"):
            r.remove(np.arange(2000))
        rc, msg = stage(r._h, remove=np.arange(2000))
        assert rc == -1 and "no document" in msg
        unchanged()
        ptr = np.zeros(301, np.int64)
        ptr[8:] = 2
        rc, msg = stage(r._h, n_new=2, indptr=ptr, rows=[1, 1], tf=[1, 1])      # a duplicate row inside one delta column
        assert rc == -1 and "strictly ascending" in msg
        rc, msg = stage(r._h, n_new=2, indptr=ptr, rows=[0, 1], tf=[1, 0])      # tf below 1
        assert rc == -1 and "frequency" in msg
        rc, msg = stage(r._h, n_new=2, indptr=ptr, rows=[0, 2], tf=[1, 1])      # a row past the delta's documents
        assert rc == -1 and "out of range" in msg
        unchanged()
        rc, msg = stage(r._h, n_new=1, indptr=ptr, rows=[0, 0], tf=[1, 1])      # a stage that is never committed ...
        assert rc == -1
        ptr[:] = 0
        ptr[8:] = 1
        rc, msg = stage(r._h, remove=[7], n_new=1, indptr=ptr, rows=[0], tf=[2])
        assert rc == 0, msg
        unchanged()                                     # ... changes nothing, and the next update discards it
        step(r, w, remove=[1], add=[[4, 4]])
        verify(r, w, q, (10,))

    with vf.BM25Retriever(path, stemmer=None) as plain:                           # not created live
        ids, sc = plain.search_columns(q, 10)
        rc, msg = stage(plain._h, remove=[1])
        assert rc == -1 and "not created live" in msg
        with pytest.raises(ValueError, match="not live"):
            plain.remove([1])
        with pytest.raises(ValueError, match="not live"):
            plain.add_texts(["some words"])
        got = plain.search_columns(q, 10)
        assert np.array_equal(got[0], ids) and np.array_equal(got[1].view(np.uint32), sc.view(np.uint32))

    import os
    os.remove(os.path.join(path, B.FILES["tf"]))                                   # a directory as bm25s writes it
    with pytest.raises(ValueError, match="build_bm25_index"):
        vf.BM25Retriever(path, stemmer=None, live=True)
    with vf.BM25Retriever(path, stemmer=None) as plain:
        with pytest.raises(ValueError, match="not live"):
            plain.update([0], ["words"])
        got = plain.search_columns(q, 10)
        assert np.array_equal(got[0], ids) and np.array_equal(got[1].view(np.uint32), sc.view(np.uint32))


def test_texts_are_tokenised_by_the_retriever_and_the_corpus_follows(tmp_path):
    texts = ["the revenue grew", "margin guidance was cut", "dividend and revenue", "nothing else here"]
    B.build_bm25_index(texts, str(tmp_path), doc_ids=["a", "b", "c", "d"], stemmer=None)
    with vf.BM25Retriever(str(tmp_path), stemmer=None, live=True) as r:
        assert r.add_texts(["Revenue revenue buyback", "the and"], doc_ids=["e", "f"]) == 4   # "buyback" is new; the second text is all stopwords
        assert r.update([1, 1], ["guidance raised"], doc_ids=["g"]) == 5
        assert r.corpus == ["a", "c", "d", "e", "f", "g"] and r.num_docs == 6
        kept = [texts[0], texts[2], texts[3], "Revenue revenue buyback", "the and", "guidance raised"]
        B.build_bm25_index(kept, str(tmp_path / "fresh"), stemmer=None)
        with vf.BM25Retriever(str(tmp_path / "fresh"), stemmer=None) as fresh:
            for query in ("revenue", "buyback revenue", "guidance", "raised margin", "nothing"):
                a, b = r.invoke(query, 6), fresh.invoke(query, 6)
                assert a[0] == b[0] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), query


# ---- end to end: a real EnsembleRetriever whose three parts follow together ---------------------------------------------------
class _Store:
    def __init__(self, docs, metas, embs):
        self.docs, self.metas, self.embs = list(docs), list(metas), list(embs)

    def get(self, ids=None, include=()):
        if ids is None:
            return {"documents": list(self.docs), "metadatas": list(self.metas), "embeddings": list(self.embs)}   # copies, as Chroma answers
        by_id = {m["doc_id"]: i for i, m in enumerate(self.metas)}
        rows = [by_id[i] for i in ids]
        return {"documents": [self.docs[r] for r in rows], "metadatas": [self.metas[r] for r in rows]}


class _Emb:
    def __init__(self, d):
        self.d = d

    def embed_query(self, text):
        import zlib
        return np.random.default_rng(zlib.crc32(text.encode())).standard_normal(self.d).astype(np.float32).tolist()


def test_ensemble_add_then_remove_equals_an_ensemble_built_fresh(tmp_path):
    from veritasfi_amd.ensemble import EnsembleRetriever
    rng = np.random.default_rng(2)
    words = [f"word{i}" for i in range(60)] + ["revenue", "margin", "guidance", "dividend"]
    n, d = 300, 32
    emb = _Emb(d)
    texts = [" ".join(rng.choice(words, size=int(rng.integers(3, 15)))) + f" uniq{i}" for i in range(n + 40)]
    metas = [{"doc_id": f"d{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": f"title {i // 40}",
              **({"bundle_id": f"b{i // 6}"} if i % 6 < 2 else {})} for i in range(n + 40)]
    vecs = [emb.embed_query(t) for t in texts]
    ts = _Store([f"title {t}" for t in range(9)], [None] * 9, rng.standard_normal((9, d)).tolist())
    queries = ["revenue guidance word3", "dividend dividend margin", "uniq310 word7", "word7 word8 word9 word10"]
    gone = [f"d{i}" for i in (0, 7, 150, 299, 305, 306)]
    keep = [i for i in range(n + 40) if f"d{i}" not in gone]

    B.build_bm25_index(texts[:n], str(tmp_path / "live"), doc_ids=[m["doc_id"] for m in metas[:n]], stemmer=None)
    store = _Store(texts[:n], metas[:n], vecs[:n])
    with vf.BM25Retriever(str(tmp_path / "live"), stemmer=None, live=True) as bm:
        er = EnsembleRetriever("unused", store, ts, 5, emb, bm25_k=12, bm25_retriever=bm, prefetch_documents=True)
        er.invoke(queries[0], [])
        store.docs += texts[n:]; store.metas += metas[n:]; store.embs += vecs[n:]      # the store is the caller's
        assert er.add_documents(texts[n:], metas[n:], embeddings=np.asarray(vecs[n:], np.float32)) == list(range(n, n + 40))
        with pytest.raises(ValueError):
            er.add_documents(["again"], [metas[3]])                                     # a doc_id that is taken: nothing changes
        with pytest.raises(ValueError):
            er.remove_documents(["d1", "nobody"])
        with pytest.raises(ValueError, match="width"):                                  # the real dense leg would refuse it: seen before any leg changes
            er.add_documents(["wrong width"], [{"doc_id": "w"}], embeddings=np.zeros((1, d + 1), np.float32))
        assert bm.num_docs == n + 40 and er.faiss_retriever.index.n == n + 40
        from veritasfi_amd.faiss_retriever import FaissRetriever
        er.faiss_retriever, kept = FaissRetriever.from_index(er.faiss_retriever.index, emb), er.faiss_retriever   # not told the corpus_dtype
        for call in (lambda: er.add_documents(["more"], [{"doc_id": "w"}]), lambda: er.remove_documents(["d1"])):
            with pytest.raises(ValueError, match="corpus_dtype"):
                call()
        er.faiss_retriever = kept
        assert bm.num_docs == n + 40 and er.faiss_retriever.index.n == n + 40
        assert er.num_chunk == n + 40 and bm.num_docs == n + 40
        assert er.remove_documents(gone) == len(gone)
        got = [er.invoke(q, []) for q in queries]
        maps = (er.docid2idx, er._bundle_rows, er._title_rows, er.chunk_metadata)

    B.build_bm25_index([texts[i] for i in keep], str(tmp_path / "fresh"), doc_ids=[f"d{i}" for i in keep], stemmer=None)
    fresh_store = _Store([texts[i] for i in keep], [metas[i] for i in keep], [vecs[i] for i in keep])
    with vf.BM25Retriever(str(tmp_path / "fresh"), stemmer=None) as bm:
        fresh = EnsembleRetriever("unused", fresh_store, ts, 5, emb, bm25_k=12, bm25_retriever=bm, prefetch_documents=True)
        want = [fresh.invoke(q, []) for q in queries]
        assert maps == (fresh.docid2idx, fresh._bundle_rows, fresh._title_rows, fresh.chunk_metadata)
    assert got == want
    assert any(c["retriever"] == "BM25" for out in got for c in out) and any(c["metadata"]["doc_id"] == "d310" for c in got[2])
