"""The host side of the live BM25 index: the index directory's term-frequency file, and ``EnsembleRetriever.add_documents`` /
``remove_documents`` with injected legs.  No GPU.  (``save`` against the builder's output, array for array, needs the device and is
in tests/test_gpu_bm25_live.py.)"""
import os

import numpy as np
import pytest

from veritasfi_amd import bm25 as B


def _ids_index(path, seed=0, n=50, vocab=30):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, size=n)
    off = np.concatenate([[0], np.cumsum(lens)])
    toks = rng.integers(0, vocab, size=int(off[-1]))
    B.build_bm25_index_from_ids(off, toks, vocab, str(path))
    return off, toks


def test_the_tf_file_round_trips_and_the_default_return_is_unchanged(tmp_path):
    off, toks = _ids_index(tmp_path)
    three = B.bm25_index_arrays(off, toks, 30)
    four = B.bm25_index_arrays(off, toks, 30, return_tf=True)
    assert len(three) == 3 and len(four) == 4 and all(np.array_equal(a, b) for a, b in zip(three, four))
    tf = four[3]
    assert tf.dtype == np.int32 and tf.min() >= 1 and tf.max() > 1 and tf.sum() == toks.size
    pairs = {(int(t), d): 0 for d in range(50) for t in toks[off[d]:off[d + 1]]}
    for d in range(50):
        for t in toks[off[d]:off[d + 1]]:
            pairs[(int(t), d)] += 1
    col = np.repeat(np.arange(30), np.diff(four[0]))
    assert [pairs[(int(c), int(r))] for c, r in zip(col, four[1])] == tf.tolist()
    ix = B.load_bm25_index(str(tmp_path))
    assert np.array_equal(ix.tf, tf) and ix.tf.dtype == np.int32 and np.array_equal(ix.data.view(np.uint32), four[2].view(np.uint32))
    assert np.array_equal(np.load(tmp_path / B.FILES["tf"]), tf)


def test_texts_write_the_tf_file_too(tmp_path):
    B.build_bm25_index(["alpha beta beta", "beta gamma", "alpha alpha alpha"], str(tmp_path), stemmer=None)
    ix = B.load_bm25_index(str(tmp_path))
    col = np.repeat(np.arange(ix.indptr.size - 1), np.diff(ix.indptr))
    got = {(c, r): t for c, r, t in zip(col.tolist(), ix.indices.tolist(), ix.tf.tolist())}
    v = ix.vocab
    assert got == {(v["alpha"], 0): 1, (v["beta"], 0): 2, (v["beta"], 1): 1, (v["gamma"], 1): 1, (v["alpha"], 2): 3}


def test_a_directory_without_tf_opens_as_before_and_refuses_live(tmp_path):
    _ids_index(tmp_path)
    os.remove(tmp_path / B.FILES["tf"])                       # what bm25s itself writes
    ix = B.load_bm25_index(str(tmp_path))
    assert ix.tf is None and ix.num_docs == 50
    with pytest.raises(ValueError) as e:
        B.BM25Retriever(str(tmp_path), stemmer=None, live=True)
    assert B.FILES["tf"] in str(e.value) and "build_bm25_index" in str(e.value) and "cannot be recovered" in str(e.value)


def test_a_tf_file_that_does_not_fit_is_refused(tmp_path):
    _ids_index(tmp_path)
    tf = np.load(tmp_path / B.FILES["tf"])
    np.save(tmp_path / B.FILES["tf"], tf[:-1])
    with pytest.raises(ValueError, match="term frequency"):
        B.load_bm25_index(str(tmp_path))
    tf[0] = 0
    np.save(tmp_path / B.FILES["tf"], tf)
    with pytest.raises(ValueError, match="term frequency"):
        B.load_bm25_index(str(tmp_path))


# ---- EnsembleRetriever with injected legs ---------------------------------------------------------------------------------------
class Store:
    def __init__(self, docs, metas, embs):
        self.docs, self.metas, self.embs = list(docs), list(metas), list(embs)

    def get(self, ids=None, include=()):
        if ids is None:
            return {"documents": list(self.docs), "metadatas": list(self.metas), "embeddings": list(self.embs)}
        by_id = {m["doc_id"]: i for i, m in enumerate(self.metas)}
        rows = [by_id[i] for i in ids]
        return {"documents": [self.docs[r] for r in rows], "metadatas": [self.metas[r] for r in rows]}


class Emb:
    def embed_query(self, text):
        import zlib
        return np.random.default_rng(zlib.crc32(text.encode())).standard_normal(16).astype(np.float32).tolist()

    def embed_documents(self, texts):
        return [self.embed_query(t) for t in texts]


class Dense:
    """Stands in for FaissRetriever: exact cosine, best first, with the live calls."""

    def __init__(self, embeddings, fn):
        self.x, self.fn, self.calls = np.asarray(embeddings, np.float32).reshape(len(embeddings), -1), fn, []

    def add_embeddings(self, e):
        self.calls.append("add_embeddings")
        self.x = np.concatenate([self.x, np.asarray(e, np.float32)])

    def add_texts(self, texts):
        self.calls.append("add_texts")
        self.x = np.concatenate([self.x, np.asarray(self.fn.embed_documents(list(texts)), np.float32)])

    def remove_ids(self, ids):
        self.calls.append("remove_ids")
        self.x = np.delete(self.x, np.asarray(ids), axis=0)

    def invoke(self, querys, k):
        q = np.asarray([self.fn.embed_query(s) for s in querys], np.float32)
        sim = (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (self.x / np.linalg.norm(self.x, axis=1, keepdims=True)).T
        kk = min(k, self.x.shape[0])
        ids, sc = np.full((len(querys), k), -1, np.int64), np.full((len(querys), k), -3.0e38, np.float32)
        for i in range(len(querys)):
            o = np.lexsort((np.arange(sim.shape[1]), -sim[i]))[:kk]
            ids[i, :kk], sc[i, :kk] = o, sim[i, o]
        return ids, sc


class FrozenDense(Dense):
    def __getattribute__(self, name):
        if name in ("add_embeddings", "add_texts", "remove_ids"):
            raise AttributeError(name)
        return object.__getattribute__(self, name)


class LiveBm25:
    """Stands in for BM25Retriever(live=True): ranks by the count of query words, ties to the lower row."""
    live, exact_prefix = True, True

    def __init__(self, texts):
        self.texts = list(texts)

    num_docs = property(lambda self: len(self.texts))

    def update(self, remove_ids, texts, doc_ids=None):
        gone = set(remove_ids)
        self.texts = [t for i, t in enumerate(self.texts) if i not in gone] + list(texts)

    def remove(self, ids):
        self.update(ids, [])

    def invoke(self, query, k):
        sc = np.asarray([sum(t.split().count(w) for w in query.split()) for t in self.texts], np.float32)
        o = np.lexsort((np.arange(sc.size), -sc))[:k]
        return [int(i) for i in o], sc[o]


WORDS = [f"w{i}" for i in range(25)]


def _chunk(rng, i):
    text = " ".join(rng.choice(WORDS, size=int(rng.integers(2, 9)))) + f" u{i}"
    md = {"doc_id": f"d{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": f"title {i % 5}"}
    if i % 4 < 2:
        md["bundle_id"] = f"b{i // 4}"
    return text, md


def _ensemble(texts, metas, emb, ts, prefetch, dense_cls=Dense, bm=None):
    from veritasfi_amd.ensemble import EnsembleRetriever
    store = Store(texts, metas, [emb.embed_query(t) for t in texts])
    er = EnsembleRetriever("unused", store, ts, 4, emb, faiss_ts_k=2, bm25_k=6, bm25_retriever=bm if bm is not None else LiveBm25(texts),
                           retriever_cls=dense_cls, prefetch_documents=prefetch)
    return er, store


@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_add_and_remove_sequences_equal_an_ensemble_built_fresh(seed, prefetch):
    rng = np.random.default_rng(seed)
    emb = Emb()
    ts = Store([f"title {t}" for t in range(5)], [None] * 5, [emb.embed_query(f"title {t}") for t in range(5)])
    corpus = [_chunk(rng, i) for i in range(40)]
    nxt = 40
    er, store = _ensemble([t for t, _ in corpus], [m for _, m in corpus], emb, ts, prefetch)
    queries = ["w1 w2 w3", "w7 w7 u5", "w20", "title 3"]
    for it in range(12):
        er.invoke(queries[it % 4], [])                        # fills the text-row cache that a removal must forget
        if it % 2 == 0:
            new = [_chunk(rng, nxt + j) for j in range(int(rng.integers(1, 6)))]
            nxt += len(new)
            store.docs += [t for t, _ in new]; store.metas += [m for _, m in new]    # the store is the caller's
            first = er.num_chunk
            rows = er.add_documents([t for t, _ in new], [m for _, m in new],
                                    embeddings=[emb.embed_query(t) for t, _ in new] if it % 4 == 0 else None)
            assert rows == list(range(first, first + len(new)))
            corpus += new
        else:
            pick = sorted(rng.choice(len(corpus), size=int(rng.integers(1, 7)), replace=False).tolist())
            assert er.remove_documents([corpus[i][1]["doc_id"] for i in pick] + [corpus[pick[0]][1]["doc_id"]]) == len(pick)
            corpus = [c for i, c in enumerate(corpus) if i not in set(pick)]
            keep = {m["doc_id"] for _, m in corpus}
            rows = [i for i, m in enumerate(store.metas) if m["doc_id"] in keep]
            store.docs, store.metas = [store.docs[i] for i in rows], [store.metas[i] for i in rows]
        fresh, _ = _ensemble([t for t, _ in corpus], [m for _, m in corpus], emb, ts, prefetch)
        assert er.num_chunk == fresh.num_chunk == len(corpus) and er.chunk_metadata == fresh.chunk_metadata
        assert (er.docid2idx, er._bundle_rows, er._title_rows) == (fresh.docid2idx, fresh._bundle_rows, fresh._title_rows)
        assert er._documents == fresh._documents
        if it % 2:
            assert set(er._text_rows.rows_of([t for t, _ in corpus])) == {-1}   # a removal forgets the remembered rows
        for q in queries:
            assert er.invoke(q, []) == fresh.invoke(q, []), (it, q)
    assert {"add_embeddings", "remove_ids"} <= set(er.faiss_retriever.calls)   # texts are embedded before any leg is asked


def test_a_refused_call_changes_nothing():
    rng = np.random.default_rng(5)
    emb = Emb()
    ts = Store(["title 0"], [None], [emb.embed_query("title 0")])
    corpus = [_chunk(rng, i) for i in range(12)]
    texts, metas = [t for t, _ in corpus], [m for _, m in corpus]
    new_t, new_m = _chunk(rng, 99)

    class PlainBm25:                                           # the host application's: not live
        def invoke(self, query, k):
            return list(range(k)), np.zeros(k, np.float32)

    def state(er):
        return (er.num_chunk, list(er.chunk_metadata), dict(er.docid2idx), {k: list(v) for k, v in er._bundle_rows.items()},
                {k: list(v) for k, v in er._title_rows.items()}, er.faiss_retriever.x.copy().tolist(),
                list(getattr(er.bm25_retriever, "texts", [])), er.invoke("w1 w2", []))

    er, _ = _ensemble(texts, metas, emb, ts, True)
    before = state(er)
    for call in (lambda: er.remove_documents(["d3", "nobody"]),                       # unknown doc_id
                 lambda: er.remove_documents([m["doc_id"] for m in metas]),            # every chunk
                 lambda: er.add_documents([new_t], [metas[3]]),                        # a doc_id that is taken
                 lambda: er.add_documents([new_t, new_t], [new_m, new_m]),             # a doc_id twice
                 lambda: er.add_documents([new_t], [new_m, new_m]),
                 lambda: er.add_documents([new_t], [new_m], embeddings=[[0.0] * 16] * 2)):
        with pytest.raises(ValueError):
            call()
        assert state(er) == before
    assert er.faiss_retriever.calls == []

    er, _ = _ensemble(texts, metas, emb, ts, True, bm=PlainBm25())                    # a BM25 leg that is not the live one
    before = state(er)
    for call in (lambda: er.add_documents([new_t], [new_m]), lambda: er.remove_documents(["d3"])):
        with pytest.raises(ValueError, match="live"):
            call()
        assert state(er) == before and er.faiss_retriever.calls == []

    er, _ = _ensemble(texts, metas, emb, ts, True, dense_cls=FrozenDense)             # a dense retriever without add_* / remove_ids
    before = state(er)
    for call in (lambda: er.add_documents([new_t], [new_m]), lambda: er.remove_documents(["d3"])):
        with pytest.raises(ValueError, match="dense"):
            call()
        assert state(er) == before
    er, _ = _ensemble(texts, metas, emb, ts, True)
    assert er.add_documents([], []) == [] and er.remove_documents([]) == 0 and er.faiss_retriever.calls == []


class _Index:
    d = 16


class RefusingDense(Dense):
    """Has every call, as this package's FaissRetriever has, and refuses the way it refuses: by raising from inside the call."""
    index = _Index()

    def add_embeddings(self, e):
        raise ValueError("rows must be [m, 16]")

    def remove_ids(self, ids):
        raise RuntimeError("a search is in flight")


class UntoldDense(Dense):
    corpus_dtype = None                                       # FaissRetriever.from_index(ix, fn) without corpus_dtype


class TextsOnlyDense(Dense):
    def __getattribute__(self, name):
        if name == "add_embeddings":
            raise AttributeError(name)
        return object.__getattribute__(self, name)


class FailingBm25(LiveBm25):
    def update(self, remove_ids, texts, doc_ids=None):
        raise RuntimeError("out of device memory")


def test_a_dense_leg_that_has_the_calls_but_refuses_leaves_every_leg_as_it_was():
    rng = np.random.default_rng(6)
    emb = Emb()
    ts = Store(["title 0"], [None], [emb.embed_query("title 0")])
    corpus = [_chunk(rng, i) for i in range(12)]
    texts, metas = [t for t, _ in corpus], [m for _, m in corpus]
    new_t, new_m = _chunk(rng, 99)

    def state(er):
        return (er.num_chunk, list(er.chunk_metadata), dict(er.docid2idx), er.faiss_retriever.x.tolist(), list(er.bm25_retriever.texts),
                er.bm25_retriever.num_docs, er.invoke("w1 w2", []))

    class BadEmb(Emb):
        def embed_documents(self, texts):
            raise OSError("the embedder is down")

    er, _ = _ensemble(texts, metas, emb, ts, True, dense_cls=RefusingDense)
    before = state(er)
    for call, err in ((lambda: er.add_documents([new_t], [new_m]), ValueError),                                   # refused inside add_embeddings
                      (lambda: er.add_documents([new_t], [new_m], embeddings=[[0.0] * 16]), ValueError),
                      (lambda: er.add_documents([new_t], [new_m], embeddings=[[0.0] * 8]), ValueError),          # the wrong width, seen here
                      (lambda: er.remove_documents(["d3"]), RuntimeError)):                                       # refused inside remove_ids
        with pytest.raises(err):
            call()
        assert state(er) == before
    er2, _ = _ensemble(texts, metas, emb, ts, True)
    er2.embeddings = BadEmb()                                                                                     # the embedder runs first
    before2 = state(er2)
    with pytest.raises(OSError):
        er2.add_documents([new_t], [new_m])
    er2.embeddings = emb
    assert state(er2) == before2 and er2.faiss_retriever.calls == []

    er, _ = _ensemble(texts, metas, emb, ts, True, dense_cls=UntoldDense)
    before = state(er)
    for call in (lambda: er.add_documents([new_t], [new_m]), lambda: er.remove_documents(["d3"])):
        with pytest.raises(ValueError, match="corpus_dtype"):
            call()
        assert state(er) == before and er.faiss_retriever.calls == []

    er, _ = _ensemble(texts, metas, emb, ts, True, bm=FailingBm25(texts))                                        # the BM25 leg fails after the dense append
    before = state(er)
    with pytest.raises(RuntimeError, match="device memory"):
        er.add_documents([new_t], [new_m])
    assert state(er) == before and er.faiss_retriever.calls == ["add_embeddings", "remove_ids"]                   # appended, then taken back

    er, _ = _ensemble(texts, metas, emb, ts, True, dense_cls=TextsOnlyDense)                                     # add_texts alone: it embeds itself
    with pytest.raises(ValueError, match="add_embeddings"):
        er.add_documents([new_t], [new_m], embeddings=[[0.0] * 16])
    assert er.add_documents([new_t], [new_m]) == [12] and er.faiss_retriever.calls == ["add_texts"] and er.bm25_retriever.num_docs == 13
