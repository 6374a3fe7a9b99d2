"""``EnsembleRetriever.prepare_where`` / ``invoke(..., where=PreparedWhere)``: what reaches the two legs and when the host work runs.
CPU-only, with stand-in retrievers that record their calls (the GPU objects are held to the unprepared calls in
tests/test_gpu_bm25_prepared.py).

A ``PreparedWhere`` reaches the dense leg as the index's ``row_subset`` object and the BM25 leg as its ``prepare_subset`` object, with
no ``stats=`` beside it; ``rows_where`` runs once for many invokes; after ``add_documents`` / ``remove_documents`` the next invoke
prepares again (the old BM25 object is closed) and the output equals that of the dict form; legs that offer neither call get the ids;
a PreparedWhere of another retriever, a closed one and a non-dict are refused."""
import numpy as np
import pytest

from test_ensemble_where import Store, SubsetCosineRetriever, _passes, _world


class FakeRowSubset:
    def __init__(self, ids):
        self.ids = np.asarray(ids, np.int64).copy()


class FakeIndex:
    device_ids = None
    d = None

    def __init__(self):
        self.made = []

    def row_subset(self, ids):
        self.made.append(FakeRowSubset(ids))
        return self.made[-1]


class LiveDense(SubsetCosineRetriever):
    """The cosine stand-in with an index that offers ``row_subset``, and rows that can be added and removed."""
    corpus_dtype = "float32"

    def __init__(self, embeddings, embedding_fn):
        super().__init__(embeddings, embedding_fn)
        self.index, self.got = FakeIndex(), []

    def invoke(self, querys, k, subset=None):
        self.got.append(subset)
        return super().invoke(querys, k, subset=subset.ids if isinstance(subset, FakeRowSubset) else subset)

    def add_embeddings(self, emb):
        x = np.asarray(emb, np.float32)
        self.x = np.concatenate([self.x, x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)])

    def remove_ids(self, ids):
        self.x = np.delete(self.x, np.asarray(ids, np.int64), axis=0)


class FakeBm25Subset:
    def __init__(self, owner, rows, stats):
        self.owner, self.rows, self.stats, self.generation, self.closed = owner, np.asarray(rows, np.int64).copy(), stats, owner.generation, False

    def close(self):
        self.closed = True


class LiveBm25:
    """A BM25 leg that filters on its own over a fixed ranking, offers ``prepare_subset`` (objects that refuse once stale), follows
    added and removed documents, and records every call."""
    exact_prefix = filtered_prefix = subset_statistics = live = True

    def __init__(self, order, scores):
        self.order, self.scores, self.calls, self.prepared, self.generation = list(order), list(scores), [], [], 1
        self.num_docs = len(self.order)

    def prepare_subset(self, rows, stats="corpus"):
        self.prepared.append(FakeBm25Subset(self, rows, stats))
        return self.prepared[-1]

    def invoke(self, query, k, **kw):
        self.calls.append((query, k, dict(kw)))
        s = kw.get("subset")
        if isinstance(s, FakeBm25Subset):
            assert "stats" not in kw, "the mode is the prepared object's own"
            if s.closed or s.generation != self.generation:
                raise ValueError("stale or closed: call prepare_subset again")
            s = s.rows
        allow = None if s is None else set(np.asarray(s).tolist())
        kept = [(r, sc) for r, sc in zip(self.order, self.scores) if allow is None or r in allow][:k]
        return [r for r, _ in kept], [sc for _, sc in kept]

    def update(self, remove, texts, doc_ids=None):
        assert not len(remove)
        for _ in texts:                      # a new document ranks first: a filter that lets it through must show it
            self.order.insert(0, self.num_docs)
            self.scores.append(self.scores[-1] * 0.5)
            self.num_docs += 1
        self.generation += 1

    def remove(self, rows):
        gone = sorted(int(r) for r in rows)
        kept = [r for r in self.order if r not in gone]
        self.order = [r - sum(g < r for g in gone) for r in kept]
        self.scores = self.scores[:len(self.order)]
        self.num_docs = len(self.order)
        self.generation += 1


class IdsOnlyBm25:
    exact_prefix = filtered_prefix = True

    def __init__(self, order, scores):
        self.order, self.scores, self.calls = list(order), list(scores), []

    def invoke(self, query, k, **kw):
        self.calls.append((query, k, dict(kw)))
        allow = None if kw.get("subset") is None else set(np.asarray(kw["subset"]).tolist())
        kept = [(r, s) for r, s in zip(self.order, self.scores) if allow is None or r in allow][:k]
        return [r for r, _ in kept], [s for _, s in kept]


def _ensemble(seed=3, bm=LiveBm25, dense=LiveDense, **kw):
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, emb, order, scores, queries = _world(seed)
    ts = Store(titles, [None] * len(titles), t_emb.tolist())
    e = EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=bm(order, scores), retriever_cls=dense,
                          prefetch_documents=True, **kw)
    counted = {"rows_where": 0}
    inner = e.rows_where

    def rows_where(where):
        counted["rows_where"] += 1
        return inner(where)

    e.rows_where = rows_where
    return e, counted, queries, base


WHERE = {"company": ["zeekr", "lotus"], "year": (2021, 2023)}


@pytest.mark.parametrize("mode", ["corpus", "subset"])
def test_a_prepared_where_reaches_both_legs_as_the_prepared_objects_and_looks_the_rows_up_once(mode):
    e, counted, queries, _ = _ensemble(where_statistics=mode)
    want = [e.invoke(q, h, where=WHERE) for q, h in queries]
    assert counted["rows_where"] == len(queries)
    counted["rows_where"] = 0
    dense, bm = e.faiss_retriever, e.bm25_retriever
    pw = e.prepare_where(WHERE)
    assert counted["rows_where"] == 1 and pw.where == WHERE
    keep = [i for i, md in enumerate(e.chunk_metadata) if _passes(md, WHERE)]
    assert pw.passing.tolist() == keep and pw.allow == set(keep)
    assert pw.dense is dense.index.made[-1] and pw.dense.ids.tolist() == keep
    assert pw.bm25 is bm.prepared[-1] and pw.bm25.rows.tolist() == keep and pw.bm25.stats == mode
    n_dense, n_bm = len(dense.got), len(bm.calls)
    got = [e.invoke(q, h, where=pw) for q, h in queries]
    assert got == want
    assert counted["rows_where"] == 1, "the rows are the prepared object's own"
    assert all(s is pw.dense for s in dense.got[n_dense:]) and len(dense.got) - n_dense == len(queries)
    assert all(c[2] == {"subset": pw.bm25} for c in bm.calls[n_bm:]) and len(bm.calls) - n_bm == len(queries)
    assert len(dense.index.made) == 1 and len(bm.prepared) == 1
    assert [e.invoke(q, h, where=dict(WHERE)) for q, h in queries] == want      # a dict still works as it did
    pw.close()
    assert bm.prepared[-1].closed and pw.dense is None
    pw.close()
    with pytest.raises(ValueError, match="closed"):
        e.invoke("q0", [], where=pw)


@pytest.mark.parametrize("mode", ["corpus", "subset"])
def test_after_an_update_the_next_invoke_prepares_again_and_equals_the_dict_form(mode):
    e, counted, queries, base = _ensemble(where_statistics=mode)
    bm = e.bm25_retriever
    with e.prepare_where(WHERE) as pw:
        first = pw.bm25
        before = [e.invoke(q, h, where=pw) for q, h in queries]
        n = e.num_chunk
        new_md = [{"doc_id": f"new{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": "title 0\nline", "company": c, "year": 2021}
                  for i, c in enumerate(("zeekr", "polestar", "lotus"))]
        rows = e.add_documents([f"new text {i}" for i in range(3)], new_md, embeddings=base[:3] * 1.5)
        assert rows == [n, n + 1, n + 2] and counted["rows_where"] == 1
        with pytest.raises(ValueError, match="prepare_subset again"):
            bm.invoke("q0", 3, subset=first)                       # the lower-level object holds rows: it stays stale
        got = [e.invoke(q, h, where=pw) for q, h in queries]
        assert counted["rows_where"] == 2 and first.closed and pw.bm25 is bm.prepared[-1] and pw.bm25 is not first
        assert pw.passing.tolist()[-2:] == [n, n + 2] and len(e.faiss_retriever.index.made) == 2
        want = [e.invoke(q, h, where=dict(WHERE)) for q, h in queries]
        assert got == want and got != before
        assert any(d["metadata"]["doc_id"] == "new0" for out in got for d in out)
        removed = e.remove_documents(["d5", "new0"])
        assert removed == 2
        got = [e.invoke(q, h, where=pw) for q, h in queries]
        assert counted["rows_where"] == 2 + len(queries) + 1 and len(bm.prepared) == 3
        assert got == [e.invoke(q, h, where=dict(WHERE)) for q, h in queries]
        assert not any(d["metadata"]["doc_id"] in ("d5", "new0") for out in got for d in out)
    assert bm.prepared[-1].closed


def test_legs_that_offer_neither_call_get_the_ids():
    e, counted, queries, _ = _ensemble(bm=IdsOnlyBm25, dense=SubsetCosineRetriever)
    want = [e.invoke(q, h, where=WHERE) for q, h in queries]
    pw = e.prepare_where(WHERE)
    n_bm = len(e.bm25_retriever.calls)
    assert [e.invoke(q, h, where=pw) for q, h in queries] == want
    assert isinstance(pw.dense, np.ndarray) and isinstance(pw.bm25, np.ndarray)
    assert all(np.array_equal(s, pw.passing) for s in e.faiss_retriever.subsets[-len(queries):])
    assert all(np.array_equal(c[2]["subset"], pw.passing) and "stats" not in c[2] for c in e.bm25_retriever.calls[n_bm:])
    pw.close()


def test_a_filter_nothing_passes_prepares_no_device_object_and_returns_nothing():
    e, _, queries, _ = _ensemble()
    pw = e.prepare_where({"company": "nobody"})
    assert pw.passing.size == 0 and not e.bm25_retriever.prepared and not e.faiss_retriever.index.made
    assert e.invoke(*queries[0], where=pw) == []


def test_refusals():
    e, _, queries, _ = _ensemble()
    other, _, _, _ = _ensemble()
    pw = other.prepare_where(WHERE)
    with pytest.raises(ValueError, match="another EnsembleRetriever"):
        e.invoke(*queries[0], where=pw)
    with pytest.raises(TypeError):
        e.prepare_where([("company", "zeekr")])
    assert other.invoke(*queries[0], where=pw) == other.invoke(*queries[0], where=WHERE)
