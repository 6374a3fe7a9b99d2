"""``EnsembleRetriever`` under the operator grammar of ``where`` (``$eq $ne $gt $gte $lt $lte $in $nin $and $or``), CPU-only: the stand-ins
of tests/test_ensemble_where.py have no device, so every filter here takes the NumPy route (``WhereProgram.evaluate_numpy``); the device
route is held to the same rule in tests/test_gpu_where.py.

The rule is the one ``invoke(..., where=)`` always had: the output is what ``invoke`` returns over a store of the passing chunks alone --
now with "passing" defined by ``where.matches``.  The ``PreparedWhere`` and ``invoke_batch`` forms give the same output and prepare again
after ``add_documents`` / ``remove_documents``; a filter on a field of list values raises the kind error on every route; a plain dict
(no ``$`` key) never reaches the new module."""
import numpy as np
import pytest

from test_ensemble_prepared_where import LiveBm25, LiveDense
from test_ensemble_where import WHERES, Bm25, Store, SubsetCosineRetriever, _world
from veritasfi_amd import where as W

OPERATOR_WHERES = (
    {"year": {"$gte": 2021, "$lt": 2024}},
    {"$or": [{"company": "zeekr"}, {"year": {"$gt": 2023}}]},
    {"company": {"$ne": "lotus"}, "year": {"$in": [2020, 2022]}},
    {"missing": {"$ne": 1}},
)
IDS = [str(i) for i in range(len(OPERATOR_WHERES))]


def _pair(world, where, **kw):
    """(the retriever over the full store, the one over the store of the passing chunks alone, the passing rows) -- tests/test_ensemble_where.py's
    pair, with ``where.matches`` deciding what passes."""
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, emb, order, scores, _ = world
    keep = [i for i, md in enumerate(metas) if W.matches(md, where)]
    new_row = {r: j for j, r in enumerate(keep)}
    ts = Store(titles, [None] * len(titles), t_emb.tolist())
    full = EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=Bm25(order, scores),
                             retriever_cls=SubsetCosineRetriever, **kw)
    kept = [(new_row[r], s) for r, s in zip(order, scores) if r in new_row]
    small = EnsembleRetriever("unused", Store([docs[i] for i in keep], [metas[i] for i in keep], base[keep].tolist()), ts, 6, emb,
                              bm25_retriever=Bm25([r for r, _ in kept], [s for _, s in kept]), retriever_cls=SubsetCosineRetriever, **kw)
    return full, small, keep


@pytest.mark.parametrize("where", OPERATOR_WHERES, ids=IDS)
@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("expand", [False, True])
def test_operator_where_is_the_store_of_the_passing_chunks(expand, prefetch, where):
    world = _world(0)
    full, small, keep = _pair(world, where, faiss_ts_k=2, bm25_k=5, enable_expand=expand, prefetch_documents=prefetch)
    n = len(world[1])
    assert (len(keep) == n) if "missing" in where else (0 < len(keep) < n)
    rows = full.rows_where(where)
    assert rows.dtype == np.int64 and rows.tolist() == keep
    emitted, hidden = 0, 0
    for q, hyde in world[8]:
        got, want = full.invoke(q, hyde, where=where), small.invoke(q, hyde)
        assert got == want, (q, where)
        assert all(W.matches(c["metadata"], where) for c in got)
        emitted += len(got)
        hidden += sum(1 for c in full.invoke(q, hyde) if not W.matches(c["metadata"], where))
    assert emitted > 0
    assert hidden > 0 or len(keep) == n, "the unfiltered call must reach chunks the filter hides, or the filter shows nothing"
    assert all(s is not None and np.array_equal(s, keep) for s in full.faiss_retriever.subsets[::2][:len(world[8])])


def _live(seed=3, **kw):
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, emb, order, scores, queries = _world(seed)
    ts = Store(titles, [None] * len(titles), t_emb.tolist())
    e = EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=LiveBm25(order, scores), retriever_cls=LiveDense,
                          prefetch_documents=True, **kw)
    counted = {"evaluations": 0}
    inner = e._eval_where

    def _eval_where(where):
        counted["evaluations"] += 1
        return inner(where)

    e._eval_where = _eval_where
    return e, counted, queries, base


@pytest.mark.parametrize("where", OPERATOR_WHERES, ids=IDS)
def test_prepared_and_batched_forms_agree_and_prepare_again_after_a_change(where):
    e, counted, queries, base = _live()
    want = [e.invoke(q, h, where=where) for q, h in queries]
    assert counted["evaluations"] == len(queries) and any(want)
    counted["evaluations"] = 0
    keep = [i for i, md in enumerate(e.chunk_metadata) if W.matches(md, where)]
    with e.prepare_where(where) as pw:
        assert counted["evaluations"] == 1
        assert pw.passing.tolist() == keep and isinstance(pw.allow, W.RowMask) and list(pw.allow) == keep and len(pw.allow) == len(keep)
        assert -1 not in pw.allow and e.num_chunk not in pw.allow
        assert pw.dense is e.faiss_retriever.index.made[-1] and pw.bm25 is e.bm25_retriever.prepared[-1] and pw.bm25.rows.tolist() == keep
        assert [e.invoke(q, h, where=pw) for q, h in queries] == want
        assert counted["evaluations"] == 1, "the rows are the prepared object's own"
        # the batch: dicts of equal content share ONE evaluation, a PreparedWhere none
        copies = [dict(where) if i % 2 else {k: (dict(v) if isinstance(v, dict) else list(v) if isinstance(v, list) else v) for k, v in where.items()}
                  for i in range(len(queries))]
        got = e.invoke_batch([q for q, _ in queries], [h for _, h in queries], wheres=copies)
        assert got == want and counted["evaluations"] == 2
        mixed = [pw if i % 2 else None for i in range(len(queries))]
        got = e.invoke_batch([q for q, _ in queries], [h for _, h in queries], wheres=mixed)
        assert got == [w if i % 2 else e.invoke(q, h) for i, (w, (q, h)) in enumerate(zip(want, queries))] and counted["evaluations"] == 2
        # a change of the corpus: the next use prepares again, from the dict
        n = e.num_chunk
        first = pw.bm25
        new_md = [{"doc_id": f"new{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": "title 0\nline", "company": c, "year": y}
                  for i, (c, y) in enumerate((("zeekr", 2022), ("polestar", 2025), ("lotus", 2019)))]
        assert e.add_documents([f"new text {i}" for i in range(3)], new_md, embeddings=base[:3] * 1.5) == [n, n + 1, n + 2]
        assert e._where_columns == {}, "the columns go where the per-field dictionaries go"
        got = [e.invoke(q, h, where=pw) for q, h in queries]
        assert counted["evaluations"] == 3 and first.closed and pw.bm25 is not first
        keep = [i for i, md in enumerate(e.chunk_metadata) if W.matches(md, where)]
        assert pw.passing.tolist() == keep and any(r >= n for r in keep)
        assert got == [e.invoke(q, h, where=dict(where)) for q, h in queries] and got != want
        assert e.remove_documents(["d5", "new0"]) == 2 and e._where_columns == {}
        got = [e.invoke(q, h, where=pw) for q, h in queries]
        keep = [i for i, md in enumerate(e.chunk_metadata) if W.matches(md, where)]
        assert pw.passing.tolist() == keep and e.rows_where(where).tolist() == keep
        assert got == [e.invoke(q, h, where=dict(where)) for q, h in queries]
        assert not any(d["metadata"]["doc_id"] in ("d5", "new0") for out in got for d in out)
    assert e.bm25_retriever.prepared[-1].closed


def test_a_filter_on_list_values_raises_the_kind_error_on_every_route():
    e, _, queries, _ = _live()
    where = {"tags": {"$in": ["a"]}}
    q, h = queries[0]
    for call in (lambda: e.rows_where(where), lambda: e.invoke(q, h, where=where), lambda: e.prepare_where(where),
                 lambda: e.invoke_batch([q], [h], wheres=[where]), lambda: e.rows_where({"$or": [{"year": 2020}, {"tags": {"$ne": "a"}}]})):
        with pytest.raises(ValueError, match=r"field 'tags' holds values of kinds \['list'\]"):
            call()
    with pytest.raises(ValueError, match="field 'year' is of kind int, the \\$gt value '2020' is of kind str"):
        e.rows_where({"year": {"$gt": "2020"}})
    with pytest.raises(ValueError, match="unknown operator '\\$between' on field 'year'"):
        e.invoke(q, h, where={"year": {"$between": [1, 2]}})
    assert e.rows_where({"tags": ["a"]}).size == 0, "the plain form keeps its rule: no filter value equals a list"


def test_a_nothing_passing_operator_filter_returns_nothing():
    e, _, queries, _ = _live()
    where = {"year": {"$gt": 2024}}
    assert e.rows_where(where).size == 0 and e.invoke(*queries[0], where=where) == []
    with e.prepare_where(where) as pw:
        assert pw.passing.size == 0 and len(pw.allow) == 0 and not e.bm25_retriever.prepared
        assert e.invoke(*queries[0], where=pw) == []


@pytest.mark.parametrize("where", WHERES, ids=[str(i) for i in range(len(WHERES))])
def test_plain_dicts_never_touch_the_new_module(monkeypatch, where):
    def boom(*a, **kw):
        raise AssertionError("a plain where reached the operator module")
    e, counted, queries, _ = _live()
    for name in ("compile_where", "build_column", "parse", "fields_of", "matches"):
        monkeypatch.setattr(W, name, boom)
    monkeypatch.setattr(W, "RowMask", boom)
    assert W.has_operators(where) is False
    rows = e.rows_where(where)
    with e.prepare_where(where) as pw:
        assert isinstance(pw.allow, set) and pw.allow == set(rows.tolist())
        want = [e.invoke(q, h, where=where) for q, h in queries]
        assert [e.invoke(q, h, where=pw) for q, h in queries] == want
        assert e.invoke_batch([q for q, _ in queries], [h for _, h in queries], wheres=[dict(where)] * len(queries)) == want
    assert counted["evaluations"] == 0 and e._where_columns == {}


def test_where_key_tells_nested_filters_apart():
    from veritasfi_amd.ensemble import EnsembleRetriever
    key = EnsembleRetriever._where_key
    a = {"$or": [{"company": "zeekr"}, {"year": {"$gt": 2023}}], "page": {"$in": [1, 2]}}
    b = {"page": {"$in": [1, 2]}, "$or": [{"company": "zeekr"}, {"year": {"$gt": 2023}}]}
    assert key(a) == key(b) and hash(key(a)) == hash(key(b))
    assert key(a) != key({"$or": [{"year": {"$gt": 2023}}, {"company": "zeekr"}], "page": {"$in": [1, 2]}})
    assert key({"flag": {"$eq": True}}) != key({"flag": {"$eq": 1}}) and key({"x": {"$gt": 1}}) != key({"x": {"$gte": 1}})
    assert key({"company": "zeekr"}) == key({"company": "zeekr"}) and key({"company": ["a", "b"]}) != key({"company": ("a", "b")})
