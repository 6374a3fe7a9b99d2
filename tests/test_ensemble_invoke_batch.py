"""``EnsembleRetriever.invoke_batch(inputs, hyde_chunks_list, wheres)`` equals ``[invoke(inputs[i], hyde_chunks_list[i], where=wheres[i])]``
as Python objects, and asks each leg ONCE for the whole batch where the leg can take a filter per query.  CPU-only, with the stand-in
retrievers of tests/test_ensemble_where.py and tests/test_ensemble_prepared_where.py (the GPU objects are held to the same equality
in tests/test_gpu_subset_multi.py).

Three tenants (the ``company`` field of the world), wheres all None / all dicts / all ``PreparedWhere`` / mixed with one that passes
nothing, both ``where_statistics`` modes, ``enable_expand`` on and off.  The legs' calls are counted on the fakes."""
import numpy as np
import pytest

from test_ensemble_prepared_where import FakeBm25Subset, FakeRowSubset, IdsOnlyBm25, LiveBm25, LiveDense
from test_ensemble_where import COMPANIES, Store, SubsetCosineRetriever, _world


class BatchDense(LiveDense):
    """The cosine stand-in that declares ``per_query_subsets``: ``subsets=`` is one filter per string, row i the one-filter answer."""
    per_query_subsets = True

    def __init__(self, embeddings, embedding_fn):
        super().__init__(embeddings, embedding_fn)
        self.batch_calls = []

    def invoke(self, querys, k, subset=None, subsets=None):
        if subsets is None:
            return super().invoke(querys, k, subset=subset)
        assert subset is None and len(subsets) == len(querys)
        self.batch_calls.append(list(subsets))
        ids, sc = [], []
        for s, sub in zip(querys, subsets):
            i, c = SubsetCosineRetriever.invoke(self, [s], k, subset=sub.ids if isinstance(sub, FakeRowSubset) else sub)
            ids.append(i[0])
            sc.append(c[0])
        return np.stack(ids), np.stack(sc)


class BatchBm25(LiveBm25):
    """The live BM25 stand-in with ``invoke_batch(queries, k, subsets=[prepared object or None])``: min(k, rows allowed) rows per query."""

    def __init__(self, order, scores):
        super().__init__(order, scores)
        self.batch_calls = []

    def invoke_batch(self, queries, k, subsets=None):
        self.batch_calls.append((list(queries), k, list(subsets)))
        out = []
        for q, s in zip(queries, subsets):
            assert s is None or isinstance(s, FakeBm25Subset)
            if s is not None and (s.closed or s.generation != self.generation):
                raise ValueError("stale or closed: call prepare_subset again")
            allow = None if s is None else set(s.rows.tolist())
            kept = [(r, sc) for r, sc in zip(self.order, self.scores) if allow is None or r in allow][:k]
            out.append(([r for r, _ in kept], [sc for _, sc in kept]))
        return out


def _ensemble(bm=BatchBm25, dense=BatchDense, **kw):
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, emb, order, scores, queries = _world(5)
    ts = Store(titles, [None] * len(titles), t_emb.tolist())
    e = EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=bm(order, scores), retriever_cls=dense,
                          prefetch_documents=True, faiss_ts_k=2, bm25_k=5, **kw)
    return e, queries, base


TENANTS = [{"company": c} for c in COMPANIES]                                     # three tenants
NOTHING = {"company": "nobody"}


def _wheres(kind, e, n):
    """(wheres for invoke_batch, the PreparedWheres to close)"""
    if kind == "none":
        return [None] * n, []
    if kind == "dicts":
        return [dict(TENANTS[i % 3]) for i in range(n)], []                       # equal content in different objects
    if kind == "prepared":
        pws = [e.prepare_where(w) for w in TENANTS]
        return [pws[i % 3] for i in range(n)], pws
    pw = e.prepare_where(TENANTS[1])
    mix = [None, dict(TENANTS[0]), pw, dict(NOTHING), {"company": ["zeekr", "lotus"], "year": (2021, 2023)}, pw]
    return [mix[i % len(mix)] for i in range(n)], [pw]


@pytest.mark.parametrize("expand", [False, True])
@pytest.mark.parametrize("mode", ["corpus", "subset"])
@pytest.mark.parametrize("kind", ["none", "dicts", "prepared", "mixed"])
def test_invoke_batch_equals_invoke_and_asks_each_leg_once(kind, mode, expand):
    e, queries, _ = _ensemble(where_statistics=mode, enable_expand=expand)
    inputs, hyde = [q for q, _ in queries], [h for _, h in queries]
    wheres, pws = _wheres(kind, e, len(queries))
    want = [e.invoke(q, h, where=w) for q, h, w in zip(inputs, hyde, wheres)]
    assert sum(len(o) for o in want) > 0
    dense, title, bm = e.faiss_retriever, e.title_summary_faiss_retriever, e.bm25_retriever
    n_dense, n_title, n_bm, n_prepared = len(dense.got), len(title.got), len(bm.calls), len(bm.prepared)
    got = e.invoke_batch(inputs, hyde, wheres)
    assert got == want
    live = [i for i, w in enumerate(wheres) if not (isinstance(w, dict) and w == NOTHING)]
    # the dense leg: ONE call, one filter per string of every live request; strings of one request share their filter object
    assert len(dense.batch_calls) == 1 and len(dense.got) == n_dense
    filters = dense.batch_calls[0]
    assert len(filters) == sum(1 + len(hyde[i]) for i in live)
    at = 0
    for i in live:
        mine = filters[at:at + 1 + len(hyde[i])]
        at += len(mine)
        assert all(f is mine[0] for f in mine)
        assert (mine[0] is None) == (wheres[i] is None)
        if isinstance(wheres[i], type(pws[0]) if pws else ()):
            assert mine[0] is wheres[i].dense
    # the title leg: one call for the live requests, never filtered
    assert len(title.got) == n_title + 1 and title.got[-1] is None and len(title.batch_calls) == 0
    # the BM25 leg: ONE invoke_batch, a prepared object or None per live request; no per-request call
    assert len(bm.batch_calls) == 1 and len(bm.calls) == n_bm
    asked, k, subsets = bm.batch_calls[0]
    assert asked == [inputs[i] for i in live] and k == 5 and len(subsets) == len(live)
    for j, i in enumerate(live):
        assert (subsets[j] is None) == (wheres[i] is None)
        if subsets[j] is not None:
            assert isinstance(subsets[j], FakeBm25Subset) and subsets[j].stats == mode
    # dicts of equal content share one preparation, released when the call ends; a caller's PreparedWhere stays open
    made = bm.prepared[n_prepared:]
    if kind == "dicts":
        assert len(made) == 3 and all(p.closed for p in made)
        assert filters[0] is filters[sum(1 + len(hyde[i]) for i in live[:3])], "requests 0 and 3 are the same tenant: one list"
    if kind == "mixed":
        assert len(made) == 2 and all(p.closed for p in made)                     # the two non-empty dicts; NOTHING prepares no object
    assert all(not pw.bm25.closed for pw in pws)
    for pw in pws:
        pw.close()


def test_a_request_whose_filter_passes_nothing_yields_nothing_and_an_all_empty_batch_asks_no_leg():
    e, queries, _ = _ensemble()
    inputs, hyde = [q for q, _ in queries[:3]], [h for _, h in queries[:3]]
    assert e.invoke_batch(inputs, hyde, [dict(NOTHING)] * 3) == [[], [], []]
    assert not e.faiss_retriever.batch_calls and not e.bm25_retriever.batch_calls and not e.title_summary_faiss_retriever.got
    assert e.invoke_batch([], []) == []


@pytest.mark.parametrize("mode", ["corpus", "subset"])
def test_legs_without_the_per_query_calls_are_asked_once_per_request(mode):
    bm = LiveBm25 if mode == "subset" else IdsOnlyBm25
    e, queries, _ = _ensemble(bm=bm, dense=LiveDense, where_statistics=mode)
    inputs, hyde = [q for q, _ in queries], [h for _, h in queries]
    pw = e.prepare_where(TENANTS[2])
    wheres = [None, dict(TENANTS[0]), pw, dict(TENANTS[0]), None, dict(NOTHING)]
    want = [e.invoke(q, h, where=w) for q, h, w in zip(inputs, hyde, wheres)]
    n_dense, n_bm = len(e.faiss_retriever.got), len(e.bm25_retriever.calls)
    assert e.invoke_batch(inputs, hyde, wheres) == want
    assert len(e.faiss_retriever.got) - n_dense == 5 and len(e.bm25_retriever.calls) - n_bm == 5      # the five live requests
    assert len(e.title_summary_faiss_retriever.got) >= 1
    pw.close()


def test_a_prepared_where_inside_a_batch_prepares_again_after_add_documents():
    e, queries, base = _ensemble()
    inputs, hyde = [q for q, _ in queries], [h for _, h in queries]
    with e.prepare_where(TENANTS[0]) as pw:
        wheres = [pw, None, dict(TENANTS[1])] * 2
        before = e.invoke_batch(inputs, hyde, wheres)
        first, n = pw.bm25, e.num_chunk
        new_md = [{"doc_id": f"new{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": "title 0\nline", "company": c, "year": 2021}
                  for i, c in enumerate(("zeekr", "other"))]
        assert e.add_documents(["new text 0", "new text 1"], new_md, embeddings=base[:2] * 1.5) == [n, n + 1]
        got = e.invoke_batch(inputs, hyde, wheres)
        assert first.closed and pw.bm25 is not first and pw.passing.tolist()[-1] == n
        assert got == [e.invoke(q, h, where=w) for q, h, w in zip(inputs, hyde, wheres)] and got != before
        assert any(d["metadata"]["doc_id"] == "new0" for d in got[0] + got[3])


def test_refusals_and_stage_brackets():
    import veritasfi_amd
    from veritasfi_amd import stages
    e, queries, _ = _ensemble()
    inputs, hyde = [q for q, _ in queries], [h for _, h in queries]
    with pytest.raises(ValueError, match="5 wheres for 6 inputs"):
        e.invoke_batch(inputs, hyde, [None] * 5)
    with pytest.raises(ValueError, match="hyde chunk lists"):
        e.invoke_batch(inputs, hyde[:2])
    with pytest.raises(TypeError, match="None, a dict"):
        e.invoke_batch(inputs, hyde, [["company", "zeekr"]] + [None] * 5)

    prof = stages.StageTimer()
    prev = veritasfi_amd.set_profiler(prof)
    try:
        outs = e.invoke_batch(inputs, hyde, [dict(TENANTS[i % 3]) for i in range(6)])
    finally:
        veritasfi_amd.set_profiler(prev)
    assert prof.profile_data["retrieve"]["calls"] == 1
    assert prof.metrics["retrieved_chunks"] == [len(o) for o in outs]
