"""``EnsembleRetriever(..., where_statistics=)``: which call the BM25 leg of a filtered request receives.  CPU-only, with stub
retrievers that record their calls (the GPU retriever's ``stats="subset"`` is held to numpy in tests/test_gpu_bm25_substats.py).

"subset" passes ``stats="subset"`` and ``subset=<the passing rows>``; the default makes exactly the calls made before the keyword
existed; a retriever that does not declare ``subset_statistics`` is refused at construction, as is an unknown value."""
import numpy as np
import pytest

from test_ensemble_where import Store, SubsetCosineRetriever, _passes, _world


class Recorder:
    """A BM25 retriever that filters on its own: returns the first k rows of a fixed ranking that ``subset`` allows, and records
    every call's positional and keyword arguments."""
    exact_prefix = True
    filtered_prefix = True

    def __init__(self, order, scores):
        self.order, self.scores, self.calls = list(order), list(scores), []

    def invoke(self, query, k, **kw):
        self.calls.append((query, k, {key: (np.asarray(v).tolist() if key == "subset" else v) for key, v in kw.items()}))
        allow = None if kw.get("subset") is None else set(np.asarray(kw["subset"]).tolist())
        kept = [(r, s) for r, s in zip(self.order, self.scores) if allow is None or r in allow][:k]
        return [r for r, _ in kept], [s for _, s in kept]


class Declares(Recorder):
    subset_statistics = True


def _ensemble(bm, **kw):
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, emb, order, scores, queries = _world(2, bundles=False)
    ts = Store(titles, [None] * len(titles), t_emb.tolist())
    e = EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=bm(order, scores),
                          retriever_cls=SubsetCosineRetriever, faiss_k=0, faiss_ts_k=0, bm25_k=7, **kw)
    return e, metas, queries


WHERE = {"company": "other", "year": [2021, 2022]}


def test_subset_passes_stats_and_the_passing_rows():
    e, metas, queries = _ensemble(Declares, where_statistics="subset")
    keep = [i for i, md in enumerate(metas) if _passes(md, WHERE)]
    assert len(keep) > 7
    got = e.invoke(queries[0][0], [], where=WHERE)
    assert e.bm25_retriever.calls == [(queries[0][0], 7, {"subset": keep, "stats": "subset"})]
    assert len(got) == 7 and all(c["retriever"] == "BM25" and _passes(c["metadata"], WHERE) for c in got)
    e.bm25_retriever.calls.clear()
    e.invoke(queries[0][0], [])                                   # no filter: no statistics to choose
    assert e.bm25_retriever.calls == [(queries[0][0], 7, {})]


@pytest.mark.parametrize("kw", [{}, {"where_statistics": "corpus"}], ids=["default", "corpus"])
def test_the_default_makes_todays_calls(kw):
    for bm in (Recorder, Declares):
        e, metas, queries = _ensemble(bm, **kw)
        keep = [i for i, md in enumerate(metas) if _passes(md, WHERE)]
        e.invoke(queries[0][0], [], where=WHERE)
        e.invoke(queries[0][0], [])
        assert e.bm25_retriever.calls == [(queries[0][0], 7, {"subset": keep}), (queries[0][0], 7, {})]


def test_a_retriever_without_subset_statistics_and_an_unknown_value_are_refused_at_construction():
    with pytest.raises(ValueError, match="subset_statistics"):
        _ensemble(Recorder, where_statistics="subset")
    with pytest.raises(ValueError, match="where_statistics"):
        _ensemble(Declares, where_statistics="company")
