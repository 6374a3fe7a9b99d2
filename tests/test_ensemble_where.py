"""``EnsembleRetriever.invoke(input, hyde_chunks, where=...)``: the result is what ``invoke`` returns over a store that holds the
passing chunks alone.  CPU-only: the dense retriever is an injected numpy one that honours ``subset=`` by scoring the listed rows
only (the GPU FaissRetriever's ``subset=`` is held to the oracle in tests/test_gpu_subset_search.py).

The reduced store is built by deleting the failing chunks: rows renumber, neighbour ids that now point nowhere stay in the metadata,
bundles lose their failing rows.  The one stated exception is the BM25 leg -- whole-corpus statistics -- so the reduced store's BM25
object returns the FULL ranking filtered and renumbered, which is also what the filtered call must use."""
import numpy as np
import pytest

COMPANIES = ("zeekr", "lotus", "other")


class Store:
    """Chroma-shaped store: get(include=[...]) returns everything, get(ids=[...]) the requested rows in order."""

    def __init__(self, docs, metas, embs):
        self.docs, self.metas, self.embs = docs, metas, embs
        self.by_id = {m["doc_id"]: i for i, m in enumerate(metas)} if metas and metas[0] else {}

    def get(self, ids=None, include=()):
        if ids is None:
            return {"documents": self.docs, "metadatas": self.metas, "embeddings": self.embs}
        rows = [self.by_id[i] for i in ids]
        return {"documents": [self.docs[r] for r in rows], "metadatas": [self.metas[r] for r in rows]}


class SubsetCosineRetriever:
    """Stands in for FaissRetriever: exact cosine, best first, ties to the lower id; ``subset`` = the only rows that are scored."""

    def __init__(self, embeddings, embedding_fn):
        x = np.asarray(embeddings, np.float32)
        self.x = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
        self.fn = embedding_fn
        self.subsets = []

    def invoke(self, querys, k, subset=None):
        self.subsets.append(None if subset is None else np.asarray(subset).copy())
        rows = np.arange(self.x.shape[0]) if subset is None else np.asarray(subset, dtype=np.int64)
        q = np.asarray([self.fn.embed_query(s) for s in querys], np.float32)
        q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-30)
        ids = np.full((len(querys), k), -1, np.int64)
        sc = np.full((len(querys), k), -np.finfo(np.float32).max, np.float32)
        for i in range(len(querys)):
            sim = np.asarray([np.dot(q[i], self.x[r]) for r in rows], np.float32)   # one row at a time: no other row's presence matters
            o = np.lexsort((rows, -sim))[:k]
            ids[i, :len(o)], sc[i, :len(o)] = rows[o], sim[o]
        return ids, sc


class Emb:
    def __init__(self, table):
        self.table = table

    def embed_query(self, text):
        return self.table[text]


class Bm25:
    def __init__(self, order, scores):
        self.order, self.scores, self.asked = list(order), list(scores), []

    def invoke(self, query, k):
        self.asked.append(k)
        return self.order[:k], self.scores[:k]


def _world(seed, n=240, d=24, n_titles=12, bundles=True):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, d)).astype(np.float32)
    for i in range(1, n):       # chains of neighbouring chunks whose embeddings drift slowly: neighbours score high together
        if i % 8:
            base[i] = 0.93 * base[i - 1] + 0.37 * base[i]
    metas, docs = [], []
    for i in range(n):
        first, last = i % 8 == 0, i % 8 == 7
        md = {"doc_id": f"d{i}", "prev_chunk_id": "" if first else f"d{i - 1}", "next_chunk_id": "" if last else f"d{i + 1}",
              "title_summary": f"title {i // (n // n_titles)}\nline", "company": COMPANIES[(i // 3) % 3], "year": 2020 + (i // 16) % 5}
        if bundles and i % 5 in (0, 1, 2):   # three-row bundles: a company boundary (every 3 rows) cuts through many of them
            md["bundle_id"] = f"b{i // 5}"
        if i % 7 == 0:
            md["tags"] = ["a", "b"]            # an unhashable value: no filter value equals it
        metas.append(md)
        docs.append(f"text of chunk {i}")
    titles = [f"title {t}\nline" for t in range(n_titles)] + ["title nobody has"]
    t_emb = rng.standard_normal((len(titles), d)).astype(np.float32)
    table, queries = {}, []
    for j, anchor in enumerate((3, 42, 100, 77, 199, 238)):
        table[f"q{j}"] = (base[anchor] + 0.05 * rng.standard_normal(d).astype(np.float32)).tolist()
        table[f"h{j}"] = (base[(anchor + 2) % n] + 0.05 * rng.standard_normal(d).astype(np.float32)).tolist()
        queries.append((f"q{j}", [f"h{j}"] if j % 2 else []))
    order = rng.permutation(n).tolist()
    scores = np.sort(rng.random(n).astype(np.float32))[::-1].tolist()
    return docs, metas, base, titles, t_emb, Emb(table), order, scores, queries


def _passes(md, where):
    for field, want in where.items():
        values = list(want) if isinstance(want, (list, tuple, set, frozenset)) else [want]
        v = md.get(field, None)
        if isinstance(v, list) or v not in values:
            return False
    return True


def _pair(world, where, **kw):
    """(the retriever over the full store, the one over the store of the passing chunks alone, the passing rows)"""
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, emb, order, scores, _ = world
    keep = [i for i, md in enumerate(metas) if _passes(md, where)]
    new_row = {r: j for j, r in enumerate(keep)}
    ts = Store(titles, [None] * len(titles), t_emb.tolist())
    full = EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=Bm25(order, scores),
                             retriever_cls=SubsetCosineRetriever, **kw)
    kept = [(new_row[r], s) for r, s in zip(order, scores) if r in new_row]
    small = None if not keep else EnsembleRetriever("unused", Store([docs[i] for i in keep], [metas[i] for i in keep], base[keep].tolist()), ts, 6, emb,
                              bm25_retriever=Bm25([r for r, _ in kept], [s for _, s in kept]), retriever_cls=SubsetCosineRetriever, **kw)
    return full, small, keep


WHERES = ({"company": "zeekr"}, {"company": ["zeekr", "lotus"], "year": 2023}, {"year": (2021, 2024)}, {"company": "lotus", "year": [2020]})


@pytest.mark.parametrize("where", WHERES, ids=[str(i) for i in range(len(WHERES))])
@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("expand", [False, True])
def test_where_is_the_store_of_the_passing_chunks(expand, prefetch, where):
    world = _world(0)
    full, small, keep = _pair(world, where, faiss_ts_k=2, bm25_k=5, enable_expand=expand, prefetch_documents=prefetch)
    assert 0 < len(keep) < len(world[1])
    emitted, multi, grown = 0, 0, 0
    for q, hyde in world[8]:
        got, want = full.invoke(q, hyde, where=where), small.invoke(q, hyde)
        assert got == want, (q, where)
        assert all(_passes(c["metadata"], where) for c in got)
        emitted += len(got)
        sizes = {}
        for c in got:
            sizes[c["bundle_id"]] = sizes.get(c["bundle_id"], 0) + 1
        multi += sum(1 for v in sizes.values() if v > 1)
        unfiltered = full.invoke(q, hyde)
        grown += sum(1 for c in unfiltered if not _passes(c["metadata"], where))
    assert emitted > 0 and multi > 0, "the cases must emit bundles of several rows"
    assert grown > 0, "the unfiltered call must reach chunks the filter hides, or the filter shows nothing"
    # the dense leg searched the passing rows alone; the title leg's retriever (over the title store) was not filtered
    assert all(s is not None and np.array_equal(s, keep) for s in full.faiss_retriever.subsets[::2])
    assert all(s is None for s in full.title_summary_faiss_retriever.subsets)


def test_expansion_stops_at_the_filters_edge():
    """With neighbour expansion on, a hit's chain grows over passing neighbours only: every emitted chunk passes, and some chain
    of the unfiltered call is longer than the filtered one's (it crossed an edge the filter closes)."""
    world = _world(1)
    where = {"company": ["zeekr", "lotus"]}
    full, small, keep = _pair(world, where, faiss_ts_k=0, bm25_k=0, enable_expand=True)
    crossed = 0
    for q, hyde in world[8]:
        got = full.invoke(q, hyde, where=where)
        assert got == small.invoke(q, hyde)
        free = full.invoke(q, hyde)
        crossed += sum(1 for c in free if not _passes(c["metadata"], where))
    assert crossed > 0


def test_bm25_leg_is_the_full_ranking_filtered():
    world = _world(2, bundles=False)
    docs, metas, base, titles, t_emb, emb, order, scores, queries = world
    where = {"company": "other", "year": [2021, 2022]}
    full, small, keep = _pair(world, where, faiss_k=0, faiss_ts_k=0, bm25_k=7)
    got = full.invoke(queries[0][0], [], where=where)
    want_rows = [r for r in order if r in set(keep)][:7]
    assert [c["metadata"]["doc_id"] for c in got] == [f"d{r}" for r in want_rows]
    assert [c["score"] for c in got] == [float(scores[order.index(r)]) for r in want_rows]
    assert all(c["retriever"] == "BM25" for c in got)
    assert full.bm25_retriever.asked == [len(metas)], "the leg is asked for the full ranking"
    assert got == small.invoke(queries[0][0], [])


@pytest.mark.parametrize("expand", [False, True])
def test_where_matching_everything_is_the_unfiltered_call(expand):
    world = _world(3)
    full, _, keep = _pair(world, {"company": list(COMPANIES)}, faiss_ts_k=2, bm25_k=5, enable_expand=expand)
    assert len(keep) == len(world[1])
    for q, hyde in world[8]:
        assert full.invoke(q, hyde, where={"company": list(COMPANIES)}) == full.invoke(q, hyde)
        assert full.invoke(q, hyde, where={}) == full.invoke(q, hyde)
        assert full.invoke(q, hyde, where=None) == full.invoke(q, hyde)


def test_where_matching_nothing_returns_nothing():
    world = _world(4)
    full, _, keep = _pair(world, {"company": "nobody"}, faiss_ts_k=2, bm25_k=5)
    assert keep == []
    assert full.invoke(world[8][0][0], [], where={"company": "nobody"}) == []
