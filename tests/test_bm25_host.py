"""The BM25 leg's host side (veritasfi_amd/bm25.py): query tokenizer, Lucene index builder, index-directory loader, the C ABI's
entry points, the ensemble's call depth, and the new kernels' register budget.  CPU only."""
import json
import math
import os
import shutil

import numpy as np
import pytest

from veritasfi_amd import bm25 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Suffix:
    """A toy stemmer object with PyStemmer's surface."""

    def stemWords(self, words):
        return [w[:-1] if w.endswith("s") else w for w in words]


def test_tokenizer_lowercases_splits_drops_stopwords_then_stems():
    stem = B.resolve_stemmer(Suffix())
    # one-letter words never match (\w\w+), punctuation splits, stopwords go before the stemmer sees them
    assert B.tokenize("The Cats, and a DOG's toys: x y_z 42!", stem) == ["cat", "dog", "toy", "y_z", "42"]
    assert B.tokenize("The Cats", None) == ["cats"]
    assert B.tokenize("The Cats", B.resolve_stemmer(None), frozenset()) == ["the", "cats"]
    assert B.tokenize("Rivers rivers", B.resolve_stemmer(lambda w: w.upper())) == ["RIVERS", "RIVERS"]
    assert B.tokenize("über Straße", None) == ["über", "straße"]   # (?u): unicode word characters
    assert B.resolve_stopwords("english") is B.STOPWORDS_EN and "the" in B.STOPWORDS_EN and len(B.STOPWORDS_EN) == 33
    assert B.resolve_stopwords(["foo"]) == frozenset({"foo"})
    with pytest.raises(ValueError):
        B.resolve_stopwords("german")
    with pytest.raises(TypeError):
        B.resolve_stemmer(42)


def test_named_stemmer_without_pystemmer_names_the_option():
    try:
        import Stemmer  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="stemmer='english'"):
            B.resolve_stemmer("english")
    else:
        assert B.resolve_stemmer("english")(["running"]) == ["run"]


def _lucene(tf, df, dl, avgdl, n, k1=1.5, b=0.75):
    idf = math.log(1 + (n - df + 0.5) / (df + 0.5))
    return np.float32(idf * tf / (tf + k1 * (1 - b + b * dl / avgdl)))


def test_builder_matches_hand_computed_lucene_values(tmp_path):
    texts = ["apple banana apple", "banana cherry", "apple apple apple cherry date"]
    B.build_bm25_index(texts, str(tmp_path), doc_ids=["d0", "d1", "d2"], stemmer=None)
    ix = B.load_bm25_index(str(tmp_path))
    assert ix.vocab == {"apple": 0, "banana": 1, "cherry": 2, "date": 3}
    assert ix.num_docs == 3 and ix.corpus == ["d0", "d1", "d2"] and ix.params["method"] == "lucene"
    avgdl = (3 + 2 + 5) / 3
    want = {  # column -> [(row, tf, df, dl)]
        0: [(0, 2, 2, 3), (2, 3, 2, 5)],
        1: [(0, 1, 2, 3), (1, 1, 2, 2)],
        2: [(1, 1, 2, 2), (2, 1, 2, 5)],
        3: [(2, 1, 1, 5)],
    }
    assert ix.indptr.tolist() == [0, 2, 4, 6, 7]
    for c, posts in want.items():
        seg = slice(ix.indptr[c], ix.indptr[c + 1])
        assert ix.indices[seg].tolist() == [p[0] for p in posts]
        got = ix.data[seg]
        exp = np.array([_lucene(tf, df, dl, avgdl, 3) for _, tf, df, dl in posts], np.float32)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (c, got, exp)
    assert ix.data.dtype == np.float32 and ix.indices.dtype == np.int32 and ix.indptr.dtype == np.int64


def test_round_trip_and_loader_refusals(tmp_path):
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 12, size=500)
    off = np.concatenate([[0], np.cumsum(lens)])
    toks = rng.zipf(1.3, size=int(off[-1])) % 300
    d = str(tmp_path / "ix")
    B.build_bm25_index_from_ids(off, toks, 300, d)
    ix = B.load_bm25_index(d, load_corpus=False)
    indptr, indices, data = B.bm25_index_arrays(off, toks, 300)
    assert np.array_equal(ix.indptr, indptr) and np.array_equal(ix.indices, indices) and np.array_equal(ix.data, data)
    assert ix.num_docs == 500 and ix.corpus is None and (ix.data > 0).all()
    for c in range(300):   # one posting per (column, document), rows ascending
        assert np.all(np.diff(ix.indices[ix.indptr[c]:ix.indptr[c + 1]]) > 0)

    # columns written with rows out of order are put in order on load (the same postings)
    shuffled = str(tmp_path / "shuffled")
    shutil.copytree(d, shuffled)
    order = np.arange(indices.size)
    for c in range(300):
        seg = order[indptr[c]:indptr[c + 1]]
        order[indptr[c]:indptr[c + 1]] = seg[::-1]
    np.save(os.path.join(shuffled, B.FILES["indices"]), indices[order])
    np.save(os.path.join(shuffled, B.FILES["data"]), data[order])
    again = B.load_bm25_index(shuffled)
    assert np.array_equal(again.indices, indices) and np.array_equal(again.data, data)

    for method in ("bm25l", "bm25+"):
        bad = str(tmp_path / method)
        shutil.copytree(d, bad)
        p = json.load(open(os.path.join(bad, B.FILES["params"])))
        p["method"] = method
        json.dump(p, open(os.path.join(bad, B.FILES["params"]), "w"))
        with pytest.raises(ValueError, match="non-occurrence"):
            B.load_bm25_index(bad)
    for value in (0.0, -0.25):
        bad = str(tmp_path / f"data{value}")
        shutil.copytree(d, bad)
        neg = data.copy()
        neg[3] = value
        np.save(os.path.join(bad, B.FILES["data"]), neg)
        with pytest.raises(ValueError, match="> 0"):
            B.load_bm25_index(bad)


def test_load_from_chroma_and_save_has_the_reference_signature(tmp_path):
    class Doc:
        def __init__(self, text, doc_id):
            self.page_content, self.metadata = text, {"doc_id": doc_id}

    try:
        import Stemmer  # noqa: F401
        have = True
    except ImportError:
        have = False
    docs = [Doc("Revenue grew in 2023", "a"), Doc("Revenue fell", "b")]
    if not have:   # the reference's stemmer is PyStemmer's English one: without it the ingest says what is missing
        with pytest.raises(ImportError, match="PyStemmer"):
            B.load_from_chroma_and_save(docs, str(tmp_path))
    else:
        B.load_from_chroma_and_save(docs, str(tmp_path))
        assert B.load_bm25_index(str(tmp_path)).corpus == ["a", "b"]


def test_abi_lists_the_bm25_entry_points():
    from veritasfi_amd import build, _ffi
    syms = build.api_symbols()
    for name in ("vf_bm25_create", "vf_bm25_search"):
        assert name in syms and name in _ffi.SIGNATURES
    assert "vf_sparse.hip" in build.SOURCES


class _Store:
    def __init__(self, docs, metas, embs):
        self.docs, self.metas, self.embs = docs, metas, embs
        self.by_id = {m["doc_id"]: i for i, m in enumerate(metas)} if metas and metas[0] else {}

    def get(self, ids=None, include=()):
        if ids is None:
            return {"documents": self.docs, "metadatas": self.metas, "embeddings": self.embs}
        rows = [self.by_id[i] for i in ids]
        return {"documents": [self.docs[r] for r in rows], "metadatas": [self.metas[r] for r in rows]}


class _Dense:
    def __init__(self, embeddings, fn):
        self.x = np.asarray(embeddings, np.float32)

    def invoke(self, querys, k):
        n = self.x.shape[0]
        ids = np.tile(np.arange(min(k, n)), (len(querys), 1))
        return ids, np.full(ids.shape, 0.5, np.float32)


class _Ranked:
    """A full ranking (total order); records the depth it is asked for.  min_score filters ids only, as upstream."""

    def __init__(self, order, scores, min_score=None):
        self.order, self.scores, self.min_score, self.depths = order, scores, min_score, []

    def invoke(self, query, k):
        self.depths.append(k)
        ids, sc = self.order[:k], self.scores[:k]
        if self.min_score is not None:
            ids = [i for i, s in zip(ids, sc) if s >= self.min_score]
        return ids, sc


class _RankedPrefix(_Ranked):
    exact_prefix = True


@pytest.mark.parametrize("min_score", [None, 0.55])
def test_ensemble_asks_an_exact_prefix_retriever_for_bm25_k_rows_only(min_score):
    from veritasfi_amd.ensemble import EnsembleRetriever
    n = 40
    rng = np.random.default_rng(3)
    metas = [{"doc_id": f"d{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": "t" if i == 5 else f"u{i}",
              **({"bundle_id": f"b{i // 4}"} if i % 4 < 2 else {})} for i in range(n)]
    chroma = _Store([f"text {i}" for i in range(n)], metas, rng.standard_normal((n, 4)).tolist())
    ts = _Store(["t"], [None], rng.standard_normal((1, 4)).tolist())
    order = rng.permutation(n).tolist()
    scores = np.sort(rng.random(n).astype(np.float32))[::-1]
    outs = []
    for cls in (_Ranked, _RankedPrefix):
        bm = cls(order, scores, min_score)
        er = EnsembleRetriever("unused", chroma, ts, 3, None, faiss_k=2, faiss_ts_k=1, bm25_k=7, bm25_retriever=bm,
                               retriever_cls=_Dense)
        outs.append(er.invoke("q", []))
        assert bm.depths == ([n] if cls is _Ranked else [7])
    assert outs[0] == outs[1] and any(c["retriever"] == "BM25" for c in outs[0])


def test_new_kernels_use_no_scratch():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    from veritasfi_amd import build as vf_build
    kernels = ru.usage(os.path.join(vf_build.CSRC, "vf_sparse.hip"))
    names = {k["pretty"] for k in kernels}
    for must in ("k_bm25_accum", "k_bm25_hist", "k_bm25_pick", "k_bm25_gather", "k_bm25_sort_small", "k_bm25_tail_write",
                 "k_bm25_reset", "k_bitonic_global", "k_bitonic_lds"):
        assert must in names, must
    bad = [(k["pretty"], k.get("scratch"), k.get("vgpr_spill")) for k in kernels
           if k.get("scratch", 0) > 0 or k.get("vgpr_spill", 0) > 0 or str(k.get("dynamic_stack", "False")) == "True"]
    assert not bad, bad
