"""BM25Retriever -- drop-in for ``src/utils/bm25Retriever.py`` (the ensemble's third leg) with scoring and ranking on the GPU.

The reference loads a bm25s index directory and, per request, tokenises the query (``bm25s.tokenize(..., stopwords="english",
stemmer=Stemmer('english'))``) and ranks every chunk (``retrieve(k=num_chunk)``, ``ensembleRetriever.py:188-190``).  Here the
index's CSC arrays live in HBM and ``vf_bm25_search`` scores and ranks on the device (``csrc/vf_sparse.hip``); tokenising and
the index files are host numpy / json only -- bm25s is not needed.

Index directory (what bm25s's ``BM25.save`` writes; this layout is UNPINNED against bm25s itself -- no bm25s installation was
available to compare with -- so the names and types below are what this module reads and writes):

* ``params.index.json``   -- json object: ``k1``, ``b``, ``method`` (``"lucene"``, ``"robertson"``, ``"atire"``; ``"bm25l"`` /
  ``"bm25+"`` are refused: they need a non-occurrence array), ``num_docs``, and ``delta``, ``idf_method``, ``dtype``,
  ``int_dtype``, ``version``, ``backend`` as bm25s writes them (ignored on load).
* ``vocab.index.json``    -- json object: token string -> column.
* ``data.csc.index.npy``  -- float32 [nnz]: the precomputed score of each posting (must all be > 0).
* ``indices.csc.index.npy`` -- integer [nnz] (int32 written): the document row of each posting.
* ``indptr.csc.index.npy``  -- integer [V + 1] (int64 written): column c holds postings ``indptr[c] .. indptr[c+1]``.
* ``corpus.jsonl``        -- optional: one json value per line, row order (the reference stores the chunk's ``doc_id``).

Query tokens: lowercase, ``(?u)\\b\\w\\w+\\b``, drop stopwords, stem; then each token's column, in order, repeats kept, tokens
the vocabulary does not know dropped.  The shipped English stopword list (``data/stopwords_en.txt``) is the 33-word Lucene
list; that it equals bm25s's ``"english"`` list is unpinned, as is PyStemmer's English stemmer against the index's tokens
(the stemmer is PyStemmer's own when it is installed).
"""
from __future__ import annotations

import json
import os
import re
import threading
from typing import List, Optional, Sequence

import numpy as np

from . import _ffi

_TOKEN = re.compile(r"(?u)\b\w\w+\b")
_HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"params": "params.index.json", "vocab": "vocab.index.json", "data": "data.csc.index.npy",
         "indices": "indices.csc.index.npy", "indptr": "indptr.csc.index.npy", "corpus": "corpus.jsonl"}
SERVED_METHODS = ("lucene", "robertson", "atire")


def _load_stopwords_en() -> frozenset:
    with open(os.path.join(_HERE, "data", "stopwords_en.txt"), encoding="utf-8") as f:
        return frozenset(w.strip() for w in f if w.strip())


STOPWORDS_EN = _load_stopwords_en()


def resolve_stopwords(stopwords) -> frozenset:
    """None / "english" / "en" -> the shipped English list; any iterable of strings -> that set (empty: no stopwords)."""
    if stopwords is None or (isinstance(stopwords, str) and stopwords.lower() in ("english", "en")):
        return STOPWORDS_EN
    if isinstance(stopwords, str):
        raise ValueError(f"stopwords={stopwords!r}: only 'english' is shipped; pass a list of words instead")
    return frozenset(stopwords)


def resolve_stemmer(stemmer):
    """-> a function list[str] -> list[str].  A string names a PyStemmer algorithm (the reference: ``Stemmer.Stemmer("english")``);
    None = no stemming; an object with ``stemWords`` or a callable (one word -> its stem) is used as given."""
    if stemmer is None:
        return lambda words: list(words)
    if isinstance(stemmer, str):
        try:
            import Stemmer  # PyStemmer
        except ImportError as e:
            raise ImportError(f"stemmer={stemmer!r} needs PyStemmer (import Stemmer), which is not installed: install it, or pass "
                              "stemmer=None, an object with stemWords(list) or a callable word -> stem") from e
        stemmer = Stemmer.Stemmer(stemmer)
    if hasattr(stemmer, "stemWords"):
        return lambda words: list(stemmer.stemWords(list(words)))
    if callable(stemmer):
        return lambda words: [stemmer(w) for w in words]
    raise TypeError("stemmer must be a PyStemmer algorithm name, None, an object with stemWords, or a callable")


def tokenize(text: str, stem=None, stopwords: frozenset = STOPWORDS_EN) -> List[str]:
    """bm25s.tokenize's steps for one text: lowercase, the token pattern, stopwords out, then the stemmer (``stem`` from
    ``resolve_stemmer``; None = none).  Order and repeats kept."""
    words = [w for w in _TOKEN.findall(text.lower()) if w not in stopwords]
    return stem(words) if stem is not None and words else words


# ---- index files -------------------------------------------------------------------------------------------------------------
def bm25_index_arrays(doc_offsets, token_ids, vocab_size: int, k1: float = 1.5, b: float = 0.75):
    """Lucene BM25 over token ids -> CSC (indptr int64 [V+1], indices int32 [nnz], data float32 [nnz]).
    Document d's tokens are ``token_ids[doc_offsets[d]:doc_offsets[d+1]]`` (repeats = term frequency).
    idf = ln(1 + (N - df + 0.5) / (df + 0.5)), data = idf * tf / (tf + k1 * (1 - b + b * dl / avgdl)): float64, rounded once."""
    off = np.asarray(doc_offsets, dtype=np.int64)
    tok = np.asarray(token_ids, dtype=np.int64)
    if off.ndim != 1 or off.size < 2 or off[0] != 0 or off[-1] != tok.size or np.any(np.diff(off) < 0):
        raise ValueError("doc_offsets must be non-decreasing, start at 0 and end at len(token_ids)")
    V, N = int(vocab_size), int(off.size - 1)
    if tok.size and (tok.min() < 0 or tok.max() >= V):
        raise ValueError("token ids must lie in [0, vocab_size)")
    dl = np.diff(off)
    doc = np.repeat(np.arange(N, dtype=np.int64), dl)
    pair, tf = np.unique(tok * N + doc, return_counts=True)      # sorted by (token, doc): CSC order
    col, row = pair // N, pair % N
    df = np.bincount(col, minlength=V).astype(np.float64)
    idf = np.log(1.0 + (N - df + 0.5) / (df + 0.5))
    avgdl = float(dl.mean()) if N else 1.0
    tf = tf.astype(np.float64)
    data = (idf[col] * tf / (tf + k1 * (1.0 - b + b * dl[row] / (avgdl if avgdl > 0 else 1.0)))).astype(np.float32)
    indptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=V), out=indptr[1:])
    return indptr, row.astype(np.int32), data


def _write_index(save_dir, indptr, indices, data, vocab: dict, num_docs: int, k1: float, b: float, corpus=None) -> str:
    os.makedirs(save_dir, exist_ok=True)
    np.save(os.path.join(save_dir, FILES["data"]), data.astype(np.float32))
    np.save(os.path.join(save_dir, FILES["indices"]), indices.astype(np.int32))
    np.save(os.path.join(save_dir, FILES["indptr"]), indptr.astype(np.int64))
    with open(os.path.join(save_dir, FILES["vocab"]), "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    params = {"k1": k1, "b": b, "delta": 0.5, "method": "lucene", "idf_method": "lucene", "dtype": "float32",
              "int_dtype": "int32", "num_docs": int(num_docs), "version": "veritasfi_amd", "backend": "numpy"}
    with open(os.path.join(save_dir, FILES["params"]), "w", encoding="utf-8") as f:
        json.dump(params, f, indent=4)
    if corpus is not None:
        with open(os.path.join(save_dir, FILES["corpus"]), "w", encoding="utf-8") as f:
            for item in corpus:
                f.write(json.dumps(item, ensure_ascii=False) + "\n")
    return save_dir


def build_bm25_index_from_ids(doc_offsets, token_ids, vocab_size: int, save_dir: str, k1: float = 1.5, b: float = 0.75,
                              vocab: Optional[dict] = None, corpus=None) -> str:
    """The index directory from token ids (no strings: 1M-10M-document test indices).  ``vocab`` defaults to {"t<i>": i}."""
    indptr, indices, data = bm25_index_arrays(doc_offsets, token_ids, vocab_size, k1, b)
    vocab = {f"t{i}": i for i in range(int(vocab_size))} if vocab is None else vocab
    return _write_index(save_dir, indptr, indices, data, vocab, len(doc_offsets) - 1, k1, b, corpus)


def build_bm25_index(texts: Sequence[str], save_dir: str, doc_ids=None, k1: float = 1.5, b: float = 0.75, stemmer="english",
                     stopwords=None) -> str:
    """The index directory of ``texts`` (bm25s ``tokenize`` + ``BM25().index`` + ``save``, Lucene method); ``doc_ids`` -> corpus.jsonl."""
    stem, stop = resolve_stemmer(stemmer), resolve_stopwords(stopwords)
    vocab: dict = {}
    offsets, ids = [0], []
    for text in texts:
        for w in tokenize(text, stem, stop):
            ids.append(vocab.setdefault(w, len(vocab)))
        offsets.append(len(ids))
    indptr, indices, data = bm25_index_arrays(offsets, np.asarray(ids, dtype=np.int64), len(vocab), k1, b)
    return _write_index(save_dir, indptr, indices, data, vocab, len(offsets) - 1, k1, b, doc_ids)


def load_from_chroma_and_save(documents, save_dir: str):
    """The reference's ingest step (bm25Retriever.py:10-20): page_content indexed, metadata['doc_id'] as the corpus."""
    build_bm25_index([d.page_content for d in documents], save_dir, doc_ids=[d.metadata["doc_id"] for d in documents])


class BM25Index:
    """The arrays and settings of an index directory (``load_bm25_index``)."""

    def __init__(self, params, vocab, indptr, indices, data, num_docs, corpus):
        self.params, self.vocab, self.indptr, self.indices, self.data = params, vocab, indptr, indices, data
        self.num_docs, self.corpus = num_docs, corpus


def load_bm25_index(dir_path: str, load_corpus: bool = True) -> BM25Index:
    """Read the directory (numpy + json).  Refuses methods that need a non-occurrence array and non-positive scores (a
    document the query does not touch must score exactly 0); rows are put in ascending order within each column."""
    with open(os.path.join(dir_path, FILES["params"]), encoding="utf-8") as f:
        params = json.load(f)
    method = str(params.get("method", "lucene")).lower()
    if method not in SERVED_METHODS:
        raise ValueError(f"BM25 index {dir_path}: method {method!r} is not served (it needs a non-occurrence array); "
                         f"served: {', '.join(SERVED_METHODS)}")
    with open(os.path.join(dir_path, FILES["vocab"]), encoding="utf-8") as f:
        vocab = json.load(f)
    data = np.ascontiguousarray(np.load(os.path.join(dir_path, FILES["data"])), dtype=np.float32)
    indices = np.load(os.path.join(dir_path, FILES["indices"]))
    indptr = np.ascontiguousarray(np.load(os.path.join(dir_path, FILES["indptr"])), dtype=np.int64)
    if data.ndim != 1 or indices.shape != data.shape or indptr.ndim != 1 or indptr.size < 1 or indptr[0] != 0 \
            or indptr[-1] != data.size or np.any(np.diff(indptr) < 0):
        raise ValueError(f"BM25 index {dir_path}: inconsistent CSC arrays")
    if data.size and not (np.isfinite(data).all() and (data > 0).all()):
        raise ValueError(f"BM25 index {dir_path}: posting scores must be finite and > 0 (an idf that can go negative, e.g. "
                         "Robertson's on very common tokens, is not served)")
    if "num_docs" not in params:
        raise ValueError(f"BM25 index {dir_path}: params.index.json has no num_docs")
    num_docs = int(params["num_docs"])
    if indices.size and (indices.min() < 0 or indices.max() >= num_docs):
        raise ValueError(f"BM25 index {dir_path}: a document row is out of range")
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    col = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    step = np.diff(indices.astype(np.int64))
    same = col[1:] == col[:-1]
    if np.any(step[same] <= 0):   # bm25s writes ascending rows (scipy's canonical CSC); sort when it did not
        order = np.lexsort((indices, col))
        indices, data = indices[order], data[order]
        if np.any(np.diff(indices.astype(np.int64))[same] == 0):
            raise ValueError(f"BM25 index {dir_path}: a document appears twice in one column")
    corpus = None
    cpath = os.path.join(dir_path, FILES["corpus"])
    if load_corpus and os.path.exists(cpath):
        with open(cpath, encoding="utf-8") as f:
            corpus = [json.loads(line) for line in f if line.strip()]
    return BM25Index(params, vocab, indptr, indices, data, num_docs, corpus)


# ---- the retriever ---------------------------------------------------------------------------------------------------------
class BM25Retriever:
    """The reference's constructor and ``invoke(query, k) -> (ids, scores)``; scoring and ranking run on the GPU.

    ``ids`` is a list of int rows, ``scores`` a float32 array of length k: score descending, ties to the lower row, untouched
    rows (score 0) after the touched ones in ascending row order.  ``min_score`` filters ``ids`` only, as upstream
    (bm25Retriever.py:83-87).  The ranking is a total order, so the first k of ``invoke(q, N)`` are ``invoke(q, k)``:
    ``exact_prefix`` tells ``EnsembleRetriever`` it may ask for ``bm25_k`` rows instead of all of them.  A handle may be
    shared across threads (the device handle serialises its calls)."""

    exact_prefix = True

    def __init__(self, dir_path: str, load_corpus: bool = True, min_score: Optional[float] = None, stemmer="english",
                 device_id: int = 0, stopwords=None):
        self.min_score = min_score
        self._stem = resolve_stemmer(stemmer)
        self._stopwords = resolve_stopwords(stopwords)
        ix = load_bm25_index(dir_path, load_corpus=load_corpus)
        self.vocab, self.corpus, self.params = ix.vocab, ix.corpus, ix.params
        self.num_docs = self.doc_len = ix.num_docs
        self._h, slots = _ffi.vp(), _ffi.c_i32()
        _ffi.check(_ffi.lib().vf_bm25_create(ix.indptr.ctypes.data_as(_ffi.p_i64), int(ix.indptr.size - 1),
                                             ix.indices.ctypes.data_as(_ffi.p_i32), ix.data.ctypes.data_as(_ffi.p_f32),
                                             int(ix.data.size), int(ix.num_docs), int(device_id), _ffi.ctypes.byref(self._h),
                                             _ffi.ctypes.byref(slots)), "vf_bm25_create")
        self._info = {"n_docs": int(ix.num_docs), "vocab": int(ix.indptr.size - 1), "nnz": int(ix.data.size), "slots": slots.value}
        self._mu = threading.Lock()

    def query_columns(self, query: str) -> np.ndarray:
        """The query's token columns in order (repeats kept, unknown tokens dropped), int32."""
        v = self.vocab
        return np.asarray([v[w] for w in tokenize(query, self._stem, self._stopwords) if w in v], dtype=np.int32)

    def search_columns(self, columns: Sequence[np.ndarray], k: int):
        """Token-column lists -> (ids int64 [nq, k], scores float32 [nq, k]) in one device call."""
        cols = [np.asarray(c, dtype=np.int32).ravel() for c in columns]
        nq, k = len(cols), int(k)
        if not 1 <= k <= self.num_docs:
            raise ValueError(f"k={k}: must be in [1, {self.num_docs}] (the number of documents)")
        offsets = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum([c.size for c in cols], out=offsets[1:])
        terms = np.ascontiguousarray(np.concatenate(cols) if nq else np.zeros(0, np.int32), dtype=np.int32)
        ids = np.empty((nq, k), dtype=np.int64)
        scores = np.empty((nq, k), dtype=np.float32)
        if nq == 0:
            return ids, scores
        with self._mu:
            if not self._h.value:
                raise RuntimeError("BM25Retriever is closed")
            _ffi.check(_ffi.lib().vf_bm25_search(self._h, offsets.ctypes.data_as(_ffi.p_i64), terms.ctypes.data_as(_ffi.p_i32),
                                                 nq, k, ids.ctypes.data_as(_ffi.p_i64), scores.ctypes.data_as(_ffi.p_f32)),
                       "vf_bm25_search")
        return ids, scores

    def _result(self, ids_row: np.ndarray, scores_row: np.ndarray):
        ids = [int(i) for i in ids_row]
        if self.min_score is not None:
            ids = [i for i, s in zip(ids, scores_row) if s >= self.min_score]
        return ids, scores_row

    def invoke(self, query: str, k: int, metadata_filters=None):
        """(ids, scores) of the k best rows (bm25Retriever.py:50-87)."""
        if metadata_filters:
            raise NotImplementedError("Metadata filtering is not supported yet.")   # as upstream (:69-72)
        ids, scores = self.search_columns([self.query_columns(query)], k)
        return self._result(ids[0], scores[0])

    def invoke_batch(self, queries: Sequence[str], k: int):
        """[(ids, scores)] per query, all in one device call."""
        ids, scores = self.search_columns([self.query_columns(q) for q in queries], k)
        return [self._result(ids[i], scores[i]) for i in range(len(ids))]

    def info(self) -> dict:
        """n_docs, vocab, nnz, and slots: queries one device pass serves."""
        return dict(self._info)

    def close(self) -> None:
        mu = getattr(self, "_mu", None)
        if mu is None:
            return
        with mu:
            if self._h.value:
                h = _ffi.vp(self._h.value)
                _ffi.lib().vf_bm25_create(None, 0, None, None, 0, 0, 0, _ffi.ctypes.byref(h), None)   # release
                self._h = _ffi.vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
