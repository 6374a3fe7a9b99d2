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
* ``tf.csc.index.npy``    -- optional, this package's own: int32 [nnz], the term frequency of each posting.  bm25s does not write
  it, and it cannot be recovered from the scores; a LIVE retriever (``live=True``: documents added and removed on the device) needs it.

Query tokens: lowercase, ``(?u)\\b\\w\\w+\\b``, drop stopwords, stem; then each token's column, in order, repeats kept, tokens
the vocabulary does not know dropped.  The shipped English stopword list (``data/stopwords_en.txt``) is the 33-word Lucene
list; that it equals bm25s's ``"english"`` list is unpinned, as is PyStemmer's English stemmer against the index's tokens
(the stemmer is PyStemmer's own when it is installed).
"""
from __future__ import annotations

import contextlib
import json
import os
import re
import threading
import time
import weakref
from typing import List, Optional, Sequence

import numpy as np

from . import _ffi
from .index import RowSubset, subset_ids

_TOKEN = re.compile(r"(?u)\b\w\w+\b")
_HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"params": "params.index.json", "vocab": "vocab.index.json", "data": "data.csc.index.npy",
         "indices": "indices.csc.index.npy", "indptr": "indptr.csc.index.npy", "corpus": "corpus.jsonl", "tf": "tf.csc.index.npy"}
SERVED_METHODS = ("lucene", "robertson", "atire")
_NO_LOCK = contextlib.nullcontext()


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
def bm25_index_arrays(doc_offsets, token_ids, vocab_size: int, k1: float = 1.5, b: float = 0.75, return_tf: bool = False):
    """Lucene BM25 over token ids -> CSC (indptr int64 [V+1], indices int32 [nnz], data float32 [nnz]); with ``return_tf`` a
    fourth array, the term frequencies int32 [nnz] in posting order.
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
    tf_int = tf.astype(np.int32)
    tf = tf.astype(np.float64)
    data = (idf[col] * tf / (tf + k1 * (1.0 - b + b * dl[row] / (avgdl if avgdl > 0 else 1.0)))).astype(np.float32)
    indptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=V), out=indptr[1:])
    if return_tf:
        return indptr, row.astype(np.int32), data, tf_int
    return indptr, row.astype(np.int32), data


def _write_index(save_dir, indptr, indices, data, vocab: dict, num_docs: int, k1: float, b: float, corpus=None, tf=None) -> str:
    os.makedirs(save_dir, exist_ok=True)
    if tf is not None:
        np.save(os.path.join(save_dir, FILES["tf"]), np.asarray(tf).astype(np.int32))
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
    indptr, indices, data, tf = bm25_index_arrays(doc_offsets, token_ids, vocab_size, k1, b, return_tf=True)
    vocab = {f"t{i}": i for i in range(int(vocab_size))} if vocab is None else vocab
    return _write_index(save_dir, indptr, indices, data, vocab, len(doc_offsets) - 1, k1, b, corpus, tf=tf)


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
    indptr, indices, data, tf = bm25_index_arrays(offsets, np.asarray(ids, dtype=np.int64), len(vocab), k1, b, return_tf=True)
    return _write_index(save_dir, indptr, indices, data, vocab, len(offsets) - 1, k1, b, doc_ids, tf=tf)


def load_from_chroma_and_save(documents, save_dir: str):
    """The reference's ingest step (bm25Retriever.py:10-20): page_content indexed, metadata['doc_id'] as the corpus."""
    build_bm25_index([d.page_content for d in documents], save_dir, doc_ids=[d.metadata["doc_id"] for d in documents])


class BM25Index:
    """The arrays and settings of an index directory (``load_bm25_index``)."""

    def __init__(self, params, vocab, indptr, indices, data, num_docs, corpus, tf=None):
        self.params, self.vocab, self.indptr, self.indices, self.data = params, vocab, indptr, indices, data
        self.num_docs, self.corpus = num_docs, corpus
        self.tf = tf   # int32 [nnz] term frequencies, or None: the directory has no tf file (bm25s's own do not)


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
    tf = None
    if os.path.exists(os.path.join(dir_path, FILES["tf"])):
        tf = np.ascontiguousarray(np.load(os.path.join(dir_path, FILES["tf"])), dtype=np.int32)
        if tf.shape != data.shape or (tf.size and tf.min() < 1):
            raise ValueError(f"BM25 index {dir_path}: {FILES['tf']} must hold one term frequency >= 1 per posting")
    col = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    step = np.diff(indices.astype(np.int64))
    same = col[1:] == col[:-1]
    if np.any(step[same] <= 0):   # bm25s writes ascending rows (scipy's canonical CSC); sort when it did not
        order = np.lexsort((indices, col))
        indices, data = indices[order], data[order]
        tf = tf[order] if tf is not None else None
        if np.any(np.diff(indices.astype(np.int64))[same] == 0):
            raise ValueError(f"BM25 index {dir_path}: a document appears twice in one column")
    corpus = None
    cpath = os.path.join(dir_path, FILES["corpus"])
    if load_corpus and os.path.exists(cpath):
        with open(cpath, encoding="utf-8") as f:
            corpus = [json.loads(line) for line in f if line.strip()]
    return BM25Index(params, vocab, indptr, indices, data, num_docs, corpus, tf)


def filter_words(subset, n: int):
    """(words, m): the bitmap ``vf_bm25_search`` takes with VF_BM25_FILTER -- uint32 [(n + 31) // 32], bit ``r & 31`` of word
    ``r >> 5`` set = row r may be returned -- and the number of rows it allows.  ``subset`` is what the dense leg's
    ``search(subset=...)`` takes: an integer array-like of ids (any order, repeats count once; an id outside [0, n) is a ValueError
    naming it), a boolean mask of length ``n``, or a ``RowSubset`` (its host ids are read).  Packed by numpy, no loop over rows."""
    n = int(n)
    if isinstance(subset, RowSubset) or hasattr(subset, "tensor"):
        ids = getattr(subset, "ids", None)
        if ids is None:
            raise TypeError("subset: this RowSubset does not expose its host ids (.ids); pass the ids or a boolean mask instead")
        subset = ids
    a = np.asarray(subset)
    mask = np.zeros((n + 31) // 32 * 32, dtype=np.bool_)
    if a.dtype == np.bool_:
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"subset: a boolean mask must have one entry per row ({n}), got shape {a.shape}")
        mask[:n] = a
    else:
        mask[subset_ids(a, n)] = True
    words = np.ascontiguousarray(np.packbits(mask, bitorder="little").view(np.dtype("<u4")), dtype=np.uint32)
    return words, int(np.count_nonzero(mask))


_STATS_UNSET = object()   # ``stats=`` was not passed: "corpus" beside rows, the object's own mode beside a ``BM25Subset``


class BM25Subset:
    """A set of rows PREPARED on a ``BM25Retriever``'s device (``prepare_subset``): the filter's bitmap and, with ``stats="subset"``,
    the subset's idf for every column of the vocabulary stay in HBM, so a search with ``subset=<this object>`` uploads nothing but its
    query and is ONE device call in both modes.  ``m`` rows allowed, ``total_len`` their tokens and ``df`` (int64 [V], their postings
    per column; both ``stats="subset"`` only, else 0 / None), ``stats`` the mode, ``generation`` the index's update generation it was
    made at, ``nbytes`` the device memory it holds (0 once closed).  It holds rows, not meaning: after the retriever's next update
    (``add_texts``, ``remove``, ...) it is stale and every search with it is refused -- call ``prepare_subset`` again.  ``close()``
    (or ``with``) frees it; ``BM25Retriever.close()`` frees all of a retriever's."""

    def __init__(self, retriever, token: int, stats: str, m: int, total_len: int, generation: int, df, nbytes: int):
        self._retriever, self._token, self._closed, self._stale = retriever, int(token), False, False
        self.stats, self.m, self.total_len, self.generation, self.df, self.nbytes = stats, int(m), int(total_len), int(generation), df, int(nbytes)

    @property
    def closed(self) -> bool:
        return self._closed

    @property
    def stale(self) -> bool:
        return self._stale

    def close(self) -> None:
        """Free the device copy; harmless twice, and after the retriever itself has closed (which has freed it)."""
        if not self._closed:
            self._retriever._release_subset(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        # never the library from a finaliser (it may run inside any call that holds the retriever's lock): the token is left for the
        # retriever's next locked call to release; a retriever that has closed marked this object closed and has nothing left to free
        try:
            if not self._closed and not self._stale:
                self._closed = True
                self._retriever._orphans.append(self._token)
        except Exception:
            pass


# ---- the retriever ---------------------------------------------------------------------------------------------------------
class BM25Retriever:
    """The reference's constructor and ``invoke(query, k) -> (ids, scores)``; scoring and ranking run on the GPU.

    ``ids`` is a list of int rows, ``scores`` a float32 array of length k: score descending, ties to the lower row, untouched
    rows (score 0) after the touched ones in ascending row order.  ``min_score`` filters ``ids`` only, as upstream
    (bm25Retriever.py:83-87).  The ranking is a total order, so the first k of ``invoke(q, N)`` are ``invoke(q, k)``:
    ``exact_prefix`` tells ``EnsembleRetriever`` it may ask for ``bm25_k`` rows instead of all of them.  A handle may be
    shared across threads (the device handle serialises its calls).

    ``subset=`` (``invoke``, ``invoke_batch``, ``search_columns``): only these rows may be returned -- ids, a boolean mask or a
    ``RowSubset``, as the dense leg takes them.  Scores keep the WHOLE corpus's statistics: the result is the unfiltered ranking with
    the other rows struck out, cut to k, filtered inside the device's kernels (``vf_bm25_search`` with VF_BM25_FILTER; the bitmap,
    n / 8 bytes, goes up with every call).  ``filtered_prefix`` tells ``EnsembleRetriever`` it may ask a filtered request for
    ``bm25_k`` rows with ``subset=`` instead of ranking every row and filtering on the host.

    ``stats="subset"`` beside ``subset=`` (a live retriever only): the scores are those of an index built from the allowed rows ALONE --
    N, df and the mean length are the subset's (one index per company, as upstream deploys) -- bit for bit what ``BM25Retriever`` over
    ``bm25_index_arrays`` of those documents returns, rows mapped back.  The device counts (``subset_statistics``), numpy takes the
    logarithm, the device scores each allowed posting from its term frequency (VF_BM25_SUBSTATS).  ``stats="corpus"`` is the default.

    ``live=True``: documents can be added and removed without a rebuild (``add_texts``, ``add_token_ids``, ``remove``, ``update``,
    ``save``).  Ids stay the positions: removed rows leave and later rows move down, new documents get the ids n .. n + m - 1, a
    token the vocabulary lacks gets a new column at the end, columns never disappear.  After every update the device holds, bit
    for bit, what ``bm25_index_arrays`` gives for the surviving documents followed by the new ones (every posting is re-scored:
    N, df and avgdl change with one document).  It needs the directory's term frequencies (``tf.csc.index.npy``) and the Lucene
    method; the posting scores are then computed on the device from tf, and the directory's own are not used.  During an update
    the device holds the postings twice.

    ``prepare_subset(subset, stats)`` -> ``BM25Subset``: the same filter on many requests (one index per tenant) is packed, checked,
    uploaded and -- with stats="subset" -- counted ONCE; passed as ``subset=`` it makes every request one device call that uploads only
    the query, with the result of the unprepared call bit for bit (VF_BM25_PREPARED).

    ``subsets=[...]`` (``search_columns``, ``invoke_batch``): a ``BM25Subset`` or None PER QUERY -- a batch whose queries belong to
    different tenants is still one device call, and query i returns what it returns alone with ``subset=subsets[i]``."""

    exact_prefix = True
    filtered_prefix = True

    def __init__(self, dir_path: str, load_corpus: bool = True, min_score: Optional[float] = None, stemmer="english",
                 device_id: int = 0, stopwords=None, live: bool = False, live_chunk: int = 0):
        self.min_score = min_score
        self._stem = resolve_stemmer(stemmer)
        self._stopwords = resolve_stopwords(stopwords)
        ix = load_bm25_index(dir_path, load_corpus=load_corpus)
        self.vocab, self.corpus, self.params = ix.vocab, ix.corpus, ix.params
        self.num_docs = self.doc_len = ix.num_docs
        self.live, self._device, self._chunk = bool(live), int(device_id), int(live_chunk)
        self._h, slots = _ffi.vp(), _ffi.c_i32()
        self._mu = threading.Lock()
        self._update_mu = threading.RLock()   # one update at a time, tokenising included (a new token's column is decided there)
        self._subsets = weakref.WeakValueDictionary()   # token -> BM25Subset: the prepared filters that can still search
        self._orphans: list = []                        # tokens of collected BM25Subsets, released by the next locked call
        self._info = {"n_docs": int(ix.num_docs), "vocab": int(ix.indptr.size - 1), "nnz": int(ix.data.size), "slots": 0}
        if self.live:
            if ix.tf is None:
                raise ValueError(f"BM25 index {dir_path}: live=True needs {FILES['tf']} (the term frequency of every posting), which "
                                 "this directory does not have -- bm25s does not write it and it cannot be recovered from the "
                                 "scores; rebuild the directory from the texts with veritasfi_amd.bm25.build_bm25_index")
            method = str(ix.params.get("method", "lucene")).lower()
            if method != "lucene":
                raise ValueError(f"BM25 index {dir_path}: live=True re-scores postings by the Lucene method, not {method!r}")
            self._k1, self._b = float(ix.params.get("k1", 1.5)), float(ix.params.get("b", 0.75))
            self._dl = np.bincount(ix.indices, weights=ix.tf, minlength=ix.num_docs).astype(np.int64)   # tokens per document
            self._df, self._total = np.zeros(0, np.int64), 0
            self._apply(np.zeros(0, np.int64), ix.num_docs, ix.indptr, ix.indices, ix.tf, self._dl.copy(), first=True)
            return
        _ffi.check(_ffi.lib().vf_bm25_create(ix.indptr.ctypes.data_as(_ffi.p_i64), int(ix.indptr.size - 1),
                                             ix.indices.ctypes.data_as(_ffi.p_i32), ix.data.ctypes.data_as(_ffi.p_f32),
                                             int(ix.data.size), int(ix.num_docs), int(device_id), _ffi.ctypes.byref(self._h),
                                             _ffi.ctypes.byref(slots)), "vf_bm25_create")
        self._info["slots"] = slots.value

    # -- the live index ------------------------------------------------------------------------------------------------------
    def _live_call(self, delta, phase: int, slots=None) -> None:
        _ffi.check(_ffi.lib().vf_bm25_create(_ffi.ctypes.cast(_ffi.ctypes.byref(delta), _ffi.p_i64), 0, None, None, 0, 0,
                                             self._device | phase, _ffi.ctypes.byref(self._h),
                                             _ffi.ctypes.byref(slots) if slots is not None else None), "vf_bm25_create")

    def _need_live(self) -> None:
        if not self.live:
            raise ValueError("this BM25Retriever is not live: construct it with live=True (from a directory that has "
                             f"{FILES['tf']}) to add or remove documents")

    def _apply(self, remove_ids, n_new: int, d_indptr, d_rows, d_tf, new_dl, first: bool = False) -> int:
        """One update: the ids leave, then the delta CSC's ``n_new`` documents (lengths ``new_dl``) are appended.  Two device calls
        with numpy's log between them: idf is computed HERE by ``bm25_index_arrays``' own expression from the counts the stage
        returns, because a device log need not agree with numpy's in the last bit.  Host state changes only after the commit."""
        self._need_live()
        remove_ids = np.ascontiguousarray(remove_ids, dtype=np.int64).ravel()
        d_indptr = np.ascontiguousarray(d_indptr, dtype=np.int64)
        d_rows, d_tf = np.ascontiguousarray(d_rows, dtype=np.int32), np.ascontiguousarray(d_tf, dtype=np.int32)
        Vn = int(d_indptr.size - 1)
        if not first:
            bad = np.flatnonzero((remove_ids < 0) | (remove_ids >= self.num_docs))
            if bad.size:
                raise ValueError(f"remove ids[{int(bad[0])}] = {int(remove_ids[bad[0]])} is outside 0 .. {self.num_docs - 1}; nothing changed")
            if self.num_docs - np.unique(remove_ids).size + int(n_new) < 1:
                raise ValueError("the update would leave no document (a BM25 index holds at least one); nothing changed")
        counts = np.zeros(Vn, np.int64)
        delta, slots = _ffi.Bm25Delta(), _ffi.c_i32()
        delta.vocab, delta.n_new, delta.n_remove, delta.chunk = Vn, int(n_new), int(remove_ids.size), self._chunk
        delta.indptr, delta.rows, delta.tf = d_indptr.ctypes.data_as(_ffi.p_i64), d_rows.ctypes.data_as(_ffi.p_i32), d_tf.ctypes.data_as(_ffi.p_i32)
        delta.remove, delta.counts = remove_ids.ctypes.data_as(_ffi.p_i64), counts.ctypes.data_as(_ffi.p_i64)
        with self._mu:
            if not first and not self._h.value:
                raise RuntimeError("BM25Retriever is closed")
            t0 = time.perf_counter()
            self._live_call(delta, _ffi.VF_BM25_LIVE)
            t1 = time.perf_counter()
            gone = np.unique(remove_ids)
            new_dl = np.asarray(new_dl, np.int64)
            dl = new_dl if first else np.concatenate([np.delete(self._dl, gone), new_dl])
            total = int(new_dl.sum()) + (0 if first else self._total - int(self._dl[gone].sum()))
            N = int(dl.size)
            df = counts.astype(np.float64)
            idf = np.ascontiguousarray(np.log(1.0 + (N - df + 0.5) / (df + 0.5)))      # as bm25_index_arrays
            avgdl = total / N   # = float(dl.mean()): numpy's float64 sum of these integers is exact below 2^53, then one division
            delta.idf, delta.avgdl = idf.ctypes.data_as(_ffi.ctypes.POINTER(_ffi.ctypes.c_double)), (avgdl if avgdl > 0 else 1.0)
            delta.k1, delta.b = self._k1, self._b
            t2 = time.perf_counter()
            self._live_call(delta, _ffi.VF_BM25_COMMIT, slots)
            # where the call's time went (tools/bench_bm25_live.py): stage = upload, row map, count, scan, counts back; host = idf and avgdl
            self.last_update_ms = {"stage": 1e3 * (t1 - t0), "host": 1e3 * (t2 - t1), "commit": 1e3 * (time.perf_counter() - t2)}
            self._retire_subsets()   # the commit invalidated every prepared filter on the device: rows have moved
            self._dl, self._df, self._total = dl, counts, total
            self.num_docs = self.doc_len = N
            self._info = {"n_docs": N, "vocab": Vn, "nnz": int(counts.sum()), "slots": slots.value}
        return int(delta.n_removed)

    def _delta_csc(self, doc_offsets, token_ids, vocab_size: int):
        """The new documents' CSC over ``vocab_size`` columns: (indptr, local rows, tf, lengths) -- ``bm25_index_arrays``' own pairing."""
        off = np.asarray(doc_offsets, dtype=np.int64)
        tok = np.asarray(token_ids, dtype=np.int64)
        if off.ndim != 1 or off.size < 1 or off[0] != 0 or off[-1] != tok.size or np.any(np.diff(off) < 0):
            raise ValueError("doc_offsets must be non-decreasing, start at 0 and end at len(token_ids)")
        m = int(off.size - 1)
        if tok.size and (tok.min() < 0 or tok.max() >= vocab_size):
            raise ValueError("token ids must lie in [0, vocab_size)")
        dl = np.diff(off)
        pair, tf = np.unique(tok * max(m, 1) + np.repeat(np.arange(m, dtype=np.int64), dl), return_counts=True)
        col, row = pair // max(m, 1), pair % max(m, 1)
        indptr = np.zeros(vocab_size + 1, dtype=np.int64)
        np.cumsum(np.bincount(col, minlength=vocab_size), out=indptr[1:])
        return indptr, row.astype(np.int32), tf.astype(np.int32), dl

    def _update_ids(self, remove_ids, doc_offsets, token_ids, vocab_size: int, new_vocab: dict, new_corpus) -> int:
        self._need_live()
        with self._update_mu:
            n0 = self.num_docs
            if len(doc_offsets) <= 1 and np.asarray(remove_ids).size == 0:
                return n0   # nothing leaves and nothing arrives: no rewrite of the index
            indptr, rows, tf, dl = self._delta_csc(doc_offsets, token_ids, max(int(vocab_size), self._info["vocab"]))
            removed = self._apply(remove_ids, int(dl.size), indptr, rows, tf, dl)
            self.vocab.update(new_vocab)
            if self.corpus is not None:
                gone = set(int(i) for i in np.asarray(remove_ids, dtype=np.int64).ravel())
                self.corpus = [c for i, c in enumerate(self.corpus) if i not in gone] + list(new_corpus)
            return n0 - removed

    def _tokens_of(self, texts):
        """(doc_offsets, column ids, {new token: column}) of ``texts`` by this retriever's tokeniser; unknown tokens get new columns."""
        new_vocab: dict = {}
        nxt = self._info["vocab"]
        offsets, ids = [0], []
        for text in texts:
            for w in tokenize(text, self._stem, self._stopwords):
                c = self.vocab.get(w)
                if c is None:
                    c = new_vocab.get(w)
                    if c is None:
                        c = new_vocab[w] = nxt
                        nxt += 1
                ids.append(c)
            offsets.append(len(ids))
        return offsets, np.asarray(ids, dtype=np.int64), new_vocab, nxt

    def update(self, remove_ids, texts, doc_ids=None) -> int:
        """Remove ``remove_ids`` and append ``texts`` in ONE pass over the index (an amended filing); returns the first new id.
        ``doc_ids`` go to ``corpus`` (default: None per text).  A refused update (an id out of range, no document left) raises
        and changes nothing."""
        texts = list(texts)
        doc_ids = [None] * len(texts) if doc_ids is None else list(doc_ids)
        if len(doc_ids) != len(texts):
            raise ValueError("doc_ids must have one entry per text")
        self._need_live()
        with self._update_mu:
            offsets, ids, new_vocab, vocab_size = self._tokens_of(texts)
            return self._update_ids(remove_ids, offsets, ids, vocab_size, new_vocab, doc_ids)

    def add_texts(self, texts, doc_ids=None) -> int:
        """Append ``texts`` (tokenised with this retriever's stemmer and stopwords); returns the first new id."""
        return self.update([], texts, doc_ids)

    def add_token_ids(self, doc_offsets, token_ids, remove_ids=()) -> int:
        """Append documents given as token columns (``build_bm25_index_from_ids``' arguments); a column past the vocabulary is
        new and is named ``t<i>``.  ``remove_ids`` leave in the same pass.  Returns the first new id."""
        self._need_live()
        tok = np.asarray(token_ids, dtype=np.int64)
        with self._update_mu:
            V0 = self._info["vocab"]
            V = max(V0, int(tok.max()) + 1) if tok.size else V0
            new_vocab = {f"t{i}": i for i in range(V0, V) if f"t{i}" not in self.vocab}
            return self._update_ids(remove_ids, doc_offsets, tok, V, new_vocab, [None] * (len(doc_offsets) - 1))

    def remove(self, ids) -> int:
        """Remove documents by id (duplicates count once): later rows move down.  Returns how many left."""
        with self._update_mu:
            n0 = self.num_docs
            self._update_ids(ids, [0], [], 0, {}, [])
            return n0 - self.num_docs

    def arrays(self):
        """The live index as it stands on the device: (indptr int64 [V + 1], indices int32, data float32, tf int32)."""
        self._need_live()
        with self._mu:
            if not self._h.value:
                raise RuntimeError("BM25Retriever is closed")
            V, nnz = self._info["vocab"], self._info["nnz"]
            indptr, indices = np.zeros(V + 1, np.int64), np.zeros(nnz, np.int32)
            data, tf = np.zeros(nnz, np.float32), np.zeros(nnz, np.int32)
            delta = _ffi.Bm25Delta()
            delta.out_indptr, delta.out_indices = indptr.ctypes.data_as(_ffi.p_i64), indices.ctypes.data_as(_ffi.p_i32)
            delta.out_data, delta.out_tf = data.ctypes.data_as(_ffi.p_f32), tf.ctypes.data_as(_ffi.p_i32)
            self._live_call(delta, _ffi.VF_BM25_FETCH)
        return indptr, indices, data, tf

    def save(self, save_dir: str) -> str:
        """Download the live index and write a directory a restart can open, live or not."""
        indptr, indices, data, tf = self.arrays()
        return _write_index(save_dir, indptr, indices, data, dict(self.vocab), self.num_docs, self._k1, self._b, self.corpus, tf=tf)

    def query_columns(self, query: str) -> np.ndarray:
        """The query's token columns in order (repeats kept, unknown tokens dropped), int32."""
        v = self.vocab
        return np.asarray([v[w] for w in tokenize(query, self._stem, self._stopwords) if w in v], dtype=np.int32)

    def _need_subset_stats(self, subset, stats: str) -> bool:
        """True for ``stats="subset"``; refuses a value that is neither mode, the mode without rows and a retriever that is not live."""
        if stats not in ("corpus", "subset"):
            raise ValueError(f"stats={stats!r}: 'corpus' (the whole index's N, df and mean length) or 'subset' (the allowed rows' own)")
        if stats == "corpus":
            return False
        if subset is None:
            raise ValueError("stats='subset' needs subset=: the statistics are those of the rows that may be returned")
        if not self.live:
            raise ValueError("stats='subset' needs a live retriever, BM25Retriever(dir, live=True): only it keeps the term "
                             "frequencies and the document lengths on the device")
        return True

    @staticmethod
    def _columns_args(columns):
        cols = [np.asarray(c, dtype=np.int32).ravel() for c in columns]
        offsets = np.zeros(len(cols) + 1, dtype=np.int64)
        np.cumsum([c.size for c in cols], out=offsets[1:])
        terms = np.ascontiguousarray(np.concatenate(cols) if cols else np.zeros(0, np.int32), dtype=np.int32)
        return cols, offsets, terms

    def _search(self, q, terms, nq: int, k: int, ids=None, scores=None) -> int:
        """``vf_bm25_search`` (``self._mu`` held) -> its code.  ``q``: the query offsets' pointer, or the struct ``nq``'s flags announce."""
        if isinstance(q, _ffi.ctypes.Structure):
            q = _ffi.ctypes.cast(_ffi.ctypes.byref(q), _ffi.p_i64)
        return _ffi.lib().vf_bm25_search(self._h, q, None if terms is None else terms.ctypes.data_as(_ffi.p_i32), nq, k,
                                         None if ids is None else ids.ctypes.data_as(_ffi.p_i64), None if scores is None else scores.ctypes.data_as(_ffi.p_f32))

    def _substats_stage(self, sq, terms, nq: int) -> np.ndarray:
        """The stage call (``self._mu`` held): fills sq.m, sq.total_len and sq.generation, returns df per q_terms position."""
        df = np.zeros(max(int(terms.size), 1), np.int64)
        sq.phase, sq.df = _ffi.VF_BM25_SUBSTATS_STAGE, df.ctypes.data_as(_ffi.p_i64)
        _ffi.check(self._search(sq, terms, nq | _ffi.VF_BM25_FILTER | _ffi.VF_BM25_SUBSTATS, 1), "vf_bm25_search")
        return df[:terms.size]

    @staticmethod
    def _subset_idf_avgdl(m: int, df, total_len: int):
        """(idf per entry of ``df``, avgdl) of ``m`` rows holding ``total_len`` tokens: ``bm25_index_arrays``' expression with N = m; 1.0 for no token."""
        df = df.astype(np.float64)
        idf = np.ascontiguousarray(np.log(1.0 + (m - df + 0.5) / (df + 0.5)))
        return idf, (float(int(total_len)) / m if m and total_len else 1.0)

    # The attribute ``subset_statistics`` declares that ``invoke`` takes stats="subset" (EnsembleRetriever(where_statistics="subset") asks
    # for a truthy one; a retriever of another make sets ``subset_statistics = True``).  Here it is the method that exposes the counts.
    def subset_statistics(self, subset, columns):
        """(m, total_len, df): the rows ``subset`` allows, the tokens they hold, and per query of ``columns`` an int64 array with, for
        each token position, the allowed postings of its column -- what ``stats="subset"`` scores by, counted on the device (the
        stage call alone)."""
        self._need_subset_stats(subset, "subset")
        cols, offsets, terms = self._columns_args(columns if len(columns) else [np.zeros(0, np.int32)])
        with self._update_mu, self._mu:
            if not self._h.value:
                raise RuntimeError("BM25Retriever is closed")
            words, _ = filter_words(subset, self.num_docs)
            sq = _ffi.Bm25SubstatsQuery(offsets.ctypes.data_as(_ffi.p_i64), words.ctypes.data_as(_ffi.ctypes.POINTER(_ffi.ctypes.c_uint32)), self.num_docs)
            df = self._substats_stage(sq, terms, len(cols))
        return int(sq.m), int(sq.total_len), [df[offsets[i]:offsets[i + 1]].copy() for i in range(len(columns))]

    # -- prepared filters ------------------------------------------------------------------------------------------------------
    def _prepared_call(self, pq, phase: int) -> int:
        """A prepare, arm or release call (``self._mu`` held); returns the code."""
        pq.phase = phase
        return self._search(pq, None, _ffi.VF_BM25_PREPARED, 1)

    def _release_token(self, token: int) -> None:
        if self._h.value:
            pq = _ffi.Bm25PreparedQuery()
            pq.token = int(token)
            self._prepared_call(pq, _ffi.VF_BM25_PREPARED_RELEASE)   # a token the device no longer knows is no failure here

    def _drop_orphans(self) -> None:
        """Release what collected ``BM25Subset``s left behind (``self._mu`` held)."""
        while self._orphans:
            self._release_token(self._orphans.pop())

    def _retire_subsets(self) -> None:
        """After a committed update (``self._mu`` held): every prepared filter is stale -- the device has freed it -- and is forgotten."""
        for s in list(self._subsets.values()):
            s._stale, s.nbytes = True, 0
            self._release_token(s._token)
        self._subsets.clear()
        self._drop_orphans()

    def _release_subset(self, s: "BM25Subset") -> None:
        with self._mu:
            if s._closed:
                return
            s._closed, s.nbytes = True, 0
            if not s._stale:
                self._subsets.pop(s._token, None)
                self._release_token(s._token)

    def prepare_subset(self, subset, stats: str = "corpus") -> BM25Subset:
        """Keep a filter on the device: ``subset`` (``filter_words``' argument) is packed, checked and uploaded ONCE, and the returned
        ``BM25Subset`` is passed as ``subset=`` to ``search_columns`` / ``invoke`` / ``invoke_batch`` any number of times; each such
        search is one device call that uploads only its query and returns, bit for bit, what the same call with the rows and this
        ``stats`` returns.  stats="subset" (a live retriever): the device also sums the allowed rows' lengths and counts their postings
        for EVERY column of the vocabulary in one pass over the index (``.df``), numpy takes the logarithm over the vocabulary (the
        builder's own line) and the idf table goes back to the device (prepare, log, arm -- under the update lock, so that no update
        lands in between).  A live retriever's ``live_chunk`` is also the number of postings one workgroup of that count takes.
        The object is stale after this retriever's next update; ``close()`` it (or use ``with``) when the filter is no longer needed."""
        if isinstance(subset, BM25Subset):
            raise TypeError("prepare_subset takes rows (ids, a boolean mask or a RowSubset), not a BM25Subset")
        if subset is None:
            raise ValueError("prepare_subset needs the rows that may be returned")
        by_subset = self._need_subset_stats(subset, stats)
        with self._update_mu, self._mu:
            if not self._h.value:
                raise RuntimeError("BM25Retriever is closed")
            self._drop_orphans()
            t0 = time.perf_counter()
            words, _ = filter_words(subset, self.num_docs)
            V = self._info["vocab"]
            pq = _ffi.Bm25PreparedQuery()
            pq.allow, pq.n_docs = words.ctypes.data_as(_ffi.ctypes.POINTER(_ffi.ctypes.c_uint32)), self.num_docs
            pq.mode = _ffi.VF_BM25_PREPARED_SUBSET if by_subset else _ffi.VF_BM25_PREPARED_CORPUS
            df = None
            if by_subset:
                df = np.zeros(max(V, 1), np.int64)
                pq.vocab, pq.df, pq.chunk = V, df.ctypes.data_as(_ffi.p_i64), self._chunk
            t1 = time.perf_counter()
            _ffi.check(self._prepared_call(pq, _ffi.VF_BM25_PREPARED_PREPARE), "vf_bm25_search")
            t2 = t3 = time.perf_counter()
            if by_subset:
                df = df[:V]
                idf, pq.avgdl = self._subset_idf_avgdl(int(pq.m), df, pq.total_len)
                pq.idf = idf.ctypes.data_as(_ffi.ctypes.POINTER(_ffi.ctypes.c_double))
                pq.k1, pq.b = self._k1, self._b
                t3 = time.perf_counter()
                rc = self._prepared_call(pq, _ffi.VF_BM25_PREPARED_ARM)
                if rc != _ffi.VF_OK:
                    msg = _ffi.last_error()
                    self._release_token(pq.token)
                    raise RuntimeError(f"vf_bm25_search failed (rc={rc}): {msg}")
            # where the time went (tools/bench_bm25_prepared.py): pack = the bitmap; prepare = its upload and, in subset mode, the two
            # counts and their way back; host = the logarithm over the vocabulary; arm = the idf table's upload
            self.last_prepare_ms = {"pack": 1e3 * (t1 - t0), "prepare": 1e3 * (t2 - t1), "host": 1e3 * (t3 - t2), "arm": 1e3 * (time.perf_counter() - t3)}
            s = BM25Subset(self, pq.token, stats, pq.m, pq.total_len if by_subset else 0, pq.generation, df, pq.bytes)
            self._subsets[s._token] = s
            return s

    def _prepared_mode(self, subset: BM25Subset, stats) -> None:
        if subset._retriever is not self:
            raise ValueError("subset: this BM25Subset was prepared on another BM25Retriever; prepare it on this one (prepare_subset)")
        if stats is not _STATS_UNSET and stats != subset.stats:
            raise ValueError(f"stats={stats!r} beside a BM25Subset prepared with stats={subset.stats!r}: the mode is the object's own; "
                             "leave stats= out, or prepare another one")

    def _search_per_query(self, columns, k: int, subsets):
        """``search_columns(columns, k, subsets=[...])``: the prepared filter of every query by its token, 0 for None (VF_BM25_PREPARED_PER_QUERY)."""
        cols, offsets, terms = self._columns_args(columns)
        nq, k = len(cols), int(k)
        subsets = list(subsets)
        if len(subsets) != nq:
            raise ValueError(f"subsets: {len(subsets)} entries for {nq} queries; one BM25Subset or None per query")
        for i, s in enumerate(subsets):
            if s is None:
                continue
            if not isinstance(s, BM25Subset):
                raise TypeError(f"subsets[{i}]: a BM25Subset (prepare_subset) or None, not {type(s).__name__}; rows that were not prepared go to subset=, one set per call")
            if s._retriever is not self:
                raise ValueError(f"subsets[{i}]: this BM25Subset was prepared on another BM25Retriever; prepare it on this one (prepare_subset)")
        if all(s is None for s in subsets):
            return self.search_columns(columns, k)
        with self._mu:
            for i, s in enumerate(subsets):   # before k: an object may have been made for another document count
                if s is not None and (s._closed or s._stale):
                    raise ValueError(f"subsets[{i}]: this BM25Subset " + ("is closed" if s._closed else "is stale (the retriever was updated "
                                     f"after it was prepared at generation {s.generation})") + ": call prepare_subset again")
            if not 1 <= k <= self.num_docs:
                raise ValueError(f"k={k}: must be in [1, {self.num_docs}] (the number of documents)")
            ids = np.empty((nq, k), dtype=np.int64)
            scores = np.empty((nq, k), dtype=np.float32)
            if not self._h.value:
                raise RuntimeError("BM25Retriever is closed")
            tokens = np.asarray([0 if s is None else s._token for s in subsets], dtype=np.uint64)
            pq = _ffi.Bm25PreparedQuery()
            pq.q_offsets, pq.phase, pq.mode = offsets.ctypes.data_as(_ffi.p_i64), _ffi.VF_BM25_PREPARED_SEARCH, _ffi.VF_BM25_PREPARED_PER_QUERY
            pq.tokens = tokens.ctypes.data_as(_ffi.ctypes.POINTER(_ffi.ctypes.c_uint64))
            _ffi.check(self._search(pq, terms, nq | _ffi.VF_BM25_PREPARED, k, ids, scores), "vf_bm25_search")
        return ids, scores

    def search_columns(self, columns: Sequence[np.ndarray], k: int, subset=None, stats=_STATS_UNSET, subsets=None):
        """Token-column lists -> (ids int64 [nq, k], scores float32 [nq, k]) in one device call.  subset (``filter_words``' argument):
        one set of rows for all the queries; with m rows allowed and k > m the ranks m .. k - 1 are padding, id -1 and score -FLT_MAX.
        stats="subset" (a live retriever, with ``subset``; default "corpus"): scored by the allowed rows' own N, df and mean length -- bit
        for bit what a retriever over ``bm25_index_arrays`` of those documents alone returns, its rows mapped back.  Two device calls (the
        counts, then the search) with numpy's log between them, as an update, and under the update lock, so that no update lands between
        them.  subset=<a ``BM25Subset``> (``prepare_subset``): the same results from ONE call that uploads only the query; the mode is
        the object's own (``stats=`` beside it must be absent or equal), a stale or closed one is a ValueError.
        subsets=[...] (in place of ``subset``): one entry per query, a ``BM25Subset`` of this retriever or None -- a batch whose queries
        belong to different tenants, still ONE device call that uploads only the queries and a token each.  Row i is, ids and score bits,
        what ``search_columns([columns[i]], k, subset=subsets[i])`` returns (the plain call for None); corpus-mode, subset-mode and
        unfiltered queries may be mixed, the mode is each object's own.  ``subset=`` or ``stats=`` beside it, a wrong length, an entry of
        another retriever and a closed or stale entry are ValueErrors that name the position; all None is the plain call."""
        if subsets is not None:
            if subset is not None:
                raise ValueError("subset= and subsets= together: one set of rows for the whole batch, or one prepared filter per query")
            if stats is not _STATS_UNSET:
                raise ValueError(f"stats={stats!r} beside subsets=: the mode is each BM25Subset's own; leave stats= out")
            return self._search_per_query(columns, k, subsets)
        prepared = isinstance(subset, BM25Subset)
        if prepared:
            self._prepared_mode(subset, stats)
            by_subset = False
        else:
            stats = "corpus" if stats is _STATS_UNSET else stats
            by_subset = self._need_subset_stats(subset, stats)
        cols, offsets, terms = self._columns_args(columns)
        nq, k = len(cols), int(k)
        with (self._update_mu if by_subset else _NO_LOCK), self._mu:   # the check of k included: a live retriever's update changes the count
            if prepared and (subset._closed or subset._stale):   # before k: the object may have been made for another document count
                raise ValueError("subset: this BM25Subset " + ("is closed" if subset._closed else "is stale (the retriever was updated "
                                 f"after it was prepared at generation {subset.generation})") + ": call prepare_subset again")
            if not 1 <= k <= self.num_docs:
                raise ValueError(f"k={k}: must be in [1, {self.num_docs}] (the number of documents)")
            ids = np.empty((nq, k), dtype=np.int64)
            scores = np.empty((nq, k), dtype=np.float32)
            if nq == 0:
                return ids, scores
            if not self._h.value:
                raise RuntimeError("BM25Retriever is closed")
            q_arg = offsets.ctypes.data_as(_ffi.p_i64)
            if prepared:
                pq = _ffi.Bm25PreparedQuery()
                pq.q_offsets, pq.token, pq.phase = q_arg, subset._token, _ffi.VF_BM25_PREPARED_SEARCH
                _ffi.check(self._search(pq, terms, nq | _ffi.VF_BM25_PREPARED, k, ids, scores), "vf_bm25_search")
                return ids, scores
            if by_subset:
                t0 = time.perf_counter()
                words, _ = filter_words(subset, self.num_docs)
                sq = _ffi.Bm25SubstatsQuery(q_arg, words.ctypes.data_as(_ffi.ctypes.POINTER(_ffi.ctypes.c_uint32)), self.num_docs)
                t1 = time.perf_counter()
                df = self._substats_stage(sq, terms, nq)
                t2 = time.perf_counter()
                idf, sq.avgdl = self._subset_idf_avgdl(int(sq.m), df, sq.total_len)
                sq.idf = idf.ctypes.data_as(_ffi.ctypes.POINTER(_ffi.ctypes.c_double))
                sq.k1, sq.b, sq.phase = self._k1, self._b, _ffi.VF_BM25_SUBSTATS_SEARCH
                t3 = time.perf_counter()
                _ffi.check(self._search(sq, terms, nq | _ffi.VF_BM25_FILTER | _ffi.VF_BM25_SUBSTATS, k, ids, scores), "vf_bm25_search")
                # where the request's time went (tools/bench_bm25_substats.py): pack = the bitmap; host = idf and avgdl
                self.last_subset_ms = {"pack": 1e3 * (t1 - t0), "stage": 1e3 * (t2 - t1), "host": 1e3 * (t3 - t2), "search": 1e3 * (time.perf_counter() - t3)}
                return ids, scores
            if subset is not None:   # packed under the lock: the mask's length is held to the count the device has now
                words, _ = filter_words(subset, self.num_docs)
                q_arg, nq = _ffi.Bm25FilterQuery(q_arg, words.ctypes.data_as(_ffi.ctypes.POINTER(_ffi.ctypes.c_uint32)), self.num_docs), nq | _ffi.VF_BM25_FILTER
            _ffi.check(self._search(q_arg, terms, nq, k, ids, scores), "vf_bm25_search")
        return ids, scores

    def _result(self, ids_row: np.ndarray, scores_row: np.ndarray):
        if ids_row.size and ids_row[-1] < 0:   # a filter of fewer than k rows: the padding is a suffix, and is not returned
            keep = int(np.count_nonzero(ids_row >= 0))
            ids_row, scores_row = ids_row[:keep], scores_row[:keep]
        ids = [int(i) for i in ids_row]
        if self.min_score is not None:
            ids = [i for i, s in zip(ids, scores_row) if s >= self.min_score]
        return ids, scores_row

    def invoke(self, query: str, k: int, metadata_filters=None, subset=None, stats=_STATS_UNSET):
        """(ids, scores) of the k best rows (bm25Retriever.py:50-87); with ``subset`` the k best of those rows, min(k, rows allowed)
        of them, scored by the whole corpus's statistics or, with stats="subset", by those rows' own (``search_columns``).  The retriever holds no metadata: ``metadata_filters`` raises as upstream, ``EnsembleRetriever.rows_where`` turns
        a metadata filter into the rows ``subset`` takes."""
        if metadata_filters:
            raise NotImplementedError("Metadata filtering is not supported yet.")   # as upstream (:69-72)
        ids, scores = self.search_columns([self.query_columns(query)], k, subset=subset, stats=stats)
        return self._result(ids[0], scores[0])

    def invoke_batch(self, queries: Sequence[str], k: int, subset=None, stats=_STATS_UNSET, subsets=None):
        """[(ids, scores)] per query, all in one device call; ``subset``: one set of rows for all of them, ``stats`` as ``search_columns``;
        ``subsets``: a ``BM25Subset`` or None per query (``search_columns``), query i then returns min(k, rows its filter allows) rows."""
        ids, scores = self.search_columns([self.query_columns(q) for q in queries], k, subset=subset, stats=stats, subsets=subsets)
        return [self._result(ids[i], scores[i]) for i in range(len(ids))]

    def info(self) -> dict:
        """n_docs, vocab, nnz, slots: queries one device pass serves, prepared: the ``BM25Subset``s that can search, and
        prepared_bytes: the device memory they hold."""
        alive = [s for s in list(self._subsets.values()) if not s._closed and not s._stale]
        return dict(self._info, prepared=len(alive), prepared_bytes=sum(s.nbytes for s in alive))

    def close(self) -> None:
        mu = getattr(self, "_mu", None)
        if mu is None:
            return
        with mu:
            for s in list(self._subsets.values()):   # the release below frees them on the device: they never touch the library again
                s._closed, s.nbytes = True, 0
            self._subsets.clear()
            del self._orphans[:]
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
