"""FaissRetriever -- drop-in for ``src/utils/faissRetriever.py:8-38`` backed by the HIP index.

Same constructor and ``invoke`` signature and return order as the reference class, so
``EnsembleRetriever`` (``src/utils/ensembleRetriever.py:40,43,66,139``) works unchanged when its
``from .faissRetriever import FaissRetriever`` is pointed here.
"""
from __future__ import annotations

import logging

import numpy as np

from .index import DenseIndex, quantize_int8

logger = logging.getLogger(__name__)


def encode_rows(embeddings: np.ndarray, corpus_dtype: str):
    """[n, d] embeddings -> (the rows as an index of ``corpus_dtype`` holds them, whether they are e4m3 codes): the one recipe of the
    constructor and of ``add_embeddings``, so appended rows are stored exactly as rows given at construction are."""
    if corpus_dtype == "f32":
        return (embeddings if embeddings.dtype == np.float16 else embeddings.astype("float32")), False
    if corpus_dtype == "f16":
        return embeddings.astype(np.float16), False
    if corpus_dtype == "fp8":
        import torch
        # torch's cast to e4m3 does not saturate (|x| > 448 becomes a NaN code) and flushes small magnitudes (the components of a
        # unit vector of 768+ dimensions sit around the subnormal edge 2^-6).  A cosine does not change under a positive per-row
        # scale, so every row is scaled by the POWER OF TWO that puts its largest magnitude into [224, 448]: exact in fp32 (the
        # rounding of in-range values is what it was), nothing can overflow, and the small components keep their three bits
        x = np.ascontiguousarray(embeddings.astype(np.float32))
        if not np.isfinite(x).all():
            raise ValueError("corpus_dtype='fp8': the embeddings hold non-finite values")
        peak = np.abs(x).max(axis=1, keepdims=True).astype(np.float64)
        x = x * np.exp2(np.floor(np.log2(448.0 / np.where(peak > 0, peak, 448.0)))).astype(np.float32)
        np.clip(x, -448.0, 448.0, out=x)
        codes = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        if ((codes & 0x7F) == 0x7F).any():
            raise ValueError("corpus_dtype='fp8': the cast produced NaN codes")
        return codes, True
    if corpus_dtype == "int8":
        try:
            return quantize_int8(embeddings), False
        except ValueError as e:
            raise ValueError(f"corpus_dtype='int8': {e}") from None
    raise ValueError(f"corpus_dtype {corpus_dtype!r}: one of f32, f16, fp8, int8")


class FaissRetriever:
    """Exact cosine retriever; the corpus lives in HBM, search runs as hand-written gfx950 kernels."""

    def __init__(self, embeddings, embedding_fn, device_id: int = 0, device_ids=None, corpus_dtype: str = "f32"):
        # reference :13-24: np.array(embeddings) -> astype('float32') -> normalize_L2 -> IndexFlatIP.add
        self.embeddings = embedding_fn
        embeddings = np.array(embeddings)
        if embeddings.ndim != 2:
            raise ValueError("embeddings must be a 2-D array-like [n, d]")
        dimension = embeddings.shape[1]
        # corpus_dtype (the optional configuration key of SURVEY.md section 5): how the rows are HELD in HBM -- "f32" as faiss holds
        # them (fp16 input stays fp16), "f16" halves the bytes the scan reads, "fp8" (OCP e4m3) quarters them (BASELINE configs[4]),
        # "int8" (quantize_int8: one scale per row, not kept) quarters them too and is about three times closer to the fp32 values.
        # Scores are the canonical cosine of the STORED values either way.
        # device_ids=[0..7]: the corpus is row-sharded over those GPUs behind the same handle (one process, no torchrun)
        # rows_as_given: the index holds the embeddings' own values (nothing was rounded to a narrower type), so a cosine taken from
        # the rows is the cosine of the embeddings (EnsembleRetriever.compute_similarity_mtx serves known texts from them)
        self.rows_as_given = corpus_dtype == "f32" or (corpus_dtype == "f16" and embeddings.dtype == np.float16)
        self.corpus_dtype = corpus_dtype
        rows, e4m3 = encode_rows(embeddings, corpus_dtype)
        make = DenseIndex.from_e4m3 if e4m3 else DenseIndex
        self.index = make(rows, device_id=device_id, device_ids=device_ids)
        logger.info(f"Building HIP dense index with {len(embeddings)} vectors of dimension {dimension}")

    @classmethod
    def from_index(cls, index: DenseIndex, embedding_fn, rows_as_given: bool = True, corpus_dtype: str = None):
        """The same retriever over an index that already exists -- ``DenseIndex.from_file`` (the corpus file the embed loop wrote,
        corpus_file.py: no Chroma round trip at start-up, ensembleRetriever.py:39-43), a device tensor, a sharded group.  Use it as
        ``EnsembleRetriever(..., retriever_cls=lambda _embeddings, fn: FaissRetriever.from_index(ix, fn))``.
        rows_as_given: the index holds the embedder's own values (see __init__).
        corpus_dtype: how that index holds its rows (``f32 | f16 | fp8 | int8``), for ``add_embeddings`` / ``add_texts``: the retriever did
        not build the index, so it appends only when told the recipe the rows were stored with."""
        if corpus_dtype is not None and corpus_dtype not in ("f32", "f16", "fp8", "int8"):
            raise ValueError(f"corpus_dtype {corpus_dtype!r}: one of f32, f16, fp8, int8")
        self = cls.__new__(cls)
        self.embeddings, self.index, self.rows_as_given, self.corpus_dtype = embedding_fn, index, bool(rows_as_given), corpus_dtype
        return self

    def add_embeddings(self, embeddings) -> np.ndarray:
        """Append [m, d] embeddings to the live index (reference: ``index.add(x)`` at :24, which upstream runs once); returns their ids,
        int64 [m].  They are stored by the constructor's recipe for this retriever's ``corpus_dtype``."""
        if getattr(self, "corpus_dtype", None) is None:
            raise ValueError("this retriever wraps an index it did not build: pass corpus_dtype to from_index to append to it")
        embeddings = np.array(embeddings)
        if embeddings.ndim != 2:
            raise ValueError("embeddings must be a 2-D array-like [m, d]")
        rows, _ = encode_rows(embeddings, self.corpus_dtype)
        first = self.index.add(rows)
        return np.arange(first, first + len(rows), dtype=np.int64)

    def add_texts(self, texts) -> np.ndarray:
        """Embed ``texts`` as documents (``embed_documents``; ``embed_query`` per text where that is all the embedder has) and append
        them; returns their ids."""
        texts = list(texts)
        if getattr(self, "corpus_dtype", None) is None:
            raise ValueError("this retriever wraps an index it did not build: pass corpus_dtype to from_index to append to it")
        if not texts:
            return np.empty(0, dtype=np.int64)
        embed_docs = getattr(self.embeddings, "embed_documents", None)
        vectors = embed_docs(texts) if embed_docs is not None else [self.embeddings.embed_query(t) for t in texts]
        return self.add_embeddings(np.asarray(vectors, dtype=np.float32).reshape(len(texts), -1))

    def remove_ids(self, ids) -> int:
        """Remove rows by id (``faiss.IndexFlat.remove_ids``): later rows shift down, so ids stay positions -- delete the same entries
        from any list kept beside the index.  Returns the number removed.  Refused where ``add_embeddings`` is: a retriever that wraps
        an index it did not build changes it only when told how that index holds its rows."""
        if getattr(self, "corpus_dtype", None) is None:
            raise ValueError("this retriever wraps an index it did not build: pass corpus_dtype to from_index to remove from it")
        return int(self.index.remove(np.asarray(ids, dtype=np.int64).ravel()))

    per_query_subsets = True   # invoke takes subsets=[one filter per query] (EnsembleRetriever.invoke_batch asks for this before it batches)

    def invoke(self, querys: list, k: int, subset=None, subsets=None):
        """(I, D) = ids and cosine scores, best first, shape [len(querys), k]; -1 / -FLT_MAX pad a corpus with fewer than k rows
        (reference :28-38: embed each string, fp32, L2-normalise, IndexFlatIP.search).  An embedder with a batched
        ``embed_queries`` -- ours has one -- gets ONE forward for all strings; any other is called per string, as upstream does.
        subset: search these rows only (ids, a boolean mask or a ``RowSubset``: ``DenseIndex.search``) -- the metadata filtering the
        reference class announces and does not have.
        subsets: one entry per string -- ids, a mask, a ``RowSubset`` or None -- passed through to ``DenseIndex.search(subsets=)``: row i
        is what ``invoke([querys[i]], k, subset=subsets[i])`` returns.  Entries that are the same object share one list."""
        texts = list(querys)
        embed_many = getattr(self.embeddings, "embed_queries", None)
        vectors = embed_many(texts) if embed_many is not None else [self.embeddings.embed_query(t) for t in texts]
        q = np.asarray(vectors, dtype=np.float32).reshape(len(texts), -1)
        if subsets is not None:
            ids, scores = self.index.search(q, k, subset=subset, subsets=subsets)
        elif subset is None:
            ids, scores = self.index.search(q, k)      # normalisation happens on the device (k_prep_queries), canonical order
        else:
            ids, scores = self.index.search(q, k, subset=subset)
        return ids, scores
