"""Candidate gathering around the dense search: ``EnsembleRetriever`` with the reference's constructor and
``invoke(input, hyde_chunks) -> list[dict]`` (``src/utils/ensembleRetriever.py:19-48`` ctor, ``:50-232`` invoke).

What the reference does per hit with an O(N) scan over every chunk's metadata -- "all rows of this bundle"
(``:77-82,155-160,203-208``) and "all rows whose title summary is this string" (``:144``) -- is answered here from
three maps built once at construction: ``bundle_id -> rows`` (ascending row order, as the scan yields them),
``title_summary -> rows`` and ``doc_id -> row`` (the reference's ``docid2idx``, ``:45``).  The dense searches go
through this package's ``FaissRetriever`` (GPU).  Output schema, ordering, the ``seen_ids`` bookkeeping, the
neighbour expansion (score > 0.72, neighbours > 0.66 in the 2048-deep score map, at most 4 rows, ``:85-107``) and
the running ``bundle_id`` counter are the reference's.

BM25: the constructor does what the reference's does (``:37``) -- it builds the host application's own
``BM25Retriever(bm25_dir)`` -- unless an object with ``invoke(query, k) -> (ids, scores)`` (``src/utils/bm25Retriever.py:50-87``)
is handed in as ``bm25_retriever``; this package's GPU one is ``bm25_retriever=veritasfi_amd.BM25Retriever(bm25_dir)`` (bm25.py).  When the BM25 branch is on (``bm25_k`` resolves
to > 0) and neither works, construction FAILS; the branch is never dropped silently.  The stores are anything with
Chroma's ``get(include=[...])`` / ``get(ids=[...], include=[...])``.
"""
from __future__ import annotations

import importlib
import threading
from collections import OrderedDict
from typing import Dict, List

import numpy as np

from . import stages
from . import where as vf_where
from .faiss_retriever import FaissRetriever
from .similarity import _embed_all, compute_similarity, compute_similarity_mtx

EXPAND_SCORE, NEIGHBOUR_SCORE, MAX_EXPANDED, SEARCH_DEPTH = 0.72, 0.66, 4, 2048
# where the host application's BM25Retriever lives, as seen from its entry points (src/ on sys.path, or the repo root)
BM25_MODULES = ("utils.bm25Retriever", "src.utils.bm25Retriever", "bm25Retriever")
TEXT_ROWS_KEPT = 65536   # chunk texts whose corpus row is remembered (a request emits tens to ~155)


class _TextRows:
    """chunk text -> corpus row, for the texts this retriever has emitted (bounded, least recently emitted first out).
    Request threads share a retriever without a lock upstream (ragManager.py:17-30), so this has its own."""

    def __init__(self, cap: int = TEXT_ROWS_KEPT):
        self._cap, self._map, self._mu = cap, OrderedDict(), threading.Lock()

    def remember(self, texts, rows) -> None:
        with self._mu:
            for text, row in zip(texts, rows):
                if row is None or row < 0:
                    continue
                self._map[text] = row
                self._map.move_to_end(text)
            while len(self._map) > self._cap:
                self._map.popitem(last=False)

    def rows_of(self, texts) -> List[int]:
        with self._mu:
            return [self._map.get(t, -1) for t in texts]


def _host_bm25(bm25_dir):
    """``BM25Retriever(bm25_dir)`` of the application this class is dropped into (ensembleRetriever.py:13,37)."""
    tried = []
    for name in BM25_MODULES:
        try:
            mod = importlib.import_module(name)
        except ImportError as e:
            tried.append(f"{name}: {e}")
            continue
        return mod.BM25Retriever(bm25_dir)
    raise ImportError("EnsembleRetriever: the BM25 branch is on (bm25_k > 0) but no BM25Retriever is importable ("
                      + "; ".join(tried) + ") -- pass bm25_retriever=<object with invoke(query, k)>, or bm25_k=0 to "
                      "switch the branch off explicitly")


class PreparedWhere:
    """A metadata filter prepared ONCE for many ``EnsembleRetriever.invoke(..., where=<this object>)`` calls (``prepare_where``): the
    same ``where`` on thousands of consecutive requests (one tenant) need not be looked up, turned into a set and shipped to both legs
    per request.  It holds ``where`` itself, the passing rows (``passing``, ``rows_where``'s answer), their set (``allow``), for the dense
    leg a device-resident ``RowSubset`` when the retriever's index is a single-device handle that offers ``row_subset`` (else the ids),
    and for the BM25 leg a ``BM25Subset`` (``prepare_subset(passing, stats=where_statistics)``) when the retriever offers
    ``prepare_subset`` (else the ids).
    It holds MEANING, not rows: after ``add_documents`` / ``remove_documents`` rows have shifted and metadata has changed, but the dict
    still means what it meant, so the next use re-prepares it from ``where`` (releasing the old device objects).  The lower-level
    ``BM25Subset`` and ``RowSubset`` hold rows and keep refusing when stale.  ``close()`` (or ``with``) releases both legs."""

    def __init__(self, retriever, where):
        if not isinstance(where, dict):
            raise TypeError("prepare_where: `where` is a dict field -> value, or field -> a collection of values")
        self._retriever, self.where = retriever, dict(where)
        self._mu = threading.Lock()
        self._closed, self._epoch = False, None
        self.passing = self.allow = self.dense = self.bm25 = None
        with self._mu:
            self._prepare()

    def _release(self) -> None:
        bm, self.bm25, self.dense = self.bm25, None, None   # a RowSubset's device ids go with its last reference
        if hasattr(bm, "close"):
            bm.close()

    def _prepare(self) -> None:
        r = self._retriever
        self._release()
        evaluated = None
        if vf_where.has_operators(self.where):   # the operator grammar: evaluated on the device where the index offers it
            self.passing, self.allow, evaluated = r._eval_where(self.where)
        else:
            self.passing = r.rows_where(self.where)
            self.allow = set(self.passing.tolist())
        self.dense = self.bm25 = self.passing
        self._epoch = r._epoch
        if self.passing.size == 0:      # invoke returns [] before any leg is asked
            return
        ix = getattr(r.faiss_retriever, "index", None)
        if evaluated is not None:       # the evaluation left the ids on the device: nothing to upload
            self.dense = evaluated
        elif r.faiss_k > 0 and hasattr(ix, "row_subset") and getattr(ix, "device_ids", None) is None:
            self.dense = ix.row_subset(self.passing)
        bm = r.bm25_retriever
        if r.bm25_k > 0 and hasattr(bm, "prepare_subset"):
            self.bm25 = bm.prepare_subset(self.passing, stats=r.where_statistics)

    def _current(self, retriever):
        """(passing, allow, dense subset, BM25 subset) for a request of ``retriever``, prepared again if the corpus has changed."""
        if retriever is not self._retriever:
            raise ValueError("where: this PreparedWhere was prepared on another EnsembleRetriever; use that retriever's prepare_where")
        with self._mu:
            if self._closed:
                raise ValueError("where: this PreparedWhere is closed; call prepare_where again")
            if self._epoch != retriever._epoch:
                self._prepare()
            return self.passing, self.allow, self.dense, self.bm25

    def close(self) -> None:
        with self._mu:
            if not self._closed:
                self._closed = True
                self._release()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class EnsembleRetriever:
    def __init__(self, bm25_dir, chroma, ts_chroma, k: int, embeddings, faiss_k: int = None, bm25_k: int = None,
                 faiss_ts_k: int = None, enable_expand: bool = False, bm25_retriever=None, retriever_cls=FaissRetriever,
                 prefetch_documents: bool = False, similarity_from_rows: bool = None, where_statistics: str = "corpus"):
        """Positional arguments as upstream (``ragManager.py:112`` passes bm25_dir, chroma, ts_chroma, k, embeddings).
        ``bm25_dir`` goes to the host application's ``BM25Retriever`` exactly as upstream (``:37``) unless
        ``bm25_retriever`` is given.
        ``prefetch_documents=True`` loads every chunk's text once and serves bundles from memory in the requested
        row order instead of one ``chroma.get(ids=...)`` per bundle (Chroma returns rows in ITS order, so leave this
        off when byte-identical ordering inside a bundle matters).
        ``similarity_from_rows``: ``compute_similarity_mtx(texts)`` -- the reference's call, texts only (vllmManager.py:462) --
        serves every text this retriever has emitted from ITS ROW of the HBM-resident corpus (``vf_cosine_matrix_rows_mixed``) and
        embeds only texts it does not know, instead of embedding all n again (ensembleRetriever.py:275).  None (default) = on when
        that is the same matrix: the rows are held as given (not rounded to a narrower ``corpus_dtype``) and the embedder has no
        query instruction (upstream stores ``embed_documents(text)`` and compares ``embed_query(text)``: the same vector unless
        the embedder prefixes queries).  False = always re-embed; True = rows even where auto would decline.
        ``where_statistics``: what the BM25 leg of a filtered request (``invoke(..., where=)``) scores by.  "corpus" (default): the
        whole corpus's N, df and mean length, today's calls.  "subset": the passing chunks' own, so that the BM25 leg too returns what
        an ensemble over the passing chunks alone would; it needs a BM25 retriever that declares ``subset_statistics`` (this package's
        ``BM25Retriever(bm25_dir, live=True)``), whose ``invoke`` is then called with ``stats="subset"``."""
        if where_statistics not in ("corpus", "subset"):
            raise ValueError(f"where_statistics={where_statistics!r}: 'corpus' or 'subset'")
        self.where_statistics = where_statistics
        self._epoch = 0   # advanced by add_documents / remove_documents: a PreparedWhere of an older epoch prepares itself again
        self.embeddings = embeddings
        self.faiss_k = faiss_k if faiss_k is not None else k
        self.bm25_k = bm25_k if bm25_k is not None else k
        self.faiss_ts_k = faiss_ts_k if faiss_ts_k is not None else k
        self.enable_expand = enable_expand
        self.chroma = chroma
        self.bm25_dir = bm25_dir
        self.bm25_retriever = bm25_retriever
        if self.bm25_retriever is None and self.bm25_k > 0:
            self.bm25_retriever = _host_bm25(bm25_dir)
        if where_statistics == "subset" and self.bm25_k > 0:
            bm = self.bm25_retriever
            if not getattr(bm, "subset_statistics", False) or getattr(bm, "live", True) is False:
                raise ValueError("where_statistics='subset' needs a BM25 retriever that declares subset_statistics, i.e. takes "
                                 "invoke(query, k, subset=rows, stats='subset') -- e.g. veritasfi_amd.BM25Retriever(bm25_dir, live=True)")

        include = ["metadatas", "embeddings"] + (["documents"] if prefetch_documents else [])
        docs = chroma.get(include=include)
        self.faiss_retriever = retriever_cls(docs["embeddings"], embeddings)
        ts_docs = ts_chroma.get(include=["documents", "embeddings"])
        self.title_summary_faiss_retriever = retriever_cls(ts_docs["embeddings"], embeddings)

        self.chunk_metadata = docs["metadatas"]
        self.num_chunk = len(self.chunk_metadata)
        self.title_summaries = ts_docs["documents"]
        self._documents = docs["documents"] if prefetch_documents else None
        # the three maps that replace the per-hit scans
        self.docid2idx: Dict[str, int] = {}
        self._bundle_rows: Dict[object, List[int]] = {}
        self._title_rows: Dict[str, List[int]] = {}
        self._build_maps()
        self._text_rows = _TextRows()
        self.similarity_from_rows = self._rows_serve_similarity() if similarity_from_rows is None else bool(similarity_from_rows)

    def _rows_serve_similarity(self) -> bool:
        ix = getattr(self.faiss_retriever, "index", None)
        if ix is None or not hasattr(ix, "cosine_matrix_rows"):
            return False
        if not getattr(self.faiss_retriever, "rows_as_given", False):
            return False
        for name in ("query_instruction", "query_instruction_for_retrieval", "embed_instruction"):
            if getattr(self.embeddings, name, None):
                return False
        return True

    # -- a live corpus --------------------------------------------------------------------------------
    def _build_maps(self) -> None:
        self.docid2idx, self._bundle_rows, self._title_rows = {}, {}, {}
        self._field_rows = {}   # rows_where's per-field dictionaries: built on first use, dropped whenever the corpus changes
        self._where_columns = {}   # ... and the operator grammar's typed key columns (where.WhereColumn), under the same rule
        for row, md in enumerate(self.chunk_metadata):
            self.docid2idx[md["doc_id"]] = row
            b = md.get("bundle_id", None)
            if b is not None:
                self._bundle_rows.setdefault(b, []).append(row)
            self._title_rows.setdefault(md.get("title_summary", ""), []).append(row)

    def _check_live(self, need_bm25: str, need_dense: str) -> None:
        """What can be known to refuse before any leg is asked: the BM25 leg is the live one and in step, the dense retriever has the
        call and -- where it is this package's -- was told how its index holds the rows (``FaissRetriever.from_index`` without
        ``corpus_dtype`` refuses every change)."""
        if self.bm25_retriever is not None:
            bm = self.bm25_retriever
            if not (getattr(bm, "live", False) is True and hasattr(bm, need_bm25)):
                raise ValueError("EnsembleRetriever: the BM25 leg cannot follow an added or removed chunk -- it must be this package's "
                                 "live one, bm25_retriever=veritasfi_amd.BM25Retriever(bm25_dir, live=True)")
            if bm.num_docs != self.num_chunk:
                raise ValueError(f"EnsembleRetriever: the BM25 leg holds {bm.num_docs} documents, the corpus {self.num_chunk}")
        dense = self.faiss_retriever
        if not hasattr(dense, need_dense):
            raise ValueError(f"EnsembleRetriever: the dense retriever has no {need_dense}(): it cannot follow an added or removed chunk")
        if getattr(dense, "corpus_dtype", "") is None:
            raise ValueError("EnsembleRetriever: the dense retriever wraps an index it did not build and was not told how that index "
                             "holds its rows (FaissRetriever.from_index(..., corpus_dtype=...)): it cannot follow an added or removed chunk")

    def add_documents(self, texts, metadatas, embeddings=None) -> List[int]:
        """Append chunks to every leg together; returns their rows (num_chunk .. num_chunk + m - 1 before the call).
        ``embeddings`` [m, d] are the chunks' vectors; without them ``texts`` are embedded here, as ``FaissRetriever.add_texts`` embeds
        them (``embed_documents``, or ``embed_query`` per text).  The BM25 leg tokenises the texts with its own tokeniser;
        ``chunk_metadata``, ``num_chunk``, the prefetched documents and the three maps follow.  Each metadata needs a ``doc_id`` no
        chunk has yet.
        Nothing changes when the call raises.  Checked before any leg is asked: the doc_ids, a BM25 leg that is not this package's
        live one or is out of step, a dense retriever that cannot append, the embedder (it runs first), the vectors' width.  Then the
        dense leg appends -- if IT refuses, nothing has changed -- and the BM25 leg follows; should that fail, the dense leg's new
        rows are removed again (the newest rows: nothing moves) before the error is passed on.
        Chroma itself (``self.chroma``: ``_fetch`` reads new chunks' texts from it unless documents are prefetched) and the
        title-summary index are the caller's: add the chunks to the store first, and a ``title_summary`` the title index does not
        hold is found by the other two branches only."""
        texts, metadatas = list(texts), list(metadatas)
        if len(texts) != len(metadatas):
            raise ValueError("add_documents: one metadata per text")
        if embeddings is not None and len(embeddings) != len(texts):
            raise ValueError("add_documents: one embedding per text")
        ids = [md["doc_id"] for md in metadatas]
        if len(set(ids)) != len(ids) or any(i in self.docid2idx for i in ids):
            raise ValueError("add_documents: a doc_id is repeated or already in the corpus")
        dense = self.faiss_retriever
        by_vectors = hasattr(dense, "add_embeddings")     # a retriever with add_texts alone embeds for itself
        if embeddings is not None and not by_vectors:
            raise ValueError("EnsembleRetriever: the dense retriever has no add_embeddings(): pass the texts without embeddings")
        self._check_live("update", "add_embeddings" if by_vectors else "add_texts")
        first = self.num_chunk
        if not texts:
            return []
        if by_vectors:
            if embeddings is None:
                embed_docs = getattr(self.embeddings, "embed_documents", None)
                embeddings = embed_docs(texts) if embed_docs is not None else [self.embeddings.embed_query(t) for t in texts]
            embeddings = np.asarray(embeddings)
            if embeddings.ndim != 2 or embeddings.shape[0] != len(texts):
                raise ValueError(f"add_documents: embeddings must be [{len(texts)}, d], got {embeddings.shape}")
            d = getattr(getattr(dense, "index", None), "d", None)
            if d is not None and embeddings.shape[1] != d:
                raise ValueError(f"add_documents: embeddings of width {embeddings.shape[1]} for an index of width {d}")
            dense.add_embeddings(embeddings)
        else:
            dense.add_texts(texts)
        if self.bm25_retriever is not None:
            try:
                self.bm25_retriever.update([], texts, doc_ids=ids)
            except Exception:
                if hasattr(dense, "remove_ids"):
                    dense.remove_ids(np.arange(first, first + len(texts), dtype=np.int64))
                raise
        self.chunk_metadata = list(self.chunk_metadata) + metadatas
        self.num_chunk = len(self.chunk_metadata)
        self._field_rows = {}
        self._where_columns = {}
        if self._documents is not None:
            self._documents = list(self._documents) + texts
        for row, md in enumerate(metadatas, start=first):
            self.docid2idx[md["doc_id"]] = row
            b = md.get("bundle_id", None)
            if b is not None:
                self._bundle_rows.setdefault(b, []).append(row)
            self._title_rows.setdefault(md.get("title_summary", ""), []).append(row)
        self._epoch += 1
        return list(range(first, self.num_chunk))

    def remove_documents(self, doc_ids) -> int:
        """Remove chunks by ``doc_id`` from every leg together; later rows move down in all of them (faiss ``remove_ids``), so the
        maps are rebuilt and the remembered text rows forgotten.  Returns the number removed.
        Refused with nothing changed: an unknown ``doc_id``, removing every chunk, a BM25 leg that is not this package's live one or
        is out of step, a dense retriever that cannot remove -- and whatever the dense leg itself refuses (a search in flight, a shard
        of a group that would be emptied), because it is asked FIRST.  The BM25 leg follows with rows that were checked here (in
        range, not all of them), so only a device failure can stop it; a removal cannot be undone in place, so that error is passed
        on as a RuntimeError saying that the legs are out of step and the retriever must be constructed again.
        Chroma itself and the title-summary index are the caller's."""
        doc_ids = list(doc_ids)
        unknown = [i for i in doc_ids if i not in self.docid2idx]
        if unknown:
            raise ValueError(f"remove_documents: unknown doc_id {unknown[0]!r}")
        rows = sorted({self.docid2idx[i] for i in doc_ids})
        if len(rows) >= self.num_chunk and rows:
            raise ValueError("remove_documents: at least one chunk must remain")
        self._check_live("remove", "remove_ids")
        if not rows:
            return 0
        self.faiss_retriever.remove_ids(np.asarray(rows, dtype=np.int64))
        if self.bm25_retriever is not None:
            try:
                self.bm25_retriever.remove(rows)
            except Exception as e:
                raise RuntimeError(f"remove_documents: the dense leg removed {len(rows)} rows and the BM25 leg then failed ({e}): the "
                                   "legs are out of step, construct the EnsembleRetriever again") from e
        gone = set(rows)
        self.chunk_metadata = [md for r, md in enumerate(self.chunk_metadata) if r not in gone]
        self.num_chunk = len(self.chunk_metadata)
        if self._documents is not None:
            self._documents = [t for r, t in enumerate(self._documents) if r not in gone]
        self._build_maps()
        self._text_rows = _TextRows()
        self._epoch += 1
        return len(rows)

    # -- metadata filters -----------------------------------------------------------------------------
    def rows_where(self, where) -> np.ndarray:
        """Sorted row numbers (int64) of the chunks whose metadata passes ``where``: a dict ``field -> value``, or ``field -> a
        collection of values`` (list, tuple, set, frozenset: any of them passes); several fields must all pass.  A chunk without the
        field passes only a filter that lists ``None``.  Served from one dictionary ``value -> rows`` per field, built on the first
        use of that field and dropped by ``add_documents`` / ``remove_documents``.
        A ``where`` with a ``$`` key anywhere speaks Chroma's operator grammar instead (``$eq $ne $gt $gte $lt $lte $in $nin $and $or``:
        veritasfi_amd/where.py has the semantics): the rows are those for which ``where.matches(metadata, where)`` holds, found by a
        compiled program over typed key columns -- on the device when the dense index offers ``eval_where``, else in NumPy."""
        if not isinstance(where, dict):
            raise TypeError("rows_where: `where` is a dict field -> value, or field -> a collection of values")
        if vf_where.has_operators(where):
            return self._eval_where(where)[0]
        rows = None
        for field, want in where.items():
            index = self._field_rows.get(field)
            if index is None:
                index = {}
                for row, md in enumerate(self.chunk_metadata):
                    try:
                        index.setdefault(md.get(field, None), []).append(row)
                    except TypeError:      # an unhashable metadata value (a list): no filter value can equal it
                        pass
                self._field_rows[field] = index
            values = list(want) if isinstance(want, (list, tuple, set, frozenset)) else [want]
            hit = sorted({r for v in values for r in index.get(v, ())})
            hit = np.asarray(hit, dtype=np.int64)
            rows = hit if rows is None else np.intersect1d(rows, hit, assume_unique=True)
        return np.arange(self.num_chunk, dtype=np.int64) if rows is None else rows

    def _where_column(self, field):
        col = self._where_columns.get(field)
        if col is None:
            col = self._where_columns[field] = vf_where.build_column([md.get(field) for md in self.chunk_metadata], field)
        return col

    def _eval_where(self, where):
        """An operator filter's (passing rows, their ``RowMask``, the device-resident ``RowSubset`` or None).  The kind check is the
        columns' construction, so every route raises it alike.  The device evaluates when the dense retriever's index is a
        single-device handle with ``eval_where`` over exactly these chunks and the program fits its limits; NumPy otherwise."""
        columns = {f: self._where_column(f) for f in vf_where.fields_of(where)}
        program = vf_where.compile_where(where, columns, n=self.num_chunk)
        ix = getattr(self.faiss_retriever, "index", None)
        if (program.fits_device and hasattr(ix, "eval_where") and getattr(ix, "device_ids", None) is None
                and getattr(ix, "n", None) == self.num_chunk):
            subset, mask = ix.eval_where(program, columns)
            offset = int(getattr(ix, "id_offset", 0))
            return (subset.ids - offset if offset else subset.ids), mask, subset
        mask = program.evaluate_numpy(columns, self.num_chunk)
        return np.flatnonzero(mask).astype(np.int64), vf_where.RowMask(mask), None

    def prepare_where(self, where) -> PreparedWhere:
        """``where`` (``rows_where``'s argument) prepared once for many ``invoke(..., where=<the returned object>)`` calls: the passing
        rows, their set, the dense leg's device-resident ``RowSubset`` and the BM25 leg's ``BM25Subset`` (under this retriever's
        ``where_statistics``) are computed here and not per request.  The output of ``invoke`` is that of the dict form.  After
        ``add_documents`` / ``remove_documents`` the object prepares itself again on its next use; ``close()`` it when done."""
        return PreparedWhere(self, where)

    # -- pieces -------------------------------------------------------------------------------------
    def _bundle_of(self, row: int, seen: set, allow=None) -> List[int]:
        """Rows emitted for a hit: the whole bundle when the chunk has one (all marked seen), else the row.  allow: the rows a filter
        lets through (a set), or None."""
        b = self.chunk_metadata[row].get("bundle_id", None)
        if b is None:
            return [row]
        rows = [r for r in self._bundle_rows[b] if allow is None or r in allow]
        seen.update(rows)
        return rows

    def _fetch(self, rows: List[int]):
        if self._documents is not None:
            return [self._documents[r] for r in rows], [self.chunk_metadata[r] for r in rows]
        got = self.chroma.get(ids=[self.chunk_metadata[r]["doc_id"] for r in rows], include=["documents", "metadatas"])
        return got["documents"], got["metadatas"]

    def _emit(self, out: list, name: str, score, rows: List[int], bundle_cnt: int) -> None:
        documents, metadatas = self._fetch(rows)
        if self.similarity_from_rows:   # the store answers in ITS order: a text's row comes from its own metadata
            self._text_rows.remember(documents, [self.docid2idx.get(md.get("doc_id"), -1) for md in metadatas])
        for text, md in zip(documents, metadatas):
            out.append({"retriever": name, "score": float(score), "page_content": text, "metadata": md,
                        "bundle_id": bundle_cnt})

    def _expand(self, rows: List[int], hit_md: dict, score_map: dict, seen: set, allow=None) -> None:
        prev_doc, next_doc = hit_md["prev_chunk_id"], hit_md["next_chunk_id"]
        while len(rows) < MAX_EXPANDED:
            grew = False
            p = self.docid2idx.get(prev_doc, -1) if prev_doc != "" else -1
            if allow is not None and p not in allow:     # a store of the passing chunks alone would not know this neighbour
                p = -1
            if p != -1 and score_map.get(p, 0) > NEIGHBOUR_SCORE and p not in seen:
                grew = True
                seen.add(p)
                rows.insert(0, p)
                prev_doc = self.chunk_metadata[p]["prev_chunk_id"]
            n = self.docid2idx.get(next_doc, -1) if next_doc != "" else -1
            if allow is not None and n not in allow:
                n = -1
            if n != -1 and score_map.get(n, 0) > NEIGHBOUR_SCORE and n not in seen:
                grew = True
                seen.add(n)
                rows.append(n)
                next_doc = self.chunk_metadata[n]["next_chunk_id"]
            if not grew:
                break

    # -- the reference's entry point ------------------------------------------------------------------
    def invoke(self, input: str, hyde_chunks: List[str], where=None) -> List[Dict]:
        """Stage brackets as upstream (``"retrieve"`` around the call, one per branch, the ``retrieved_chunks`` metric): no-ops
        unless ``veritasfi_amd.set_profiler`` was given the host's profiler (stages.py).
        where (``rows_where``'s argument; None = no filter, today's call): only chunks whose metadata passes are returned.  The rule:
        the result is what ``invoke`` would return over a store that held the passing chunks alone -- the dense leg searches those
        rows only (``FaissRetriever.invoke(subset=...)``: the retriever must take ``subset``), bundles and the neighbour expansion see
        passing rows only, the title-summary leg's rows are filtered here.  ONE stated exception, under ``where_statistics="corpus"``
        (the default) only, the BM25 leg: it keeps the
        whole corpus's statistics (idf, average length), as upstream's own sketch does (bm25Retriever.py:91-132) -- its result is
        the first ``bm25_k`` passing rows of the full ranking.  Under ``where_statistics="subset"`` there is no exception: the leg is
        asked with ``stats="subset"`` and scores by the passing chunks' own statistics.  A retriever that declares ``filtered_prefix`` (this package's
        ``BM25Retriever``) is asked for exactly those, ``invoke(input, min(bm25_k, passing rows), subset=passing)``, and filters
        inside its kernels, so the exception costs nothing; any other retriever is asked for the full ranking, which is
        filtered here.  A filter nothing passes returns [].  A ``PreparedWhere`` (``prepare_where``) in place of the dict gives the same
        output without the per-request host work: the rows, their set and both legs' device-resident filters are its own."""
        with stages.stage("retrieve"):
            out = self._invoke(input, hyde_chunks, where)
        stages.metric("retrieved_chunks", len(out))
        return out

    def _resolve_where(self, where):
        """(passing, allow, dense filter, BM25 filter) of one request: what the two legs take as subset= is the passing rows, or a
        PreparedWhere's device-resident filters."""
        if isinstance(where, PreparedWhere):
            return where._current(self)
        if isinstance(where, dict) and vf_where.has_operators(where):
            passing, allow, dense = self._eval_where(where)   # the dense leg takes the ids where the evaluation left them
            return passing, allow, passing if dense is None else dense, passing
        passing = None if where is None else self.rows_where(where)
        allow = None if passing is None else set(passing.tolist())
        return passing, allow, passing, passing

    def _invoke(self, input: str, hyde_chunks: List[str], where=None) -> List[Dict]:
        seen: set = set()
        out: list = []
        bundle_cnt = 0
        passing, allow, dense_rows, bm25_rows = self._resolve_where(where)
        if passing is not None and passing.size == 0:
            return out
        if self.faiss_k > 0:
            with stages.stage("retrieve_faiss"):
                bundle_cnt = self._faiss_branch(input, hyde_chunks, seen, out, bundle_cnt, passing, allow, dense_rows)
        if self.faiss_ts_k > 0:
            with stages.stage("retrieve_faiss_ts"):
                bundle_cnt = self._title_branch(input, seen, out, bundle_cnt, allow)
        if self.bm25_k > 0:
            with stages.stage("retrieve_bm25"):
                bundle_cnt = self._bm25_branch(input, seen, out, bundle_cnt, allow, passing, bm25_rows)
        return out

    # Each branch is an ASK (what the leg is called with) and a CONSUME (what is emitted from its answer): invoke runs them back to
    # back, invoke_batch asks once for many requests and consumes per request -- the same consuming code, so the same output.
    def _faiss_depth(self) -> int:
        # upstream always searches 2048 deep (:64-66) and reads the tail only as the neighbour expansion's score map (:85-107): without
        # enable_expand the first faiss_k entries are all that is looked at, and an exact search's top-k is a prefix of its top-2048
        return SEARCH_DEPTH if self.enable_expand else min(SEARCH_DEPTH, max(1, int(self.faiss_k)))

    @staticmethod
    def _dense_filter(passing, dense_rows):
        return passing if dense_rows is None else dense_rows

    def _faiss_ask(self, input, hyde_chunks, passing=None, dense_rows=None):
        inputs = [input] + list(hyde_chunks)
        if passing is None:
            return self.faiss_retriever.invoke(inputs, self._faiss_depth())
        # rows are ids here (the retriever's index starts at 0, as upstream's does)
        return self.faiss_retriever.invoke(inputs, self._faiss_depth(), subset=self._dense_filter(passing, dense_rows))

    def _faiss_consume(self, ids_list, scores_list, seen, out, bundle_cnt, allow=None):
        for ids, scores in zip(ids_list, scores_list):
            ids = [int(i) for i in ids]
            score_map = dict(zip(ids, scores))
            for row, score in zip(ids[:self.faiss_k], scores[:self.faiss_k]):
                if row < 0 or row in seen:   # -1 pads a corpus smaller than the search depth
                    continue
                seen.add(row)
                md = self.chunk_metadata[row]
                rows = self._bundle_of(row, seen, allow)
                if score > EXPAND_SCORE and self.enable_expand:
                    self._expand(rows, md, score_map, seen, allow)
                self._emit(out, "FAISS", score, rows, bundle_cnt)
                bundle_cnt += 1
        return bundle_cnt

    def _faiss_branch(self, input, hyde_chunks, seen, out, bundle_cnt, passing=None, allow=None, dense_rows=None):
        ids_list, scores_list = self._faiss_ask(input, hyde_chunks, passing, dense_rows)
        return self._faiss_consume(ids_list, scores_list, seen, out, bundle_cnt, allow)

    def _title_consume(self, t_ids, t_scores, seen, out, bundle_cnt, allow=None):
        for t, score in zip(t_ids, t_scores):
            if t < 0:
                continue
            for row in self._title_rows.get(self.title_summaries[int(t)], ()):
                if row in seen or (allow is not None and row not in allow):
                    continue
                seen.add(row)
                self._emit(out, "Title Summary", score, self._bundle_of(row, seen, allow), bundle_cnt)
                bundle_cnt += 1
        return bundle_cnt

    def _title_branch(self, input, seen, out, bundle_cnt, allow=None):
        t_ids, t_scores = self.title_summary_faiss_retriever.invoke([input], self.faiss_ts_k)
        return self._title_consume(t_ids[0], t_scores[0], seen, out, bundle_cnt, allow)

    def _bm25_depth(self, passing=None) -> int:
        """Rows a retriever with a total order is asked for: bm25_k, or fewer where fewer exist (or pass)."""
        return max(1, min(int(self.bm25_k), self.num_chunk if passing is None else len(passing)))

    def _bm25_ask(self, input, allow=None, passing=None, bm25_rows=None):
        """The (row, score) pairs the branch emits from, at most bm25_k of them."""
        if allow is not None:
            # filtered: the first bm25_k passing rows of the full ranking (whole-corpus statistics: the stated exception) -- from a
            # retriever that filters on its own (filtered_prefix), else from the full ranking, filtered here
            if passing is not None and bm25_rows is not None and bm25_rows is not passing:   # a prepared filter: its mode is its own
                b_ids, b_scores = self.bm25_retriever.invoke(input, self._bm25_depth(passing), subset=bm25_rows)
                return [(int(r), s) for r, s in zip(b_ids, b_scores)]
            if passing is not None and self.where_statistics == "subset":   # no exception: the passing chunks' own statistics
                b_ids, b_scores = self.bm25_retriever.invoke(input, self._bm25_depth(passing), subset=passing, stats="subset")
                return [(int(r), s) for r, s in zip(b_ids, b_scores)]
            if passing is not None and getattr(self.bm25_retriever, "filtered_prefix", False) is True:
                b_ids, b_scores = self.bm25_retriever.invoke(input, self._bm25_depth(passing), subset=passing)
                return [(int(r), s) for r, s in zip(b_ids, b_scores)]
            b_ids, b_scores = self.bm25_retriever.invoke(input, self.num_chunk)
            return [(int(r), s) for r, s in zip(b_ids, b_scores) if int(r) in allow][:self.bm25_k]
        # upstream ranks every chunk (:188) and reads the first bm25_k; a retriever whose ranking is a total order
        # (exact_prefix, e.g. veritasfi_amd.BM25Retriever) returns exactly that prefix when asked for bm25_k rows -- min_score
        # included, since it keeps a prefix of a descending ranking.  Others keep the upstream call.
        depth = self.num_chunk
        if getattr(self.bm25_retriever, "exact_prefix", False) is True:
            depth = self._bm25_depth()
        b_ids, b_scores = self.bm25_retriever.invoke(input, depth)
        return list(zip(b_ids[:self.bm25_k], b_scores[:self.bm25_k]))

    def _bm25_consume(self, kept, seen, out, bundle_cnt, allow=None):
        for row, score in kept:
            if row in seen:
                continue
            seen.add(row)
            self._emit(out, "BM25", score, self._bundle_of(row, seen, allow), bundle_cnt)
            bundle_cnt += 1
        return bundle_cnt

    def _bm25_branch(self, input, seen, out, bundle_cnt, allow=None, passing=None, bm25_rows=None):
        return self._bm25_consume(self._bm25_ask(input, allow, passing, bm25_rows), seen, out, bundle_cnt, allow)

    # -- many requests at once ------------------------------------------------------------------------
    def invoke_batch(self, inputs, hyde_chunks_list, wheres=None) -> List[List[Dict]]:
        """``[invoke(inputs[i], hyde_chunks_list[i], where=wheres[i]) for i]``, equal as Python objects, with each leg asked ONCE for
        the whole batch where it can be: requests of different tenants share the device calls.
        wheres: None, or one of None / dict / ``PreparedWhere`` per request.  A dict is prepared for the duration of the call
        (``prepare_where``) and released after; dicts of equal content share one preparation.
        Dense leg: one ``invoke(every input and hyde chunk, depth, subsets=[the request's dense filter per string])`` when the retriever
        declares ``per_query_subsets`` (this package's ``FaissRetriever``), else one call per request, as ``invoke`` makes it.
        Title-summary leg: one ``invoke(inputs, faiss_ts_k)``.  BM25 leg: one ``invoke_batch(inputs, min(bm25_k, chunks),
        subsets=[BM25Subset or None])`` when the retriever offers ``prepare_subset``, an ``invoke_batch`` that takes ``subsets=`` and
        declares ``exact_prefix``; each request keeps its own ``min(bm25_k, passing rows)`` because that call returns
        ``min(k, rows allowed)`` rows per query.  Else one call per request.  A request whose filter passes nothing yields [] and asks
        no leg.  ``seen``, the bundle counter and the order of emission are per request, exactly as in ``invoke``.  Stage brackets: one
        ``"retrieve"`` around the batch; the ``retrieved_chunks`` metric is recorded once per request."""
        inputs = list(inputs)
        hyde = [list(h) for h in hyde_chunks_list]
        if len(hyde) != len(inputs):
            raise ValueError(f"invoke_batch: {len(hyde)} hyde chunk lists for {len(inputs)} inputs")
        wheres = [None] * len(inputs) if wheres is None else list(wheres)
        if len(wheres) != len(inputs):
            raise ValueError(f"invoke_batch: {len(wheres)} wheres for {len(inputs)} inputs")
        for w in wheres:
            if w is not None and not isinstance(w, (dict, PreparedWhere)):
                raise TypeError("invoke_batch: each entry of `wheres` is None, a dict (rows_where's argument) or a PreparedWhere")
        with stages.stage("retrieve"):
            outs = self._invoke_batch(inputs, hyde, wheres)
        for out in outs:
            stages.metric("retrieved_chunks", len(out))
        return outs

    @staticmethod
    def _where_key(where: dict):
        """Dicts of equal content share one preparation: the key of a dict's content, or of the object itself where a value cannot
        be hashed."""
        def frozen(v, deep=False):   # deep: inside an operator dict or a list, where 1 and True are different filters
            if isinstance(v, dict):
                return ("dict", frozenset((f, frozen(x, True)) for f, x in v.items()))
            if isinstance(v, (set, frozenset)):
                return (type(v).__name__, frozenset(frozen(x, deep) for x in v))
            if isinstance(v, (list, tuple)):
                return (type(v).__name__, tuple(frozen(x, deep or isinstance(x, dict)) for x in v))
            return (type(v).__name__, v) if deep else v
        try:
            key = frozenset((f, frozen(v)) for f, v in where.items())
            hash(key)
            return key
        except TypeError:
            return ("object", id(where))

    def _bm25_takes_subsets(self) -> bool:
        bm = self.bm25_retriever
        fn = getattr(bm, "invoke_batch", None)
        if fn is None or not hasattr(bm, "prepare_subset") or getattr(bm, "exact_prefix", False) is not True:
            return False
        import inspect
        try:
            params = inspect.signature(fn).parameters
        except (TypeError, ValueError):
            return False
        return "subsets" in params or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())

    def _invoke_batch(self, inputs, hyde, wheres) -> List[List[Dict]]:
        temps = {}   # the dicts of this call, prepared once per content
        try:
            state = []
            for w in wheres:
                if isinstance(w, dict):
                    key = self._where_key(w)
                    if key not in temps:
                        temps[key] = PreparedWhere(self, w)
                    w = temps[key]
                state.append(self._resolve_where(w))
            n = len(inputs)
            outs = [[] for _ in range(n)]
            seen = [set() for _ in range(n)]
            cnt = [0] * n
            live = [i for i in range(n) if state[i][0] is None or state[i][0].size > 0]   # the others yield [] and ask no leg
            if not live:
                return outs
            if self.faiss_k > 0:
                with stages.stage("retrieve_faiss"):
                    answers = self._faiss_ask_batch(live, inputs, hyde, state)
                    for i in live:
                        cnt[i] = self._faiss_consume(answers[i][0], answers[i][1], seen[i], outs[i], cnt[i], state[i][1])
            if self.faiss_ts_k > 0:
                with stages.stage("retrieve_faiss_ts"):
                    t_ids, t_scores = self.title_summary_faiss_retriever.invoke([inputs[i] for i in live], self.faiss_ts_k)
                    for j, i in enumerate(live):
                        cnt[i] = self._title_consume(t_ids[j], t_scores[j], seen[i], outs[i], cnt[i], state[i][1])
            if self.bm25_k > 0:
                with stages.stage("retrieve_bm25"):
                    kept = self._bm25_ask_batch(live, inputs, state)
                    for i in live:
                        cnt[i] = self._bm25_consume(kept[i], seen[i], outs[i], cnt[i], state[i][1])
            return outs
        finally:
            for pw in temps.values():
                pw.close()

    def _faiss_ask_batch(self, live, inputs, hyde, state) -> dict:
        """request -> (ids_list, scores_list), one entry per string of the request ([input] + hyde chunks)."""
        if getattr(self.faiss_retriever, "per_query_subsets", False) is not True:
            return {i: self._faiss_ask(inputs[i], hyde[i], state[i][0], state[i][2]) for i in live}
        strings, subsets, spans = [], [], {}
        for i in live:
            mine = [inputs[i]] + hyde[i]
            passing, _, dense_rows, _ = state[i]
            spans[i] = (len(strings), len(strings) + len(mine))
            strings += mine
            subsets += [None if passing is None else self._dense_filter(passing, dense_rows)] * len(mine)   # the same object: one list
        ids, scores = self.faiss_retriever.invoke(strings, self._faiss_depth(), subsets=subsets)
        return {i: (ids[a:b], scores[a:b]) for i, (a, b) in spans.items()}

    def _bm25_ask_batch(self, live, inputs, state) -> dict:
        """request -> the (row, score) pairs its BM25 branch emits from."""
        bm = self.bm25_retriever
        batched = self._bm25_takes_subsets()
        if batched:   # every filtered request must bring an object the retriever prepared
            batched = all(state[i][0] is None or (state[i][3] is not None and state[i][3] is not state[i][0]) for i in live)
        if not batched:
            return {i: self._bm25_ask(inputs[i], state[i][1], state[i][0], state[i][3]) for i in live}
        answers = bm.invoke_batch([inputs[i] for i in live], self._bm25_depth(), subsets=[None if state[i][0] is None else state[i][3] for i in live])
        kept = {}
        for j, i in enumerate(live):
            b_ids, b_scores = answers[j]
            if state[i][0] is None:
                kept[i] = list(zip(b_ids[:self.bm25_k], b_scores[:self.bm25_k]))
            else:   # min(bm25_k, passing rows) of them: the call returns min(k, rows allowed) per query
                want = self._bm25_depth(state[i][0])
                kept[i] = [(int(r), s) for r, s in zip(b_ids[:want], b_scores[:want])]
        return kept

    # ensembleRetriever.py:235-281
    def compute_similarity(self, chunks, selected_indices, candidate_index):
        return compute_similarity(self.embeddings, chunks, selected_indices, candidate_index)

    def compute_similarity_mtx(self, chunks):
        """The reference's signature and return (``[n, n]`` tensor indexed ``similar_mtx[idx, selected] > 0.9``,
        vllmManager.py:462,476).  Texts this retriever emitted are read from their corpus rows in HBM; the others are embedded in
        ONE batched call; with ``similarity_from_rows`` off (or nothing known) every text is embedded, as upstream."""
        chunks = list(chunks)
        rows = self._text_rows.rows_of(chunks) if self.similarity_from_rows else []
        if not chunks or not any(r >= 0 for r in rows):
            return compute_similarity_mtx(self.embeddings, chunks)
        unknown = [t for t, r in zip(chunks, rows) if r < 0]
        extra = _embed_all(self.embeddings, unknown) if unknown else None
        ix = self.faiss_retriever.index
        ids = np.asarray([r + ix.id_offset if r >= 0 else -1 for r in rows], dtype=np.int64)
        import torch
        return torch.from_numpy(ix.cosine_matrix_rows(ids, extra))
