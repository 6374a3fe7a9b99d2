"""Corpus file (.vfc) writer / reader -- the on-disk form of the embedding matrix.

Stands where the reference re-reads every embedding from Chroma into Python lists on each start
(``src/utils/ensembleRetriever.py:39-43`` -> ``src/utils/faissRetriever.py:14``): the embed loop
(``src/load_data.py:120-128``) appends its batches here once, and each rank's ``DenseIndex.from_file`` streams
only its row shard from disk into HBM (``vf_index_create_from_file``).  Layout: include/veritasfi_hip.h.
"""
from __future__ import annotations

import ctypes
import os
import struct

import numpy as np

from . import _ffi

MAGIC = b"VFCORPUS"
_HDR = struct.Struct("<8sIIQII32x")
_DT = {np.dtype(np.float32): _ffi.VF_DTYPE_F32, np.dtype(np.float16): _ffi.VF_DTYPE_F16, np.dtype(np.uint8): _ffi.VF_DTYPE_FP8_E4M3,
       np.dtype(np.int8): _ffi.VF_DTYPE_INT8}
_NP = {v: k for k, v in _DT.items()}


class CorpusWriter:
    """Append row batches, then close (writes the header last so that a partial file never validates).

    ``mode="a"`` extends a file that exists (``d`` and ``dtype`` default to the header's and must equal it when given; every batch
    carries ids exactly when the file has an id table): what a live index was given through ``DenseIndex.add`` is written here, so
    a restart that loads the file sees the same rows.  The new rows are written first, then the id table, then the header: a
    file WITHOUT an id table is valid at every instant (the header names the old row count until ``close``, and the old rows
    are never touched).  A file WITH one keeps its table behind the rows, so the new rows overwrite it: between the first ``append``
    and ``close`` the header still validates but the table it points to is gone -- ``abort`` (and leaving the ``with`` block on an
    error) puts the old table back; an append cut short by a crash does not, so keep the ids elsewhere until ``close`` returns."""

    def __init__(self, path: str, d: int = None, dtype=None, e4m3: bool = False, mode: str = "w"):
        if mode not in ("w", "a"):
            raise ValueError("mode must be 'w' or 'a'")
        self.path, self.mode = path, mode
        self._ids = []
        self._want_ids = None   # None: the first batch decides ("w"); True / False: what the file holds ("a")
        if mode == "a":
            h = read_header(path)
            held = _NP[h["dtype"]]
            want = None if (dtype is None and not e4m3) else (np.dtype(np.uint8) if e4m3 else np.dtype(dtype))
            if d is not None and int(d) != h["d"]:
                raise ValueError(f"{path} holds rows of {h['d']} elements, not {int(d)}")
            if want is not None and want != held:
                raise ValueError(f"{path} holds {held} rows, not {want}")
            self.d, self.n, self.dtype = int(h["d"]), int(h["n"]), held
            self._n0, self._want_ids = self.n, bool(h["has_ids"])
            self._size0 = _HDR.size + self.n * self.d * held.itemsize + (8 * self.n if h["has_ids"] else 0)
            if os.path.getsize(path) < self._size0:
                raise ValueError(f"{path} is truncated")
            self._old_ids = np.array(external_ids(path)) if h["has_ids"] else None
            if self._old_ids is not None:
                self._ids.append(self._old_ids)
            self._f = open(path, "r+b")
            self._f.seek(_HDR.size + self.n * self.d * held.itemsize)   # behind the last row: onto the id table, if there is one
            return
        if d is None:
            raise ValueError("d is required for a new corpus file")
        self.d, self.n = int(d), 0
        self.dtype = np.dtype(np.uint8) if e4m3 else np.dtype(np.float16 if dtype is None else dtype)
        if self.dtype not in _DT:
            raise TypeError(f"unsupported corpus dtype {self.dtype}")
        self._f = open(path, "wb")
        self._f.write(b"\0" * _HDR.size)

    def append(self, rows, ids=None) -> None:
        # (one-byte codes -- e4m3 bytes, int8 rows -- are taken as they are or refused below, never cast: a cast would wrap them)
        # (an extended file takes rows of its own type only: its older rows were written from that type, and so is a live index's copy)
        if self.mode == "a" and np.asarray(rows).dtype != self.dtype:
            raise ValueError(f"batch must be [m, {self.d}] of {self.dtype}")
        rows = np.ascontiguousarray(np.asarray(rows), dtype=self.dtype) if self.dtype.itemsize > 1 else np.ascontiguousarray(rows)
        if rows.dtype != self.dtype or rows.ndim != 2 or rows.shape[1] != self.d:
            raise ValueError(f"batch must be [m, {self.d}] of {self.dtype}")
        if self._want_ids is not None and (ids is not None) != self._want_ids:
            raise ValueError("the file has an id table: every batch must carry ids" if self._want_ids else
                             "the file has no id table: no batch may carry ids")
        if (ids is None) != (not self._ids) and self.n:
            raise ValueError("either every batch carries ids or none does")
        if ids is not None:
            ids = np.asarray(ids, dtype=np.int64)
            if ids.shape != (rows.shape[0],):
                raise ValueError("ids must be one int64 per row")
        self._f.write(rows.tobytes())
        if ids is not None:
            self._ids.append(ids)
        self.n += rows.shape[0]

    def abort(self) -> None:
        """Leave on an error.  A new file: the header is NOT written (the file keeps its zeroed first 64 bytes, which no reader
        accepts) and the partial file is removed.  An extended file: it is put back as it was -- the old id table rewritten behind
        the old rows, the new rows cut off; its header was never touched."""
        if self._f is None:
            return
        if self.mode == "a":
            self._f.seek(_HDR.size + self._n0 * self.d * self.dtype.itemsize)
            if self._old_ids is not None:
                self._f.write(self._old_ids.tobytes())
            self._f.truncate(self._size0)
            self._f.close()
            self._f = None
            return
        self._f.close()
        self._f = None
        try:
            os.remove(self.path)
        except OSError:
            pass

    def close(self) -> None:
        if self._f is None:
            return
        if self._ids:
            self._f.write(np.concatenate(self._ids).tobytes())
        self._f.flush()   # rows and id table are in the file before the header names them
        self._f.seek(0)
        self._f.write(_HDR.pack(MAGIC, 1, _DT[self.dtype], self.n, self.d, 1 if self._ids else 0))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *a):
        if exc_type is not None:
            self.abort()
        else:
            self.close()


def write(path: str, rows, ids=None, e4m3: bool = False) -> None:
    rows = np.asarray(rows)
    with CorpusWriter(path, rows.shape[1], rows.dtype, e4m3=e4m3) as w:
        w.append(rows, ids)


def append(path: str, rows, ids=None) -> int:
    """Extend the corpus file at ``path`` by ``rows`` (and their ``ids``, when the file has an id table); returns the row number of
    the first one.  See ``CorpusWriter`` (mode "a") for what an interrupted call leaves behind."""
    with CorpusWriter(path, mode="a") as w:
        first = w.n
        w.append(rows, ids)
    return first


def remove(path: str, ids, block_rows: int = 65536) -> int:
    """Remove the rows ``ids`` (file row numbers; duplicates count once) from the corpus file at ``path``, later rows moving down as
    they do in a live index (``DenseIndex.remove``): a restart that loads the file sees what the index saw.  Returns the number
    removed.  The compacted file -- with its id table, if it has one -- is written beside the old one, synced, and takes its place in one
    ``os.replace``: a crash leaves the old file intact or the new one complete, never a mixture.  The directory is synced afterwards
    where the platform allows it, so that the replacement itself survives a power loss; where it does not (the sync is refused), the
    old file may come back after one.  A row number outside the file raises ValueError and changes nothing."""
    ids = np.asarray(ids, dtype=np.int64).ravel()
    h = read_header(path)
    n, d, dt = int(h["n"]), int(h["d"]), _NP[h["dtype"]]
    bad = np.flatnonzero((ids < 0) | (ids >= n))
    if bad.size:
        raise ValueError(f"remove: ids[{int(bad[0])}] = {int(ids[bad[0]])} is outside the file's rows [0, {n})")
    gone = np.unique(ids)
    if gone.size == 0:
        return 0
    if os.path.getsize(path) < _HDR.size + n * d * dt.itemsize + (8 * n if h["has_ids"] else 0):
        raise ValueError(f"{path} is truncated")
    keep = np.ones(n, dtype=bool)
    keep[gone] = False
    rows = rows_memmap(path)
    old_ids = external_ids(path)
    tmp = f"{path}.remove-{os.getpid()}.tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(_HDR.pack(MAGIC, 1, h["dtype"], n - int(gone.size), d, 1 if h["has_ids"] else 0))
            for r0 in range(0, n, block_rows):
                f.write(np.ascontiguousarray(rows[r0:r0 + block_rows][keep[r0:r0 + block_rows]]).tobytes())
            if old_ids is not None:
                f.write(np.ascontiguousarray(np.asarray(old_ids)[keep]).tobytes())
            f.flush()
            os.fsync(f.fileno())
        del rows, old_ids
        os.replace(tmp, path)
        try:                                                           # the rename is durable once its directory is
            dfd = os.open(os.path.dirname(os.path.abspath(path)), os.O_RDONLY)
            try:
                os.fsync(dfd)
            finally:
                os.close(dfd)
        except OSError:
            pass
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise
    return int(gone.size)


def info(path: str) -> dict:
    """Header fields through the library's own validator (vf_corpus_file_info)."""
    n, d, dt, has = _ffi.c_i64(0), _ffi.c_i32(0), _ffi.c_i32(0), _ffi.c_i32(0)
    _ffi.check(_ffi.lib().vf_corpus_file_info(path.encode(), ctypes.byref(n), ctypes.byref(d), ctypes.byref(dt),
                                              ctypes.byref(has)), "vf_corpus_file_info")
    return {"n": n.value, "d": d.value, "dtype": dt.value, "has_ids": bool(has.value)}


def read_header(path: str) -> dict:
    """Pure-Python header read (no GPU library needed): for tools and CPU tests."""
    with open(path, "rb") as f:
        raw = f.read(_HDR.size)
    if len(raw) != _HDR.size:
        raise ValueError("corpus file too short")
    magic, version, dt, n, d, flags = _HDR.unpack(raw)
    if magic != MAGIC or version != 1 or dt not in _NP or d == 0:
        raise ValueError("not a version-1 corpus file")
    return {"n": n, "d": d, "dtype": dt, "has_ids": bool(flags & 1)}


def rows_memmap(path: str):
    h = read_header(path)
    return np.memmap(path, mode="r", dtype=_NP[h["dtype"]], offset=_HDR.size, shape=(h["n"], h["d"]))


def external_ids(path: str):
    """int64[n] external ids (row -> caller's id), or None when the file carries none."""
    h = read_header(path)
    if not h["has_ids"]:
        return None
    off = _HDR.size + h["n"] * h["d"] * _NP[h["dtype"]].itemsize
    return np.memmap(path, mode="r", dtype=np.int64, offset=off, shape=(h["n"],))


def embed_to_file(path: str, texts, embedder, batch_size: int = 100, dtype=np.float16, ids=None, on_batch=None) -> int:
    """The embed loop of ``import_collection_from_dir`` (``src/load_data.py:120-128,151``: batches of 100 texts through
    ``embed_documents``) writing a corpus file instead of one Chroma insert per batch.  ``embedder`` is anything with
    ``embed_documents(list[str]) -> list[list[float]]`` (``HipEmbeddings``, or the reference's ``HuggingFaceEmbeddings``).
    Returns the number of rows written."""
    texts = list(texts)
    if ids is not None and len(ids) != len(texts):
        raise ValueError("one id per text")
    w = None
    try:
        for i in range(0, len(texts), batch_size):
            vecs = np.asarray(embedder.embed_documents(texts[i:i + batch_size]), dtype=np.float32)
            if w is None:
                w = CorpusWriter(path, vecs.shape[1], dtype)
            w.append(vecs.astype(dtype), None if ids is None else np.asarray(ids[i:i + batch_size], dtype=np.int64))
            if on_batch is not None:
                on_batch(i + vecs.shape[0], len(texts))
        if w is None:
            raise ValueError("no texts to embed")
        n = w.n
    except BaseException:
        if w is not None:
            w.abort()  # a failed embed loop must not leave a truncated file that validates
        raise
    w.close()
    return n
