"""DenseIndex -- Python handle over ``vf_index_*`` (exact cosine top-k on one MI355X).

Stands where ``faiss.IndexFlatIP`` + ``faiss.normalize_L2`` stand in the reference
(``src/utils/faissRetriever.py:18-24,35-37``).  NumPy in / NumPy out for the drop-in classes; torch
CUDA tensors in / out (zero copy, device pointers through the C ABI) for the serving and multi-GPU
paths.  PyTorch is plumbing here: device memory and streams only.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np

from . import _ffi


def _is_torch_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def quantize_int8(x) -> np.ndarray:
    """[n, d] floats -> int8 codes, one scale per row (not kept: a cosine does not see a positive per-row scale, so an int8 index
    stores the codes alone).  The recipe is the device's own (k_prep_image), in fp32: ``sc = absmax / 127`` (zero rows: 1),
    ``code = clip(rint(x / sc), -127, 127)`` with ties to even.  Non-finite input raises ValueError."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("quantize_int8: x must be [n, d]")
    x = np.ascontiguousarray(x, dtype=np.float32)
    if not np.isfinite(x).all():
        raise ValueError("quantize_int8: the rows hold non-finite values")
    mx = np.abs(x).max(axis=1, keepdims=True) if x.shape[1] else np.zeros((x.shape[0], 1), np.float32)
    sc = np.where(mx > 0, mx / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    return np.clip(np.rint(x / sc), -127.0, 127.0).astype(np.int8)


def subset_ids(subset, n: int, id_offset: int = 0) -> np.ndarray:
    """What ``DenseIndex.search(subset=...)`` hands to the library: a contiguous int64 array of global ids, strictly ascending.
    ``subset`` is an int64 array-like of ids (any order, repeats count once) or a boolean mask of length ``n`` (True = row
    ``id_offset + i`` is searched).  The ascending check runs first and costs one pass; only a list that fails it is sorted and made
    distinct.  Ids outside ``[id_offset, id_offset + n)`` raise ValueError naming the first offender's position in the caller's list."""
    a = np.asarray(subset)
    if a.dtype == np.bool_:
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"subset: a boolean mask must have one entry per row ({n}), got shape {a.shape}")
        return np.flatnonzero(a).astype(np.int64) + np.int64(id_offset)
    if a.size == 0:
        return np.empty(0, dtype=np.int64)
    if a.dtype.kind not in "iu":
        raise TypeError(f"subset: ids must be integers or a boolean mask, got {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"subset: ids must be one-dimensional, got shape {a.shape}")
    if a.dtype == np.uint64 and a.max() > np.uint64(np.iinfo(np.int64).max):
        raise ValueError("subset: an id does not fit int64")
    ids = np.ascontiguousarray(a, dtype=np.int64)
    lo, hi = int(id_offset), int(id_offset) + int(n)
    bad = np.flatnonzero((ids < lo) | (ids >= hi))
    if bad.size:
        raise ValueError(f"subset: ids[{int(bad[0])}] = {int(ids[bad[0]])} is outside the index's ids [{lo}, {hi})")
    if ids.size > 1 and not bool((ids[1:] > ids[:-1]).all()):
        ids = np.unique(ids)   # sorted, distinct
    return ids


class RowSubset:
    """A list of row ids kept ON THE DEVICE for repeated subset searches (``DenseIndex.row_subset``): a tenant's filter is uploaded
    once, not 8 bytes per row per query.  It holds ids, not rows: after ``DenseIndex.remove`` (ids shift) make a new one -- the
    library's range check catches a stale one only when it reaches past the new end of the index."""

    def __init__(self, ids: np.ndarray, device_id: int):
        import torch
        self.ids = ids                       # host copy (int64, strictly ascending)
        self.device_id = int(device_id)
        self.tensor = torch.from_numpy(ids).to(f"cuda:{self.device_id}")

    @classmethod
    def adopt(cls, tensor, ids: np.ndarray, device_id: int) -> "RowSubset":
        """A RowSubset around ids that are ALREADY on the device (``DenseIndex.eval_where`` leaves them there): ``tensor`` (int64, CUDA,
        strictly ascending global ids) and its host copy ``ids``; nothing is uploaded."""
        rs = cls.__new__(cls)
        rs.ids, rs.device_id, rs.tensor = ids, int(device_id), tensor
        return rs

    def __len__(self) -> int:
        return int(self.ids.size)


SUBSETS_MAX_IDS = 16384   # the longest list the library's list-per-query mode serves (kSubsetRankRows, vf_subset_multi.h)


def subsets_plan(subsets, nq: int, n: int, id_offset: int = 0, device_id=None, subset=None) -> dict:
    """How ``DenseIndex.search(queries, k, subsets=[...])`` is served -- a pure function of its arguments (no GPU, no library).
    ``subsets`` holds one entry per query: ids, a boolean mask, a ``RowSubset`` or None.  Entries that are the SAME OBJECT share one
    list; equal contents in different objects do not (nothing is compared).  The answer:
    ``plain``: the queries whose entry is None -- one unfiltered call for all of them;
    ``long``: ``[{"subset", "queries"}]``, one per distinct object of more than ``SUBSETS_MAX_IDS`` ids -- one ``subset=`` call each;
    ``multi``: None, or ``{"form", "queries", "lists", "list_of", "first_query"}`` -- ONE list-per-query call for all the rest:
    ``lists[list_of[i]]`` serves ``queries[i]``, ``first_query[j]`` is the first query of the call's ``subsets`` that uses ``lists[j]``.
    ``form`` is "device" when every list is a ``RowSubset`` on ``device_id`` (``lists`` then holds those objects), else "host"
    (``lists`` holds int64 arrays; a ``RowSubset`` gives its host copy)."""
    if subset is not None:
        raise ValueError("search: subset= (one list for the whole call) and subsets= (one per query) cannot be given together")
    entries = list(subsets)
    if len(entries) != int(nq):
        raise ValueError(f"subsets: {len(entries)} entries for {int(nq)} queries (one entry per query; None = no filter)")
    plain, slot_of, groups = [], {}, []
    for q, e in enumerate(entries):
        if e is None:
            plain.append(q)
            continue
        g = slot_of.get(id(e))
        if g is None:
            is_rs = isinstance(e, RowSubset)
            ids = e.ids if is_rs else subset_ids(e, n, id_offset)
            g = slot_of[id(e)] = len(groups)
            groups.append({"object": e, "ids": ids, "row_subset": is_rs, "queries": []})
        groups[g]["queries"].append(q)
    long = [{"subset": g["object"] if g["row_subset"] else g["ids"], "queries": g["queries"]} for g in groups if g["ids"].size > SUBSETS_MAX_IDS]
    short = [g for g in groups if g["ids"].size <= SUBSETS_MAX_IDS]
    multi = None
    if short:
        on_device = device_id is not None and all(g["row_subset"] and g["object"].device_id == int(device_id) for g in short)
        pairs = sorted((q, j) for j, g in enumerate(short) for q in g["queries"])
        multi = {"form": "device" if on_device else "host", "queries": [q for q, _ in pairs], "list_of": [j for _, j in pairs],
                 "lists": [g["object"] if on_device else g["ids"] for g in short], "first_query": [g["queries"][0] for g in short]}
    return {"plain": plain, "long": long, "multi": multi}


def _name_subsets(message: str, first_query) -> str:
    """The library names ``lists[j]``; the caller knows ``subsets[i]``: the first query that uses that list."""
    import re
    return re.sub(r"lists\[(\d+)\]", lambda mo: f"subsets[{first_query[int(mo.group(1))]}]" if int(mo.group(1)) < len(first_query) else mo.group(0), message)


def _dev_array(device_ids):
    ids = [int(x) for x in device_ids]
    if not ids:
        raise ValueError("device_ids must name at least one device")
    return (_ffi.c_i32 * len(ids))(*ids), ids


class DenseIndex:
    _where_ids = None   # eval_where's n-sized id scratch (one per index, made on first use)

    def __init__(self, rows, device_id: int = 0, id_offset: int = 0, device_ids=None):
        """rows: [n, d] float32 / float16 ndarray (copied to HBM) or a CUDA torch tensor (borrowed).
        FP8: a torch.float8_e4m3fn tensor (CPU or CUDA), or a uint8 ndarray / tensor of OCP e4m3 codes passed with
        ``DenseIndex.from_e4m3``; the bytes stay fp8 in HBM (scanned as fp8, converted exactly in registers).
        INT8: an int8 ndarray or torch.int8 tensor (CPU or CUDA; ``quantize_int8`` makes one from floats) -- one byte per element in
        HBM, scored as the canonical cosine of the integers; always copied (a CUDA tensor is not borrowed and may be freed at once).
        device_ids=[...]: ONE handle over several GPUs in this process (``vf_index_create_sharded``): host rows are
        split into contiguous blocks, one per listed device; every search method works on it unchanged, device
        buffers live on the home device ``device_ids[0]``."""
        L = _ffi.lib()
        self._h = _ffi.vp()
        self._keepalive = None
        self.device_id = int(device_id)
        self.device_ids = None
        e4m3 = getattr(self, "_e4m3", False)
        if device_ids is not None:
            if _is_torch_tensor(rows):
                import torch
                if rows.dtype == getattr(torch, "float8_e4m3fn", None):
                    rows, e4m3 = rows.view(torch.uint8), True
                rows = rows.cpu().numpy()   # the sharded constructor distributes HOST rows (DenseIndex.group adopts device shards)
            rows = np.asarray(rows)
            if rows.ndim != 2:
                raise ValueError("rows must be [n, d]")
            if e4m3:
                if rows.dtype != np.uint8:
                    raise TypeError("e4m3 rows must be uint8 codes")
                dt = _ffi.VF_DTYPE_FP8_E4M3
            elif rows.dtype == np.int8:
                dt = _ffi.VF_DTYPE_INT8
            elif rows.dtype == np.float16:
                dt = _ffi.VF_DTYPE_F16
            else:
                rows, dt = rows.astype(np.float32, copy=False), _ffi.VF_DTYPE_F32
            rows = np.ascontiguousarray(rows)
            arr, ids = _dev_array(device_ids)
            self.n, self.d, self.id_offset = int(rows.shape[0]), int(rows.shape[1]), 0
            self.device_id, self.device_ids = ids[0], ids
            _ffi.check(L.vf_index_create_sharded(ctypes.byref(self._h), rows.ctypes.data, self.n, self.d, dt, arr, len(ids)),
                       "vf_index_create_sharded")
            self._warn_if_staged()
            return
        if _is_torch_tensor(rows):
            import torch
            if rows.dtype == getattr(torch, "float8_e4m3fn", None):
                rows, e4m3 = rows.view(torch.uint8), True
            if not rows.is_cuda:
                rows = rows.cpu().numpy()
            else:
                if rows.dim() != 2 or not rows.is_contiguous():
                    raise ValueError("rows must be a contiguous [n, d] tensor")
                if e4m3 and rows.dtype == torch.uint8:
                    dt = _ffi.VF_DTYPE_FP8_E4M3
                elif rows.dtype == torch.int8 and not e4m3:
                    dt = _ffi.VF_DTYPE_INT8
                elif rows.dtype == torch.float16:
                    dt = _ffi.VF_DTYPE_F16
                elif rows.dtype == torch.float32:
                    dt = _ffi.VF_DTYPE_F32
                else:
                    raise TypeError(f"unsupported corpus dtype {rows.dtype}")
                self.device_id = rows.device.index if rows.device.index is not None else self.device_id
                self._keepalive = None if dt == _ffi.VF_DTYPE_INT8 else rows   # (int8 rows are copied: re-biased on the way)
                self.n, self.d = int(rows.shape[0]), int(rows.shape[1])
                _ffi.check(L.vf_index_create_device(ctypes.byref(self._h), rows.data_ptr(), self.n, self.d, dt,
                                                    self.device_id, int(id_offset)), "vf_index_create_device")
                self.id_offset = int(id_offset)
                return
        rows = np.asarray(rows)
        if rows.ndim != 2:
            raise ValueError("rows must be [n, d]")
        if e4m3:
            if rows.dtype != np.uint8:
                raise TypeError("e4m3 rows must be uint8 codes")
            dt = _ffi.VF_DTYPE_FP8_E4M3
        elif rows.dtype == np.int8:
            dt = _ffi.VF_DTYPE_INT8
        elif rows.dtype == np.float16:
            dt = _ffi.VF_DTYPE_F16
        else:
            rows = rows.astype(np.float32, copy=False)  # faissRetriever.py:21  x = embeddings.astype('float32')
            dt = _ffi.VF_DTYPE_F32
        rows = np.ascontiguousarray(rows)
        self.n, self.d = int(rows.shape[0]), int(rows.shape[1])
        self.id_offset = int(id_offset)
        _ffi.check(L.vf_index_create(ctypes.byref(self._h), rows.ctypes.data, self.n, self.d, dt, self.device_id,
                                     self.id_offset), "vf_index_create")

    @classmethod
    def from_file(cls, path: str, rank: int = 0, world: int = 1, device_id: int = 0, device_ids=None):
        """Rows of this rank's shard of a corpus file (veritasfi_amd/corpus_file.py), streamed disk -> HBM by the
        library; returned ids are file row numbers (id_offset = the shard's first row).  device_ids=[...]: the whole
        file, one block per listed device, behind one handle (single-process multi-GPU)."""
        from .sharded import shard_bounds
        n, d, dt, has = _ffi.c_i64(0), _ffi.c_i32(0), _ffi.c_i32(0), _ffi.c_i32(0)
        L = _ffi.lib()
        _ffi.check(L.vf_corpus_file_info(path.encode(), ctypes.byref(n), ctypes.byref(d), ctypes.byref(dt),
                                         ctypes.byref(has)), "vf_corpus_file_info")
        self = cls.__new__(cls)
        self._h = _ffi.vp()
        self._keepalive = None
        self.device_ids = None
        if device_ids is not None:
            arr, ids = _dev_array(device_ids)
            self.device_id, self.device_ids, self.id_offset = ids[0], ids, 0
            self.n, self.d = int(n.value), int(d.value)
            _ffi.check(L.vf_index_create_sharded_from_file(ctypes.byref(self._h), path.encode(), arr, len(ids)),
                       "vf_index_create_sharded_from_file")
            self._warn_if_staged()
            return self
        lo, hi = shard_bounds(n.value, world, rank)
        self.device_id, self.id_offset = int(device_id), int(lo)
        self.n, self.d = int(hi - lo), int(d.value)
        _ffi.check(L.vf_index_create_from_file(ctypes.byref(self._h), path.encode(), lo, hi, self.device_id, lo),
                   "vf_index_create_from_file")
        return self

    @classmethod
    def group(cls, shards):
        """Adopt per-device indexes (contiguous row blocks in ascending order, each built with id_offset = its first
        row) as ONE handle (``vf_index_group``).  The group owns them: the given objects are emptied."""
        shards = list(shards)
        L = _ffi.lib()
        arr = (_ffi.vp * len(shards))(*[s._h for s in shards])
        self = cls.__new__(cls)
        self._h = _ffi.vp()
        _ffi.check(L.vf_index_group(ctypes.byref(self._h), arr, len(shards)), "vf_index_group")
        self._keepalive = [s._keepalive for s in shards]   # borrowed device rows stay alive with the group
        self.device_ids = [s.device_id for s in shards]
        self.device_id, self.id_offset = shards[0].device_id, shards[0].id_offset
        self.n, self.d = sum(s.n for s in shards), shards[0].d
        for s in shards:
            s._h = _ffi.vp()
            s._keepalive = None
        self._warn_if_staged()
        return self

    @classmethod
    def from_e4m3(cls, codes, device_id: int = 0, id_offset: int = 0, device_ids=None):
        """codes: [n, d] uint8 OCP-e4m3 bytes (ndarray, CPU or CUDA tensor)."""
        self = cls.__new__(cls)
        self._e4m3 = True
        self.__init__(codes, device_id=device_id, id_offset=id_offset, device_ids=device_ids)
        return self

    @classmethod
    def from_int8(cls, codes, device_id: int = 0, id_offset: int = 0, device_ids=None):
        """codes: [n, d] int8 (ndarray, CPU or CUDA tensor) -- what ``DenseIndex(codes)`` does for int8 input, but anything else is
        refused instead of being read as floats (uint8 bytes are e4m3 codes: ``from_e4m3``)."""
        dt = str(getattr(codes, "dtype", None))
        if dt not in ("int8", "torch.int8"):
            raise TypeError(f"int8 rows must be int8, got {dt} (uint8 codes are e4m3: DenseIndex.from_e4m3)")
        return cls(codes, device_id=device_id, id_offset=id_offset, device_ids=device_ids)

    # -- appending -----------------------------------------------------------------------------------
    def _held_dtype(self) -> int:
        """VF_DTYPE_* of the rows as the index holds them (``vf_index_info``)."""
        dt = _ffi.c_i32(0)
        _ffi.check(_ffi.lib().vf_index_info(self._h, None, None, ctypes.byref(dt), None), "vf_index_info")
        return int(dt.value)

    def add(self, rows) -> int:
        """Append rows to the live index (``faiss.IndexFlatIP.add``, faissRetriever.py:24, on an index that exists) and return the id
        of the first one; the rest follow it (``id_offset + n`` before the call, upward), and ``self.n`` grows by their count.
        Inputs are the constructor's: an ndarray or CPU tensor (copied), or a CUDA tensor on the index's device (read in place, free
        afterwards); e4m3 rows as uint8 codes or ``float8_e4m3fn``; int8 rows as int8.  The rows must be of the type the index holds --
        the one the constructor would have picked for them -- or TypeError is raised: nothing is cast across widths.  An index that
        borrowed a CUDA tensor at construction takes its own copy on the first call and lets the tensor go.  Only the new rows are
        prepared (``reserve`` keeps the arrays from growing); a group handle puts them into its last shard."""
        L = _ffi.lib()
        held = self._held_dtype()
        names = {_ffi.VF_DTYPE_F32: "float32", _ffi.VF_DTYPE_F16: "float16", _ffi.VF_DTYPE_FP8_E4M3: "e4m3 codes (uint8)", _ffi.VF_DTYPE_INT8: "int8"}

        def refuse(got):
            raise TypeError(f"add: the index holds {names[held]} rows, got {got}")

        first = self.id_offset + self.n
        if _is_torch_tensor(rows):
            import torch
            if rows.dtype == getattr(torch, "float8_e4m3fn", None):
                if held != _ffi.VF_DTYPE_FP8_E4M3:
                    refuse(rows.dtype)
                rows = rows.view(torch.uint8)
            if rows.is_cuda:
                if rows.dim() != 2 or not rows.is_contiguous():
                    raise ValueError("rows must be a contiguous [m, d] tensor")
                dt = {torch.uint8: _ffi.VF_DTYPE_FP8_E4M3, torch.int8: _ffi.VF_DTYPE_INT8, torch.float16: _ffi.VF_DTYPE_F16,
                      torch.float32: _ffi.VF_DTYPE_F32}.get(rows.dtype)
                if dt != held:
                    refuse(rows.dtype)
                if int(rows.shape[1]) != self.d:
                    raise ValueError(f"rows must be [m, {self.d}], got {tuple(rows.shape)}")
                m = int(rows.shape[0])
                dev = rows.device.index if rows.device.index is not None else self.device_id
                _ffi.check(L.vf_index_create_device(ctypes.byref(self._h), rows.data_ptr(), m, self.d, dt | _ffi.VF_INDEX_APPEND, dev, 0),
                           "vf_index_create_device (append)")
                return self._added(first, m)
            rows = rows.numpy()
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != self.d:
            raise ValueError(f"rows must be [m, {self.d}], got {rows.shape}")
        if rows.dtype == np.uint8 and held == _ffi.VF_DTYPE_FP8_E4M3:
            dt = held
        elif rows.dtype == np.int8:
            dt = _ffi.VF_DTYPE_INT8
        elif rows.dtype == np.float16:
            dt = _ffi.VF_DTYPE_F16
        else:
            dt = _ffi.VF_DTYPE_F32
        if dt != held:
            refuse(rows.dtype)
        if dt == _ffi.VF_DTYPE_F32:
            rows = rows.astype(np.float32, copy=False)
        rows = np.ascontiguousarray(rows)
        m = int(rows.shape[0])
        _ffi.check(L.vf_index_create(ctypes.byref(self._h), rows.ctypes.data, m, self.d, dt | _ffi.VF_INDEX_APPEND, self.device_id, 0),
                   "vf_index_create (append)")
        return self._added(first, m)

    def _added(self, first: int, m: int) -> int:
        self.n += m
        if m and self.device_ids is None:
            self._keepalive = None   # the index holds its own copy of the rows now
        return first

    def remove(self, ids) -> int:
        """Remove rows from the live index by id (``faiss.IndexFlat.remove_ids``) and return how many left (distinct ids; duplicates in
        ``ids`` count once).  Every later row moves down, so ids stay the positions ``id_offset .. id_offset + n - 1``: a host list
        indexed by id stays aligned after ``del lst[i]`` for the same rows (highest first).  An id outside the index raises ValueError
        and removes nothing; a pending search raises RuntimeError.  Afterwards the index is what a fresh one over the remaining rows
        would be.  Capacity does not shrink: a later ``add`` uses the room.  An index that borrowed a CUDA tensor takes its own copy
        first and lets the tensor go (it is never written).  A group removes in every shard that holds one of the ids and refuses
        (RuntimeError, rc=-4) a removal that would empty a shard.  ``remove`` then ``add`` replaces a row (the new one gets a new id)."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).ravel())
        if ids.size == 0:
            return 0
        lo, hi = self.id_offset, self.id_offset + self.n
        bad = np.flatnonzero((ids < lo) | (ids >= hi))
        if bad.size:
            raise ValueError(f"remove: ids[{int(bad[0])}] = {int(ids[bad[0]])} is outside the index's ids [{lo}, {hi})")
        m = int(np.unique(ids).size)
        _ffi.check(_ffi.lib().vf_index_create(ctypes.byref(self._h), ids.ctypes.data, int(ids.size), self.d, _ffi.VF_INDEX_REMOVE,
                                              self.device_id, 0), "vf_index_create (remove)")
        self.n -= m
        if self.device_ids is None:
            self._keepalive = None   # the index holds its own copy of the rows now
        return m

    def reserve(self, total: int) -> None:
        """Room for ``total`` rows now (option ``reserve_rows``), so that ``add`` up to that count moves nothing."""
        self.set_option("reserve_rows", int(total))
        if int(total) > self.n and self.device_ids is None:
            self._keepalive = None

    # -- host buffers ------------------------------------------------------------------------------
    def search(self, queries, k: int, subset=None, subsets=None):
        """queries [nq, d] -> (ids int64 [nq, k], scores float32 [nq, k]); ids first, as
        FaissRetriever.invoke returns them (faissRetriever.py:38).
        subsets: one entry PER QUERY -- ids, a boolean mask, a ``RowSubset`` or None.  Row i is, ids and score bits, what
        ``search(queries[i:i+1], k, subset=subsets[i])`` returns (None: the plain search), in one library call for every list of at
        most 16 384 ids (``subsets_plan`` says how the rest is routed).  Entries that are the same object share a list; equal contents
        in different objects do not.  Single-device handles only.
        subset: search these rows only -- an int64 array-like of ids, a boolean mask of length n, or a ``RowSubset``.  The result is
        what an index over those rows alone would return, ids mapped back (``vf_index_search`` with ``VF_SEARCH_SUBSET``: only the listed rows are
        read).  An unsorted or repeating list is sorted and made distinct on the host first (``subset_ids``); fewer than k rows pad
        with -1 / -FLT_MAX; an empty subset returns all padding."""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"queries must be [nq, {self.d}], got {q.shape}")
        k = int(k)
        if subsets is not None:
            return self._search_subsets(q, k, subsets, subset)
        ids = np.empty((q.shape[0], k), dtype=np.int64)
        scores = np.empty((q.shape[0], k), dtype=np.float32)
        if isinstance(subset, RowSubset):
            return self._search_row_subset(q, k, subset)
        if subset is not None:
            sel = subset_ids(subset, self.n, self.id_offset)
            _ffi.check(_ffi.search_subset(_ffi.lib(), self._h, q.ctypes.data, q.shape[0], k, sel.ctypes.data, int(sel.size),
                                          ids.ctypes.data, scores.ctypes.data), "vf_index_search (subset)")
            return ids, scores
        _ffi.check(_ffi.lib().vf_index_search(self._h, q.ctypes.data, q.shape[0], k, ids.ctypes.data,
                                              scores.ctypes.data), "vf_index_search")
        return ids, scores

    def row_subset(self, ids_or_mask) -> RowSubset:
        """The ids of ``ids_or_mask`` (as ``search(subset=...)`` takes them), sorted, made distinct and kept on the index's device for
        ``search(..., subset=row_subset)``: the device entry point reads them where they are.  Single-device handles (a group
        takes lists: its shards split them on the host)."""
        if self.device_ids is not None:
            raise ValueError("row_subset: a sharded handle takes id lists (search(subset=ids)), not a device-resident subset")
        return RowSubset(subset_ids(ids_or_mask, self.n, self.id_offset), self.device_id)

    def eval_where(self, program, columns, tile_rows: int = 0):
        """A compiled metadata filter (``where.compile_where``) evaluated on the index's device: ``(RowSubset, RowMask)`` of the passing
        rows.  ``columns``: field -> ``where.WhereColumn``, made for this index's rows as they are NOW (after ``add`` / ``remove`` build
        them again: stale ones are refused).  Each column's keys and validity words go to the device on first use and stay on the
        column; the id list is written into ONE n-sized int64 scratch tensor this index keeps (calls take turns on it) and its first
        m entries are copied out for the ``RowSubset``, which therefore costs no upload.  One library call (``vf_index_search_device``
        with ``VF_SEARCH_WHERE``).  Single-device handles; a program over the device's limits (``program.fits_device``) raises ValueError:
        both are served by ``program.evaluate_numpy(columns)``."""
        import torch
        from . import where as vf_where
        if self.device_ids is not None:
            raise ValueError("eval_where: a sharded handle evaluates no filter on the device; use the numpy route (WhereProgram.evaluate_numpy)")
        if not program.fits_device:
            raise ValueError("eval_where: the program exceeds the device evaluator's limits; use the numpy route (WhereProgram.evaluate_numpy)")
        dev = torch.device(f"cuda:{self.device_id}")
        ptrs = []
        for f in program.fields:
            col = columns[f]
            held = col._device.get(self.device_id)
            if held is None:
                keys = torch.from_numpy(col.keys).to(dev)
                valid = None if col.valid is None else torch.from_numpy(col.valid_words().view(np.int32)).to(dev)
                held = col._device[self.device_id] = (keys, valid)
            ptrs.append((held[0].data_ptr(), None if held[1] is None else held[1].data_ptr()))
        n = int(program.n)
        words = torch.empty(2 * ((n + 63) // 64), dtype=torch.int32, device=dev)
        with self.__dict__.setdefault("_where_lock", threading.Lock()):   # (atomic: every constructor is served without naming it)
            if self._where_ids is None or int(self._where_ids.shape[0]) < max(n, 1):
                self._where_ids = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
            scratch = self._where_ids
            rc, m = _ffi.eval_where_device(_ffi.lib(), self._h, n, ptrs, program.leaves, program.ops, program.set_values, words.data_ptr(),
                                           scratch.data_ptr(), int(scratch.shape[0]), torch.cuda.current_stream(dev).cuda_stream, tile_rows)
            _ffi.check(rc, "vf_index_search_device (where)")
            ids = scratch[:m].clone()
        mask = vf_where.RowMask.from_words(words.cpu().numpy().view(np.uint32), n, m)
        return RowSubset.adopt(ids, ids.cpu().numpy(), self.device_id), mask

    def _search_subsets(self, q: np.ndarray, k: int, subsets, subset=None):
        if self.device_ids is not None:
            raise ValueError("search: a sharded handle takes one id list per call (search(subset=ids)), not subsets=")
        nq = q.shape[0]
        plan = subsets_plan(subsets, nq, self.n, self.id_offset, self.device_id, subset)
        ids = np.empty((nq, k), dtype=np.int64)
        scores = np.empty((nq, k), dtype=np.float32)
        if plan["plain"]:
            ids[plan["plain"]], scores[plan["plain"]] = self.search(q[plan["plain"]], k)
        for part in plan["long"]:
            ids[part["queries"]], scores[part["queries"]] = self.search(q[part["queries"]], k, subset=part["subset"])
        multi = plan["multi"]
        if multi is not None:
            qm = np.ascontiguousarray(q[multi["queries"]])
            lens = [len(x) for x in multi["lists"]]
            try:
                if multi["form"] == "device":
                    got = self._search_subsets_device(qm, k, multi["lists"], lens, multi["list_of"])
                else:
                    got = np.empty((qm.shape[0], k), dtype=np.int64), np.empty((qm.shape[0], k), dtype=np.float32)
                    _ffi.check(_ffi.search_subsets(_ffi.lib(), self._h, qm.ctypes.data, qm.shape[0], k, [x.ctypes.data for x in multi["lists"]], lens,
                                                   multi["list_of"], got[0].ctypes.data, got[1].ctypes.data), "vf_index_search (subsets)")
            except RuntimeError as e:
                raise RuntimeError(_name_subsets(str(e), multi["first_query"])) from None
            ids[multi["queries"]], scores[multi["queries"]] = got
        return ids, scores

    def _search_subsets_device(self, qm: np.ndarray, k: int, row_subsets, lens, list_of):
        import torch
        dev = torch.device(f"cuda:{self.device_id}")
        dq = torch.from_numpy(qm).to(dev)
        out_ids = torch.empty((qm.shape[0], k), dtype=torch.int64, device=dev)
        out_scores = torch.empty((qm.shape[0], k), dtype=torch.float32, device=dev)
        _ffi.check(_ffi.search_subsets_device(_ffi.lib(), self._h, dq.data_ptr(), qm.shape[0], k, [rs.tensor.data_ptr() for rs in row_subsets], lens,
                                              list_of, out_ids.data_ptr(), out_scores.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream), "vf_index_search_device (subsets)")
        return out_ids.cpu().numpy(), out_scores.cpu().numpy()

    def _search_row_subset(self, q: np.ndarray, k: int, rs: RowSubset):
        import torch
        if self.device_ids is not None or rs.device_id != self.device_id:
            raise ValueError("search: the RowSubset lives on another device than the index (or the handle is sharded)")
        dev = torch.device(f"cuda:{self.device_id}")
        dq = torch.from_numpy(q).to(dev)
        out_ids = torch.empty((q.shape[0], k), dtype=torch.int64, device=dev)
        out_scores = torch.empty((q.shape[0], k), dtype=torch.float32, device=dev)
        _ffi.check(_ffi.search_subset_device(_ffi.lib(), self._h, dq.data_ptr(), q.shape[0], k, rs.tensor.data_ptr(), len(rs),
                                             out_ids.data_ptr(), out_scores.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream), "vf_index_search_device (subset)")
        return out_ids.cpu().numpy(), out_scores.cpu().numpy()

    # -- device buffers (torch CUDA tensors) ---------------------------------------------------------
    def _dev_args(self, queries, k, out_ids, out_scores):
        import torch
        if not (queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()):
            raise ValueError("queries must be a contiguous float32 CUDA tensor")
        nq = int(queries.shape[0])
        if out_ids is None:
            out_ids = torch.empty((nq, k), dtype=torch.int64, device=queries.device)
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
        stream = torch.cuda.current_stream(queries.device).cuda_stream
        return nq, out_ids, out_scores, stream

    def search_device(self, queries, k: int, out_ids=None, out_scores=None):
        nq, out_ids, out_scores, stream = self._dev_args(queries, int(k), out_ids, out_scores)
        _ffi.check(_ffi.lib().vf_index_search_device(self._h, queries.data_ptr(), nq, int(k), out_ids.data_ptr(),
                                                     out_scores.data_ptr(), stream), "vf_index_search_device")
        return out_ids, out_scores

    def search_begin(self, slot: int, queries, k: int, out_ids=None, out_scores=None):
        """Enqueue a batch into `slot` and return at once; results are valid after search_end(slot).
        The caller keeps `queries` alive until then."""
        nq, out_ids, out_scores, stream = self._dev_args(queries, int(k), out_ids, out_scores)
        _ffi.check(_ffi.lib().vf_index_search_begin(self._h, int(slot), queries.data_ptr(), nq, int(k),
                                                    out_ids.data_ptr(), out_scores.data_ptr(), stream),
                   "vf_index_search_begin")
        return out_ids, out_scores

    def search_end(self, slot: int):
        _ffi.check(_ffi.lib().vf_index_search_end(self._h, int(slot)), "vf_index_search_end")

    @property
    def slots(self) -> int:
        out = _ffi.c_i32(0)
        _ffi.check(_ffi.lib().vf_index_slots(self._h, ctypes.byref(out)), "vf_index_slots")
        return int(out.value)

    # -- misc --------------------------------------------------------------------------------------
    def shard_devices(self) -> list:
        """Devices of the shards behind this handle ([] for a plain single-device index)."""
        n = _ffi.c_i32(0)
        devs = (_ffi.c_i32 * 64)()
        _ffi.check(_ffi.lib().vf_index_shards(self._h, ctypes.byref(n), devs, 64), "vf_index_shards")
        return [int(devs[i]) for i in range(min(int(n.value), 64))]

    def peer_access(self) -> list:
        """Per shard: True when xGMI peer access between the home device and the shard's device is enabled in both
        directions (or they are the same device); False = that shard's query / result copies are staged through the host."""
        ok = (_ffi.c_i32 * 64)()
        missing = _ffi.c_i32(0)
        _ffi.check(_ffi.lib().vf_index_peer_access(self._h, ok, 64, ctypes.byref(missing)), "vf_index_peer_access")
        return [bool(ok[i]) for i in range(len(self.shard_devices()))]

    def _warn_if_staged(self):
        flags = self.peer_access()
        if flags and not all(flags):
            import warnings
            devs = self.shard_devices()
            warnings.warn("veritasfi_amd: no peer (xGMI) access between the home device and device(s) "
                          f"{[d for d, f in zip(devs, flags) if not f]}: the exchange of those shards is staged through "
                          "the host (correct, slower)", RuntimeWarning, stacklevel=3)

    def stats(self) -> dict:
        st = _ffi.SearchStats()
        _ffi.check(_ffi.lib().vf_index_stats(self._h, ctypes.byref(st)), "vf_index_stats")
        return st.as_dict()

    def profile(self) -> dict:
        """HIP-event totals since set_option("profile", 1): main k_scan ms / launches, pipeline ms."""
        ms, n, pipe, nbytes = ctypes.c_double(0), _ffi.c_i64(0), ctypes.c_double(0), _ffi.c_i64(0)
        _ffi.check(_ffi.lib().vf_index_profile(self._h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(pipe),
                                               ctypes.byref(nbytes)), "vf_index_profile")
        span, nl = ctypes.c_double(0), _ffi.c_i64(0)
        _ffi.check(_ffi.lib().vf_index_profile_span(self._h, ctypes.byref(span), ctypes.byref(nl)), "vf_index_profile_span")
        return {"scan_ms_total": ms.value, "scan_launches": int(n.value), "pipeline_ms_total": pipe.value,
                "scan_bytes_per_launch": int(nbytes.value), "span_ms": span.value}

    def set_option(self, name: str, value: int) -> None:
        _ffi.check(_ffi.lib().vf_index_set_option(self._h, name.encode(), int(value)), "vf_index_set_option")

    def cosine_matrix_rows(self, ids, extra=None) -> np.ndarray:
        """[n, n] canonical cosine matrix of rows already in this index, picked by global id (``vf_cosine_matrix_rows``): the
        similarity matrix of retrieved chunks without re-embedding their texts.
        ``extra`` ([m, d] fp32): positions whose id is -1 take the next row of ``extra`` instead (``vf_cosine_matrix_rows_mixed``)
        -- texts the corpus does not hold, embedded by the caller."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).ravel()
        out = np.empty((ids.size, ids.size), np.float32)
        if not ids.size:
            return out
        if extra is None or len(extra) == 0:
            _ffi.check(_ffi.lib().vf_cosine_matrix_rows(self._h, ids.ctypes.data, int(ids.size), out.ctypes.data),
                       "vf_cosine_matrix_rows")
            return out
        extra = np.ascontiguousarray(extra, dtype=np.float32)
        if extra.ndim != 2 or extra.shape[1] != self.d:
            raise ValueError(f"extra must be [m, {self.d}]")
        _ffi.check(_ffi.lib().vf_cosine_matrix_rows_mixed(self._h, ids.ctypes.data, int(ids.size), extra.ctypes.data,
                                                          int(extra.shape[0]), out.ctypes.data), "vf_cosine_matrix_rows_mixed")
        return out

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _ffi.lib().vf_index_destroy(self._h)
            self._h = _ffi.vp()
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def cosine_scores(a, b, device_id: int = 0) -> np.ndarray:
    """Canonical cosine matrix [na, nb] (step3_mul.py:275 ``cosine_similarity(E, C)``)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("cosine_scores: a [na, d], b [nb, d]")
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.float32)
    _ffi.check(_ffi.lib().vf_cosine_scores(a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], a.shape[1],
                                           out.ctypes.data, int(device_id)), "vf_cosine_scores")
    return out


def cosine_matrix(x, device_id: int = 0) -> np.ndarray:
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    out = np.empty((x.shape[0], x.shape[0]), dtype=np.float32)
    _ffi.check(_ffi.lib().vf_cosine_matrix(x.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data, int(device_id)),
               "vf_cosine_matrix")
    return out


def merge_topk_device(ids_parts, score_parts, k: int):
    """[G, nq, k] CUDA tensors (parts in ascending id-range order) -> ([nq, k], [nq, k])."""
    import torch
    g, nq, kk = ids_parts.shape
    assert kk == k and ids_parts.is_contiguous() and score_parts.is_contiguous()
    ids = torch.empty((nq, k), dtype=torch.int64, device=ids_parts.device)
    sc = torch.empty((nq, k), dtype=torch.float32, device=ids_parts.device)
    dev = ids_parts.device.index or 0
    _ffi.check(_ffi.lib().vf_merge_topk_device(ids_parts.data_ptr(), score_parts.data_ptr(), g, nq, k, ids.data_ptr(),
                                               sc.data_ptr(), dev, torch.cuda.current_stream(ids_parts.device).cuda_stream),
               "vf_merge_topk_device")
    return ids, sc


def packed_part_bytes(nq: int, k: int) -> int:
    """Bytes of one packed per-shard result: [ids nq*k int64][scores nq*k fp32], padded to a multiple of 16 so that
    every part of an all-gathered buffer keeps its int64 ids aligned (the library computes the same stride)."""
    return (nq * k * 12 + 15) // 16 * 16


def packed_result_buffer(nq: int, k: int, device):
    """One contiguous device blob [ids nq*k int64][scores nq*k fp32][pad to 16 B] plus the two typed views into it:
    a shard writes its search result through the views and ships the blob with a single all-gather."""
    import torch
    blob = torch.zeros(packed_part_bytes(nq, k), dtype=torch.uint8, device=device)
    ids = blob[: nq * k * 8].view(torch.int64).view(nq, k)
    scores = blob[nq * k * 8: nq * k * 12].view(torch.float32).view(nq, k)
    return blob, ids, scores


def merge_topk_packed_device(parts_blob, nparts: int, nq: int, k: int, out_ids=None, out_scores=None):
    """parts_blob: uint8 tensor of nparts packed results (rank order == ascending id ranges)."""
    import torch
    dev = parts_blob.device
    if out_ids is None:
        out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
    if out_scores is None:
        out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    _ffi.check(_ffi.lib().vf_merge_topk_packed_device(parts_blob.data_ptr(), nparts, nq, k, out_ids.data_ptr(),
                                                      out_scores.data_ptr(), dev.index or 0,
                                                      torch.cuda.current_stream(dev).cuda_stream),
               "vf_merge_topk_packed_device")
    return out_ids, out_scores


def fuse_rank(rerank_scores, time_scores, device_id: int = 0):
    a = np.ascontiguousarray(np.asarray(rerank_scores, dtype=np.float32))
    b = np.ascontiguousarray(np.asarray(time_scores, dtype=np.float32))
    assert a.shape == b.shape and a.ndim == 1
    out = np.empty_like(a)
    order = np.empty(a.shape[0], dtype=np.int64)
    _ffi.check(_ffi.lib().vf_fuse_rank(a.ctypes.data, b.ctypes.data, a.shape[0], out.ctypes.data, order.ctypes.data,
                                       int(device_id)), "vf_fuse_rank")
    return out, order
