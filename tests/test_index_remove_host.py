"""Removing rows, the parts that need no GPU: compacting a corpus file (``corpus_file.remove``) and the argument errors of the removal
flag (``VF_INDEX_REMOVE`` as the whole dtype of ``vf_index_create``), which the library reports before its first HIP call -- so they
are the same on a box without a device.

Of the six argument errors, null ``out`` and a null handle can be provoked here.  The other four -- ``d`` mismatch, device mismatch, null
ids with ``n_ids > 0``, negative ``n_ids`` -- are compared against a LIVE handle, and a handle only exists where a device built it: they are
checked in tests/test_gpu_index_remove.py (``test_errors_leave_the_index_as_it_was``).  The library reports them from the same block of
code, before its first HIP call (``remove_entry`` in vf_api.hip)."""
import ctypes
import os

import numpy as np
import pytest

from veritasfi_amd import _ffi, corpus_file

VF_EINVAL = -1


def _rows(n, d, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).itemsize == 1:
        return rng.integers(-100 if dtype == np.int8 else 0, 100, size=(n, d)).astype(dtype)
    return rng.standard_normal((n, d)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.uint8, np.int8])   # (uint8: e4m3 codes)
def test_remove_without_an_id_table(tmp_path, dtype):
    path = str(tmp_path / "c.vfc")
    a = _rows(23, 24, dtype, 1)
    corpus_file.write(path, a, e4m3=dtype == np.uint8)
    gone = [0, 22, 7, 8, 9, 7, 0]                                      # first, last, a run; duplicates count once
    assert corpus_file.remove(path, gone) == 5
    h = corpus_file.read_header(path)
    assert (h["n"], h["d"], h["dtype"], h["has_ids"]) == (18, 24, corpus_file._DT[np.dtype(dtype)], False)
    assert np.array_equal(np.asarray(corpus_file.rows_memmap(path)), np.delete(a, gone, 0))
    assert corpus_file.external_ids(path) is None
    assert os.path.getsize(path) == 64 + 18 * 24 * np.dtype(dtype).itemsize
    assert os.listdir(tmp_path) == ["c.vfc"]                           # the temporary file is gone
    assert corpus_file.remove(path, np.arange(18, dtype=np.int32)) == 18   # every row: an empty file that still validates
    assert corpus_file.read_header(path)["n"] == 0 and os.path.getsize(path) == 64


@pytest.mark.parametrize("dtype", [np.float16, np.int8])
def test_remove_with_an_id_table(tmp_path, dtype):
    path = str(tmp_path / "c.vfc")
    a, ids = _rows(15, 16, dtype, 2), np.arange(100, 115)
    corpus_file.write(path, a, ids=ids)
    assert corpus_file.remove(path, np.array([3, 14, 3])) == 2
    assert corpus_file.read_header(path) == {"n": 13, "d": 16, "dtype": corpus_file._DT[np.dtype(dtype)], "has_ids": True}
    assert np.array_equal(np.asarray(corpus_file.rows_memmap(path)), np.delete(a, [3, 14], 0))
    assert np.array_equal(np.asarray(corpus_file.external_ids(path)), np.delete(ids, [3, 14]))
    assert os.path.getsize(path) == 64 + 13 * 16 * np.dtype(dtype).itemsize + 13 * 8
    assert os.listdir(tmp_path) == ["c.vfc"]
    # what a live index does in the same order: remove, then append -- the file keeps step
    b = _rows(2, 16, dtype, 3)
    assert corpus_file.append(path, b, ids=np.array([7, 8])) == 13
    assert np.array_equal(np.asarray(corpus_file.rows_memmap(path)), np.concatenate([np.delete(a, [3, 14], 0), b]))


def test_remove_in_blocks_smaller_than_the_file(tmp_path):
    path = str(tmp_path / "c.vfc")
    a = _rows(101, 8, np.float32, 4)
    corpus_file.write(path, a, ids=np.arange(101))
    gone = np.array([0, 6, 7, 8, 50, 100])
    assert corpus_file.remove(path, gone, block_rows=7) == 6
    assert np.array_equal(np.asarray(corpus_file.rows_memmap(path)), np.delete(a, gone, 0))
    assert np.array_equal(np.asarray(corpus_file.external_ids(path)), np.delete(np.arange(101), gone))


@pytest.mark.parametrize("bad", [[5, 12], [-1], [0, 1, 2 ** 40]])
def test_an_out_of_range_id_leaves_the_file_as_it_was(tmp_path, bad):
    path = str(tmp_path / "c.vfc")
    corpus_file.write(path, _rows(12, 8, np.int8, 5), ids=np.arange(12))
    before = open(path, "rb").read()
    with pytest.raises(ValueError, match=r"ids\[\d\]"):
        corpus_file.remove(path, bad)
    assert open(path, "rb").read() == before and os.listdir(tmp_path) == ["c.vfc"]
    assert corpus_file.remove(path, []) == 0                           # no ids: nothing happens
    assert open(path, "rb").read() == before and os.listdir(tmp_path) == ["c.vfc"]


# ---- the removal flag's argument errors: reported before any HIP call, so they are the same without a GPU ----------------------

def _rc(fn_name, handle, ptr, n, d, dtype):
    L = _ffi.lib()
    h = _ffi.vp(handle)
    rc = getattr(L, fn_name)(ctypes.byref(h) if handle is not False else None, ptr, n, d, dtype, 0, 0)
    return rc, _ffi.last_error(), h.value


def test_remove_flag_argument_errors_need_no_device():
    assert _ffi.VF_INDEX_REMOVE == 0x200
    ids = np.zeros(2, np.int64)
    rm = _ffi.VF_INDEX_REMOVE
    rc, msg, h = _rc("vf_index_create", None, ids.ctypes.data, 2, 8, rm)
    assert rc == VF_EINVAL and "VF_INDEX_REMOVE" in msg and "live handle" in msg and h is None, (rc, msg)
    rc, msg, _ = _rc("vf_index_create", None, None, 0, 8, rm)                     # (no ids is fine; no handle is not)
    assert rc == VF_EINVAL and "live handle" in msg, (rc, msg)
    rc, msg, _ = _rc("vf_index_create", False, ids.ctypes.data, 2, 8, rm)
    assert rc == VF_EINVAL and "null out" in msg, (rc, msg)
    # the flag is the whole dtype or it is nothing: with any other bit the value stays an unknown dtype, as before
    for dtype in (rm | _ffi.VF_DTYPE_F16, rm | _ffi.VF_DTYPE_INT8, rm | 4, rm | 0x400, _ffi.VF_INDEX_APPEND | rm, _ffi.VF_INDEX_APPEND | rm | _ffi.VF_DTYPE_F16):
        rc, msg, h = _rc("vf_index_create", None, ids.ctypes.data, 2, 8, dtype)
        assert rc == VF_EINVAL and "unknown dtype" in msg and h is None, (hex(dtype), rc, msg)


def test_there_is_no_device_id_form_of_the_removal():
    ids = np.zeros(2, np.int64)
    rm = _ffi.VF_INDEX_REMOVE
    for dtype in (rm, _ffi.VF_INDEX_APPEND | rm, _ffi.VF_INDEX_APPEND | rm | _ffi.VF_DTYPE_F16, rm | _ffi.VF_DTYPE_F16):
        rc, msg, _ = _rc("vf_index_create_device", None, ids.ctypes.data, 2, 8, dtype)
        assert rc == VF_EINVAL and "unknown dtype" in msg, (hex(dtype), rc, msg)


def test_retriever_refuses_removal_where_it_refuses_appends():
    from veritasfi_amd.faiss_retriever import FaissRetriever

    class _Index:   # records what remove receives
        n, id_offset = 10, 0

        def remove(self, ids):
            self.got = ids
            m = len(np.unique(ids))
            self.n -= m
            return m

    r = FaissRetriever.from_index(_Index(), None)
    with pytest.raises(ValueError):
        r.remove_ids([1])                        # the retriever did not build the index and was not told how it holds its rows
    r = FaissRetriever.from_index(_Index(), None, corpus_dtype="f16")
    assert r.remove_ids([3, 4, 3]) == 2 and r.index.got.dtype == np.int64 and r.index.n == 8
