"""Appending rows, the parts that need no GPU: extending a corpus file (``corpus_file.CorpusWriter(mode="a")`` / ``corpus_file.append``)
and the argument errors of the append flag (``VF_INDEX_APPEND`` or'ed into the dtype of ``vf_index_create*``), which the library
reports before its first HIP call -- so they are the same on a box without a device."""
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


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.uint8, np.int8])
def test_append_round_trip_without_ids(tmp_path, dtype):
    path = str(tmp_path / "c.vfc")
    a, b, c = _rows(7, 24, dtype, 1), _rows(5, 24, dtype, 2), _rows(1, 24, dtype, 3)
    corpus_file.write(path, a)
    assert corpus_file.append(path, b) == 7
    with corpus_file.CorpusWriter(path, mode="a") as w:
        assert (w.n, w.d, w.dtype) == (12, 24, np.dtype(dtype))
        w.append(c)
    h = corpus_file.read_header(path)
    assert (h["n"], h["d"], h["has_ids"]) == (13, 24, False)
    assert np.array_equal(np.asarray(corpus_file.rows_memmap(path)), np.concatenate([a, b, c]))
    assert corpus_file.external_ids(path) is None
    assert os.path.getsize(path) == 64 + 13 * 24 * np.dtype(dtype).itemsize


def test_append_round_trip_with_ids(tmp_path):
    path = str(tmp_path / "c.vfc")
    a, b = _rows(6, 16, np.float16, 1), _rows(9, 16, np.float16, 2)
    ia, ib = np.arange(100, 106), np.arange(900, 909)
    corpus_file.write(path, a, ids=ia)
    assert corpus_file.append(path, b, ids=ib) == 6
    assert corpus_file.read_header(path) == {"n": 15, "d": 16, "dtype": _ffi.VF_DTYPE_F16, "has_ids": True}
    assert np.array_equal(np.asarray(corpus_file.rows_memmap(path)), np.concatenate([a, b]))
    assert np.array_equal(np.asarray(corpus_file.external_ids(path)), np.concatenate([ia, ib]))
    assert os.path.getsize(path) == 64 + 15 * 16 * 2 + 15 * 8


def test_append_refuses_another_width_type_or_id_presence(tmp_path):
    plain, with_ids = str(tmp_path / "p.vfc"), str(tmp_path / "i.vfc")
    a = _rows(4, 16, np.float16, 1)
    corpus_file.write(plain, a)
    corpus_file.write(with_ids, a, ids=np.arange(4))
    before = open(plain, "rb").read(), open(with_ids, "rb").read()
    with pytest.raises(ValueError):
        corpus_file.append(plain, _rows(2, 17, np.float16, 2))                    # d
    with pytest.raises(ValueError):
        corpus_file.append(plain, _rows(2, 16, np.int8, 2))                       # dtype (one-byte rows are never cast)
    with pytest.raises(ValueError):
        corpus_file.CorpusWriter(plain, d=17, mode="a")
    with pytest.raises(ValueError):
        corpus_file.CorpusWriter(plain, dtype=np.float32, mode="a")
    with pytest.raises(ValueError):
        corpus_file.CorpusWriter(plain, e4m3=True, mode="a")
    with pytest.raises(ValueError):
        corpus_file.append(plain, _rows(2, 16, np.float16, 2), ids=np.arange(2))  # ids into a file without a table
    with pytest.raises(ValueError):
        corpus_file.append(with_ids, _rows(2, 16, np.float16, 2))                 # no ids into a file with one
    with pytest.raises(ValueError):
        corpus_file.append(with_ids, _rows(2, 16, np.float16, 2), ids=np.arange(3))
    with pytest.raises(ValueError):
        corpus_file.CorpusWriter(str(tmp_path / "missing.vfc"), d=16, mode="x")
    with pytest.raises(OSError):
        corpus_file.CorpusWriter(str(tmp_path / "missing.vfc"), mode="a")
    # every refusal left its file as it was, bytes and all (the id table too: abort puts it back)
    assert (open(plain, "rb").read(), open(with_ids, "rb").read()) == before


def test_header_keeps_the_old_row_count_until_close(tmp_path):
    path = str(tmp_path / "c.vfc")
    a, b = _rows(5, 8, np.float32, 1), _rows(3, 8, np.float32, 2)
    corpus_file.write(path, a)
    w = corpus_file.CorpusWriter(path, mode="a")
    w.append(b)
    w._f.flush()
    # mid-append: the new rows are in the file, the header does not name them yet, and the old rows read as before
    assert os.path.getsize(path) == 64 + 8 * 8 * 4
    assert corpus_file.read_header(path)["n"] == 5
    assert np.array_equal(np.asarray(corpus_file.rows_memmap(path)), a)
    w.close()
    assert corpus_file.read_header(path)["n"] == 8
    assert np.array_equal(np.asarray(corpus_file.rows_memmap(path)), np.concatenate([a, b]))


def test_abort_restores_a_file_with_an_id_table(tmp_path):
    path = str(tmp_path / "c.vfc")
    a = _rows(5, 8, np.int8, 1)
    corpus_file.write(path, a, ids=np.arange(50, 55))
    before = open(path, "rb").read()
    with pytest.raises(RuntimeError):
        with corpus_file.CorpusWriter(path, mode="a") as w:
            w.append(_rows(4, 8, np.int8, 2), ids=np.arange(4))   # lands on the old id table
            raise RuntimeError("embedder failed")
    assert open(path, "rb").read() == before


# ---- the append flag's argument errors: reported before any HIP call, so they are the same without a GPU ----------------------

def _append_rc(fn_name, handle, rows_ptr, n, d, dtype):
    L = _ffi.lib()
    h = _ffi.vp(handle)
    rc = getattr(L, fn_name)(ctypes.byref(h) if handle is not False else None, rows_ptr, n, d, dtype, 0, 0)
    return rc, _ffi.last_error(), h.value


@pytest.mark.parametrize("fn_name", ["vf_index_create", "vf_index_create_device"])
def test_append_flag_argument_errors_need_no_device(fn_name):
    assert _ffi.VF_INDEX_APPEND == 0x100
    buf = np.zeros((2, 8), np.float32)
    ap = _ffi.VF_INDEX_APPEND
    rc, msg, h = _append_rc(fn_name, None, buf.ctypes.data, 2, 8, ap | _ffi.VF_DTYPE_F32)
    assert rc == VF_EINVAL and "live handle" in msg and h is None, (rc, msg)
    rc, msg, _ = _append_rc(fn_name, None, buf.ctypes.data, -1, 8, ap | _ffi.VF_DTYPE_F32)
    assert rc == VF_EINVAL and "bad rows/n/d" in msg, (rc, msg)
    rc, msg, _ = _append_rc(fn_name, None, None, 2, 8, ap | _ffi.VF_DTYPE_F32)
    assert rc == VF_EINVAL and "bad rows/n/d" in msg, (rc, msg)
    rc, msg, _ = _append_rc(fn_name, None, buf.ctypes.data, 2, 8, ap | 4)
    assert rc == VF_EINVAL and "unknown dtype" in msg, (rc, msg)
    rc, msg, _ = _append_rc(fn_name, None, buf.ctypes.data, 2, 8, ap | 0x200 | _ffi.VF_DTYPE_F16)   # no other bit means anything
    assert rc == VF_EINVAL and "unknown dtype" in msg, (rc, msg)
    rc, msg, _ = _append_rc(fn_name, False, buf.ctypes.data, 2, 8, ap | _ffi.VF_DTYPE_F32)
    assert rc == VF_EINVAL and "null out" in msg, (rc, msg)


def test_retriever_encodes_appended_rows_by_the_constructors_recipe():
    """encode_rows is the one recipe behind FaissRetriever(...) and add_embeddings: same input, same stored rows."""
    from veritasfi_amd.faiss_retriever import FaissRetriever, encode_rows
    from veritasfi_amd.index import quantize_int8
    x = np.random.default_rng(3).standard_normal((5, 32)).astype(np.float32)
    rows, e4m3 = encode_rows(x, "int8")
    assert not e4m3 and rows.dtype == np.int8 and np.array_equal(rows, quantize_int8(x))
    rows, e4m3 = encode_rows(x, "fp8")
    assert e4m3 and rows.dtype == np.uint8 and not ((rows & 0x7F) == 0x7F).any()
    assert encode_rows(x, "f16")[0].dtype == np.float16 and encode_rows(x.astype(np.float16), "f32")[0].dtype == np.float16
    with pytest.raises(ValueError):
        encode_rows(x, "bf16")

    class _Index:   # records what add receives
        n, id_offset = 10, 0

        def add(self, rows):
            self.got = rows
            first, self.n = self.n, self.n + len(rows)
            return first

    class _Embedder:
        def embed_query(self, t):
            return [float(len(t)), 1.0, 0.0, 0.0]

    r = FaissRetriever.from_index(_Index(), _Embedder())
    with pytest.raises(ValueError):
        r.add_embeddings(x)                      # the retriever did not build the index and was not told how it holds its rows
    with pytest.raises(ValueError):
        r.add_texts(["a"])
    r = FaissRetriever.from_index(_Index(), _Embedder(), corpus_dtype="int8")
    assert np.array_equal(r.add_embeddings(x), np.arange(10, 15)) and np.array_equal(r.index.got, quantize_int8(x))
    ids = r.add_texts(["ab", "abcd"])            # embed_query per text: this embedder has nothing else
    assert np.array_equal(ids, [15, 16]) and r.index.got.shape == (2, 4) and r.index.got.dtype == np.int8
    assert r.add_texts([]).size == 0
