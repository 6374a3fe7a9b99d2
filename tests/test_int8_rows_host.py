"""int8 rows, the host side (no GPU): the quantiser `quantize_int8` against its formula -- k_prep_image's recipe in fp32 --, the residual
it leaves on N(0, 1) rows, the corpus file of dtype 3 through the writer and the library's own header parser, and the configuration key."""
import numpy as np
import pytest


def _formula(x):
    """sc = absmax / 127 (an fp32 division; zero rows: 1), code = clip(rint(x / sc), -127, 127), element by element in fp32."""
    x = np.asarray(x, dtype=np.float32)
    out = np.empty(x.shape, np.int8)
    for i, row in enumerate(x):
        mx = np.float32(np.abs(row).max())
        sc = np.float32(mx / np.float32(127.0)) if mx > 0 else np.float32(1.0)
        for j, v in enumerate(row):
            q = np.float32(v / sc)
            out[i, j] = int(min(max(np.rint(q), -127.0), 127.0))
    return out


def test_quantize_int8_follows_the_formula_on_its_edge_rows():
    import veritasfi_amd as vf
    rng = np.random.default_rng(5)
    x = rng.standard_normal((9, 40)).astype(np.float32)
    x[1] = 0.0                                               # a zero row: scale 1, codes 0
    x[2] = 0.0; x[2, 7] = -3.0                               # absmax at a negative element: code -127, never -128
    x[3] = np.float32(2.0) * np.arange(40, dtype=np.float32) / np.float32(2.0)
    x[3, :6] = [127.0, 0.5, 1.5, 2.5, -0.5, -3.5]            # sc = 1: x / sc lands on .5 -> ties to even: 0, 2, 2, -0, -4
    x[4] *= 1e-30                                            # tiny rows keep their shape
    x[5] *= 1e30
    codes = vf.quantize_int8(x)
    assert codes.dtype == np.int8 and codes.shape == x.shape
    assert np.array_equal(codes, _formula(x))
    assert not codes[1].any()
    assert codes[2, 7] == -127 and codes[2].astype(np.int32).sum() == -127 and codes.min() >= -127
    assert codes[3, :6].tolist() == [127, 0, 2, 2, 0, -4]
    assert np.abs(codes[[0, 4, 5, 6, 7, 8]].astype(np.int32)).max(axis=1).tolist() == [127] * 6
    # fp16 input is widened exactly, then quantised like fp32 input
    x16 = x[[0, 1, 2, 3, 6]].astype(np.float16)
    assert np.array_equal(vf.quantize_int8(x16), _formula(x16.astype(np.float32)))


def test_quantize_int8_refuses_non_finite_rows_and_other_shapes():
    import veritasfi_amd as vf
    for bad in (np.inf, -np.inf, np.nan):
        x = np.ones((3, 4), np.float32)
        x[1, 2] = bad
        with pytest.raises(ValueError, match="non-finite"):
            vf.quantize_int8(x)
    with pytest.raises(ValueError):
        vf.quantize_int8(np.ones(4, np.float32))


def test_int8_codes_of_normal_rows_leave_less_than_a_64th_of_the_row():
    """rho = ||x - sc code|| / ||x||, the quantity an fp16 index's int8 image is held to (1 / 64): an int8 index made with the same
    recipe is at least as faithful.  4 096 seeded N(0, 1) rows of 768 elements, in fp64."""
    import veritasfi_amd as vf
    x = np.random.default_rng(11).standard_normal((4096, 768)).astype(np.float32)
    codes = vf.quantize_int8(x)
    sc = (np.abs(x).max(axis=1, keepdims=True) / np.float32(127.0)).astype(np.float64)
    rho = np.linalg.norm(x.astype(np.float64) - sc * codes, axis=1) / np.linalg.norm(x.astype(np.float64), axis=1)
    print(f"rho: mean {rho.mean():.5f} max {rho.max():.5f}")
    assert rho.max() <= 1.0 / 64


def test_corpus_file_of_int8_rows_round_trips_as_dtype_3(tmp_path):
    from veritasfi_amd import _ffi, corpus_file
    assert _ffi.VF_DTYPE_INT8 == 3
    rng = np.random.default_rng(3)
    rows = rng.integers(-128, 128, size=(37, 24), dtype=np.int8)
    rows[0, :2] = [-128, 127]
    ids = np.arange(1000, 1037, dtype=np.int64)
    p = str(tmp_path / "i8.vfc")
    corpus_file.write(p, rows, ids)
    assert corpus_file.read_header(p) == {"n": 37, "d": 24, "dtype": 3, "has_ids": True}
    assert corpus_file.info(p) == {"n": 37, "d": 24, "dtype": 3, "has_ids": True}          # the library's parser (vf_corpus_file_info)
    back = corpus_file.rows_memmap(p)
    assert back.dtype == np.int8 and np.array_equal(np.asarray(back), rows)
    assert np.array_equal(np.asarray(corpus_file.external_ids(p)), ids)
    with corpus_file.CorpusWriter(str(tmp_path / "w.vfc"), 24, np.int8) as w:
        w.append(rows[:5])
        with pytest.raises(ValueError):
            w.append(rows[:5].astype(np.int16))             # values that do not fit are not narrowed silently ...
    # a header of dtype 4 is corrupt
    raw = bytearray(open(p, "rb").read())
    raw[12] = 4
    q = str(tmp_path / "i8_bad.vfc")
    open(q, "wb").write(bytes(raw))
    with pytest.raises(Exception, match="corrupt"):
        corpus_file.info(q)
    with pytest.raises(ValueError):
        corpus_file.read_header(q)


def test_from_config_accepts_int8_and_still_rejects_int4():
    import veritasfi_amd as vf
    cfg = {"embeddings_model_name": "BAAI/bge-m3", "rerank_model": "BAAI/bge-reranker-v2-gemma", "rerank_topk": 5}
    for spelled in ("int8", "INT8", "Int8"):
        parts = vf.from_config(dict(cfg, corpus_dtype=spelled), load_models=False)
        assert parts.corpus_dtype == "int8" and parts.retriever_cls.keywords["corpus_dtype"] == "int8"
    with pytest.raises(ValueError, match="corpus_dtype"):
        vf.from_config(dict(cfg, corpus_dtype="int4"), load_models=False)


def test_dense_index_from_int8_refuses_uint8_before_any_device_call():
    import veritasfi_amd as vf
    with pytest.raises(TypeError, match="int8"):
        vf.DenseIndex.from_int8(np.zeros((4, 8), np.uint8))
    with pytest.raises(TypeError, match="int8"):
        vf.DenseIndex.from_int8(np.zeros((4, 8), np.float32))
