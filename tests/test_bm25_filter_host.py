"""The host side of a filtered BM25 search, CPU-only: the bitmap ``BM25Retriever`` packs from ``subset=`` (``bm25.filter_words``)
against ``np.packbits(..., bitorder="little")``, the ctypes struct against the header, and the ensemble's choice between a retriever
that filters on its own (``filtered_prefix``) and the full ranking filtered on the host."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_ensemble_where import Store, SubsetCosineRetriever, _passes, _world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _want_words(mask):
    n = len(mask)
    padded = np.zeros((n + 31) // 32 * 32, np.uint8)
    padded[:n] = mask
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 1000, 70001])
def test_ids_and_masks_pack_to_little_endian_bit_words(n):
    from veritasfi_amd.bm25 import filter_words
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.3
    mask[n - 1] = True                                  # the last word's last valid bit
    want = _want_words(mask)
    assert want.size == (n + 31) // 32
    ids = np.flatnonzero(mask)
    shuffled = rng.permutation(np.concatenate([ids, ids[: max(1, ids.size // 3)]]))   # unsorted, with repeats: they count once
    for subset in (mask, ids, ids.astype(np.int32), ids.tolist(), shuffled):
        words, m = filter_words(subset, n)
        assert words.dtype == np.uint32 and words.flags["C_CONTIGUOUS"] and np.array_equal(words, want)
        assert m == int(mask.sum())
    for r in (0, n - 1):                                # bit r & 31 of word r >> 5
        words, m = filter_words([r], n)
        assert m == 1 and words[r >> 5] == np.uint32(1) << np.uint32(r & 31) and int(words.astype(np.uint64).sum()) == 1 << (r & 31)
    words, m = filter_words([], n)
    assert m == 0 and words.size == (n + 31) // 32 and not words.any()
    words, m = filter_words(np.ones(n, bool), n)
    assert m == n and np.array_equal(words, _want_words(np.ones(n, bool)))


def test_bad_subsets_are_refused_by_name():
    from veritasfi_amd.bm25 import filter_words
    with pytest.raises(ValueError, match=r"ids\[2\] = 100 "):
        filter_words([3, 5, 100, 7], 100)
    with pytest.raises(ValueError, match=r"ids\[0\] = -1 "):
        filter_words([-1], 100)
    with pytest.raises(ValueError, match="one entry per row"):
        filter_words(np.ones(99, bool), 100)
    with pytest.raises(ValueError, match="one entry per row"):
        filter_words(np.ones((10, 10), bool), 100)
    with pytest.raises(TypeError):
        filter_words([0.5, 2.0], 100)

    class Opaque:           # a device-resident subset that does not show its host ids
        tensor = object()

    with pytest.raises(TypeError, match="host ids"):
        filter_words(Opaque(), 100)

    class Shown(Opaque):
        ids = np.asarray([4, 9], np.int64)

    words, m = filter_words(Shown(), 100)
    assert m == 2 and words[0] == (1 << 4) | (1 << 9)


def test_the_ctypes_struct_is_the_headers():
    from veritasfi_amd import _ffi
    text = open(os.path.join(ROOT, "include", "veritasfi_hip.h")).read()
    assert re.search(r"#define\s+VF_BM25_FILTER\s+0x40000000\b", text) and _ffi.VF_BM25_FILTER == 0x40000000
    body = re.search(r"typedef struct vf_bm25_filter_query \{(.*?)\} vf_bm25_filter_query;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(" ".join(f.split()[:-1]).replace(" *", "*"), f.split()[-1].lstrip("*")) for f in body.split(";") if f.strip()]
    assert fields == [("const int64_t*", "q_offsets"), ("const uint32_t*", "allow"), ("int64_t", "n_docs")]
    S = _ffi.Bm25FilterQuery
    assert [name for name, _ in S._fields_] == [name for _, name in fields]
    assert S.q_offsets.offset == 0 and S.allow.offset == ctypes.sizeof(ctypes.c_void_p) and S.n_docs.offset == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(S) == 2 * ctypes.sizeof(ctypes.c_void_p) + 8
    assert S._fields_[1][1] is ctypes.POINTER(ctypes.c_uint32) and S._fields_[2][1] is ctypes.c_int64
    from veritasfi_amd.bm25 import BM25Retriever
    assert BM25Retriever.filtered_prefix is True


class _Recording:
    """A BM25 stand-in over a fixed ranking that records what it is asked."""

    def __init__(self, order, scores):
        self.order, self.scores, self.calls = list(order), list(scores), []

    def invoke(self, query, k, subset=None):
        self.calls.append((k, None if subset is None else np.asarray(subset).copy()))
        if subset is None:
            return self.order[:k], self.scores[:k]
        allow = set(int(r) for r in subset)
        kept = [(r, s) for r, s in zip(self.order, self.scores) if r in allow][:k]
        return [r for r, _ in kept], [s for _, s in kept]


class _Filtering(_Recording):
    filtered_prefix = True


def _ensemble(world, bm, **kw):
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, emb, _, _, _ = world
    ts = Store(titles, [None] * len(titles), t_emb.tolist())
    return EnsembleRetriever("unused", Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=bm, retriever_cls=SubsetCosineRetriever, **kw)


@pytest.mark.parametrize("where, bm25_k", [({"company": "other", "year": [2021, 2022]}, 7), ({"company": "lotus", "year": [2020]}, 50)])
def test_a_filtering_retriever_is_asked_for_the_prefix_with_the_passing_rows(where, bm25_k):
    world = _world(2, bundles=False)
    metas, order, scores, queries = world[1], world[6], world[7], world[8]
    keep = [i for i, md in enumerate(metas) if _passes(md, where)]
    assert 0 < len(keep) < len(metas)
    outs = []
    for cls in (_Filtering, _Recording):
        bm = cls(order, scores)
        er = _ensemble(world, bm, faiss_k=0, faiss_ts_k=0, bm25_k=bm25_k)
        outs.append(er.invoke(queries[0][0], [], where=where))
        if cls is _Filtering:
            assert len(bm.calls) == 1 and bm.calls[0][0] == min(bm25_k, len(keep)) != len(metas), "never the full ranking"
            assert np.array_equal(bm.calls[0][1], keep), "subset= the passing rows, sorted"
        else:
            assert len(bm.calls) == 1 and bm.calls[0][0] == len(metas) and bm.calls[0][1] is None, "a plain retriever keeps the full ranking"
        er.invoke(queries[0][0], [])                        # unfiltered: no subset, whatever the retriever declares
        assert bm.calls[-1][1] is None
    assert outs[0] == outs[1] and len(outs[0]) == min(bm25_k, len(keep))
    want_rows = [r for r in order if r in set(keep)][:bm25_k]
    assert [c["metadata"]["doc_id"] for c in outs[0]] == [f"d{r}" for r in want_rows]
