"""ctypes binding of ``libveritasfi_hip.so`` (C ABI: ``include/veritasfi_hip.h``).

There is NO fallback: if the library is missing or fails to load, every entry point raises.  Build it
with ``python -m veritasfi_amd.build`` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VF_LIB_PATH") or os.path.join(_HERE, "lib", "libveritasfi_hip.so")   # VF_LIB_PATH: A/B builds

VF_OK = 0
VF_DTYPE_F32, VF_DTYPE_F16, VF_DTYPE_FP8_E4M3, VF_DTYPE_INT8 = 0, 1, 2, 3
VF_INDEX_APPEND = 0x100   # or'ed into the dtype of vf_index_create / vf_index_create_device: append to the handle in *out
VF_INDEX_REMOVE = 0x200   # the whole dtype of vf_index_create: `rows` are int64 ids to remove from the handle in *out

VF_SEARCH_SUBSET = 0x40000000   # or'ed into nq of vf_index_search / vf_index_search_device: `queries` is then a SubsetQuery

c_i32, c_i64, c_f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
p_i32, p_i64, p_f32 = ctypes.POINTER(c_i32), ctypes.POINTER(c_i64), ctypes.POINTER(c_f32)
vp = ctypes.c_void_p


# phases of a live BM25 update, or'ed into the device_id of vf_bm25_create (whose first argument is then a Bm25Delta)
VF_BM25_LIVE, VF_BM25_COMMIT, VF_BM25_DISCARD, VF_BM25_FETCH = 0x1000, 0x2000, 0x4000, 0x8000


class Bm25Delta(ctypes.Structure):
    """vf_bm25_delta of include/veritasfi_hip.h."""
    _fields_ = [
        ("vocab", c_i64), ("n_new", c_i64), ("indptr", ctypes.POINTER(c_i64)), ("rows", ctypes.POINTER(c_i32)),
        ("tf", ctypes.POINTER(c_i32)), ("remove", ctypes.POINTER(c_i64)), ("n_remove", c_i64), ("counts", ctypes.POINTER(c_i64)),
        ("n_removed", c_i64), ("idf", ctypes.POINTER(ctypes.c_double)), ("avgdl", ctypes.c_double), ("k1", ctypes.c_double),
        ("b", ctypes.c_double), ("chunk", c_i32), ("out_indptr", ctypes.POINTER(c_i64)), ("out_indices", ctypes.POINTER(c_i32)),
        ("out_data", ctypes.POINTER(c_f32)), ("out_tf", ctypes.POINTER(c_i32)), ("out_doc_len", ctypes.POINTER(c_i32)),
    ]


VF_BM25_FILTER = 0x40000000   # or'ed into nq of vf_bm25_search: `q_offsets` is then a Bm25FilterQuery


class Bm25FilterQuery(ctypes.Structure):
    """vf_bm25_filter_query of include/veritasfi_hip.h (host memory): the query offsets, the bitmap of the rows that may be returned
    (uint32 words, bit r & 31 of word r >> 5) and the document count the bitmap was made for."""
    _fields_ = [("q_offsets", ctypes.POINTER(c_i64)), ("allow", ctypes.POINTER(ctypes.c_uint32)), ("n_docs", c_i64)]


# or'ed into nq beside VF_BM25_FILTER: `q_offsets` is then a Bm25SubstatsQuery, and the request is two calls (its two phases)
VF_BM25_SUBSTATS, VF_BM25_SUBSTATS_STAGE, VF_BM25_SUBSTATS_SEARCH = 0x20000000, 1, 2


class Bm25SubstatsQuery(ctypes.Structure):
    """vf_bm25_substats_query of include/veritasfi_hip.h: Bm25FilterQuery's three members, the phase, what the stage writes (df per
    q_terms position, the allowed rows' tokens, their number, the handle's update generation) and what the search reads (idf per
    position, avgdl, k1, b and that generation)."""
    _fields_ = [("q_offsets", ctypes.POINTER(c_i64)), ("allow", ctypes.POINTER(ctypes.c_uint32)), ("n_docs", c_i64),
                ("phase", c_i32), ("df", ctypes.POINTER(c_i64)), ("total_len", c_i64), ("m", c_i64), ("generation", ctypes.c_uint64),
                ("idf", ctypes.POINTER(ctypes.c_double)), ("avgdl", ctypes.c_double), ("k1", ctypes.c_double), ("b", ctypes.c_double)]


# or'ed into nq alone: `q_offsets` is then a Bm25PreparedQuery, and its phase says which of the four calls this is
VF_BM25_PREPARED = 0x10000000
VF_BM25_PREPARED_PREPARE, VF_BM25_PREPARED_ARM, VF_BM25_PREPARED_SEARCH, VF_BM25_PREPARED_RELEASE = 1, 2, 3, 4
VF_BM25_PREPARED_CORPUS, VF_BM25_PREPARED_SUBSET = 0, 1
VF_BM25_PREPARED_PER_QUERY = 2   # `mode` of a search: `tokens` [nq] names a prepared filter per query, 0 = none


class Bm25PreparedQuery(ctypes.Structure):
    """vf_bm25_prepared_query of include/veritasfi_hip.h: a row filter kept on the device.  Prepare reads allow, n_docs, mode, chunk
    (and vocab, df in subset mode) and writes token, m, generation, bytes (and total_len, df); arm reads token, vocab, idf, avgdl, k1, b;
    search reads token and q_offsets -- or, with mode VF_BM25_PREPARED_PER_QUERY, tokens [nq] in place of token; release reads token."""
    _fields_ = [("q_offsets", ctypes.POINTER(c_i64)), ("allow", ctypes.POINTER(ctypes.c_uint32)), ("n_docs", c_i64),
                ("phase", c_i32), ("mode", c_i32), ("token", ctypes.c_uint64), ("vocab", c_i64), ("df", ctypes.POINTER(c_i64)),
                ("total_len", c_i64), ("m", c_i64), ("generation", ctypes.c_uint64), ("bytes", c_i64),
                ("idf", ctypes.POINTER(ctypes.c_double)), ("avgdl", ctypes.c_double), ("k1", ctypes.c_double), ("b", ctypes.c_double),
                ("chunk", c_i32), ("tokens", ctypes.POINTER(ctypes.c_uint64))]


class SubsetQuery(ctypes.Structure):
    """vf_subset_query of include/veritasfi_hip.h: what `queries` points to when nq carries VF_SEARCH_SUBSET (host memory; in the
    device form the two pointers inside are device pointers)."""
    _fields_ = [("queries", ctypes.c_void_p), ("ids", ctypes.c_void_p), ("n_ids", ctypes.c_int64)]


def search_subset(L, handle, queries_ptr, nq, k, ids_ptr, n_ids, out_ids_ptr, out_scores_ptr) -> int:
    """vf_index_search in its subset form; returns the code."""
    sq = SubsetQuery(queries_ptr, ids_ptr, n_ids)
    return L.vf_index_search(handle, ctypes.addressof(sq), int(nq) | VF_SEARCH_SUBSET, k, out_ids_ptr, out_scores_ptr)


def search_subset_device(L, handle, d_queries_ptr, nq, k, d_ids_ptr, n_ids, d_out_ids_ptr, d_out_scores_ptr, stream) -> int:
    """vf_index_search_device in its subset form; returns the code."""
    sq = SubsetQuery(d_queries_ptr, d_ids_ptr, n_ids)
    return L.vf_index_search_device(handle, ctypes.addressof(sq), int(nq) | VF_SEARCH_SUBSET, k, d_out_ids_ptr, d_out_scores_ptr, stream)


VF_SEARCH_SUBSETS = 0x20000000  # or'ed into nq of vf_index_search / vf_index_search_device: `queries` is then a SubsetsQuery


class SubsetsQuery(ctypes.Structure):
    """vf_subsets_query of include/veritasfi_hip.h: a list PER QUERY (host memory; `lists`, `n_ids` and `list_of` are host arrays, the
    pointers `queries` and lists[j] are host or device pointers by the call's form)."""
    _fields_ = [("queries", ctypes.c_void_p), ("lists", ctypes.POINTER(ctypes.c_void_p)), ("n_ids", ctypes.POINTER(c_i64)),
                ("n_lists", c_i32), ("list_of", ctypes.POINTER(c_i32))]


def _subsets_query(queries_ptr, list_ptrs, n_ids, list_of):
    """(SubsetsQuery, the arrays it points into): the caller keeps the second alive for the call."""
    n = len(list_ptrs)
    lists = (ctypes.c_void_p * max(n, 1))(*[int(p) if p else None for p in list_ptrs])
    lens = (c_i64 * max(n, 1))(*[int(v) for v in n_ids])
    of = (c_i32 * max(len(list_of), 1))(*[int(v) for v in list_of])
    sq = SubsetsQuery(queries_ptr, ctypes.cast(lists, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(lens, ctypes.POINTER(c_i64)), n,
                      ctypes.cast(of, ctypes.POINTER(c_i32)))
    return sq, (lists, lens, of)


def search_subsets(L, handle, queries_ptr, nq, k, list_ptrs, n_ids, list_of, out_ids_ptr, out_scores_ptr) -> int:
    """vf_index_search with a list per query (host pointers): query i is searched under list_ptrs[list_of[i]]; returns the code."""
    sq, keep = _subsets_query(queries_ptr, list_ptrs, n_ids, list_of)
    return L.vf_index_search(handle, ctypes.addressof(sq), int(nq) | VF_SEARCH_SUBSETS, k, out_ids_ptr, out_scores_ptr)


def search_subsets_device(L, handle, d_queries_ptr, nq, k, d_list_ptrs, n_ids, list_of, d_out_ids_ptr, d_out_scores_ptr, stream) -> int:
    """vf_index_search_device with a list per query (device pointers); returns the code."""
    sq, keep = _subsets_query(d_queries_ptr, d_list_ptrs, n_ids, list_of)
    return L.vf_index_search_device(handle, ctypes.addressof(sq), int(nq) | VF_SEARCH_SUBSETS, k, d_out_ids_ptr, d_out_scores_ptr, stream)


VF_SEARCH_WHERE = 0x10000000   # or'ed into nq of vf_index_search_device: `d_queries` is then a WhereQuery; the count bits are 0


class WhereColumnPtr(ctypes.Structure):
    """vf_where_column of include/veritasfi_hip.h: one field's int64 keys and its validity words (device pointers; valid NULL = every
    row has the field)."""
    _fields_ = [("keys", ctypes.c_void_p), ("valid", ctypes.c_void_p)]


class WhereLeaf(ctypes.Structure):
    """vf_where_leaf: kind 0 an inclusive key interval [lo, hi] (lo > hi passes nothing), kind 1 membership in the strictly ascending
    run set_values[lo : lo + hi], kind 2 "the row lacks the field" -- the layout of ``where.LEAF_DTYPE``."""
    _fields_ = [("kind", c_i32), ("column", c_i32), ("lo", c_i64), ("hi", c_i64)]


class WhereQuery(ctypes.Structure):
    """vf_where_query: a compiled filter (``where.WhereProgram``) and its outputs.  Host memory, as are ``columns``, ``leaves``, ``ops``
    and ``set_values``; the pointers inside ``columns``, ``d_bitmap`` (2 * ceil(n / 64) uint32 words) and ``d_ids`` (int64, ids_cap >= n, or
    NULL) are device pointers.  ``m`` is written by the call.  Limits: 64 leaves, 128 ops, stack depth 32, 16 columns, 65 536 set values."""
    _fields_ = [("n", c_i64), ("columns", ctypes.POINTER(WhereColumnPtr)), ("n_columns", c_i32), ("leaves", ctypes.c_void_p), ("n_leaves", c_i32),
                ("ops", ctypes.c_void_p), ("n_ops", c_i32), ("set_values", ctypes.c_void_p), ("n_set_values", c_i64),
                ("d_bitmap", ctypes.c_void_p), ("d_ids", ctypes.c_void_p), ("ids_cap", c_i64), ("m", c_i64), ("tile_rows", c_i32)]


def eval_where_device(L, handle, n, column_ptrs, leaves, ops, set_values, d_bitmap_ptr, d_ids_ptr, ids_cap, stream, tile_rows=0, flags=0,
                      host_form=False):
    """vf_index_search_device in its VF_SEARCH_WHERE form; returns (code, m).  column_ptrs: [(keys device pointer, valid device pointer
    or None)]; leaves: a ``where.LEAF_DTYPE`` array; ops: uint8; set_values: int64 (host arrays).  ``flags`` is or'ed into nq and
    ``host_form`` sends the call to vf_index_search: both exist for the tests of the refusals."""
    import numpy as np
    cols = (WhereColumnPtr * max(len(column_ptrs), 1))(*[WhereColumnPtr(int(k) if k else None, int(v) if v else None) for k, v in column_ptrs])
    leaves = np.ascontiguousarray(leaves)
    ops = np.ascontiguousarray(ops, dtype=np.uint8)
    sets = np.ascontiguousarray(set_values, dtype=np.int64)
    wq = WhereQuery(int(n), ctypes.cast(cols, ctypes.POINTER(WhereColumnPtr)), len(column_ptrs), leaves.ctypes.data if leaves.size else None,
                    int(leaves.shape[0]), ops.ctypes.data if ops.size else None, int(ops.size), sets.ctypes.data if sets.size else None, int(sets.size),
                    d_bitmap_ptr, d_ids_ptr, int(ids_cap), -1, int(tile_rows))
    nq = VF_SEARCH_WHERE | int(flags)
    if host_form:
        rc = L.vf_index_search(handle, ctypes.addressof(wq), nq, 0, None, None)
    else:
        rc = L.vf_index_search_device(handle, ctypes.addressof(wq), nq, 0, None, None, stream)
    return rc, int(wq.m)


class EncoderConfig(ctypes.Structure):
    _fields_ = [
        ("vocab", c_i32), ("hidden", c_i32), ("layers", c_i32), ("heads", c_i32), ("ffn", c_i32), ("max_pos", c_i32),
        ("type_vocab", c_i32), ("roberta_pad_idx", c_i32), ("pooling", c_i32), ("normalize", c_i32), ("head", c_i32),
        ("ln_eps", c_f32),
    ]


class DecoderConfig(ctypes.Structure):
    _fields_ = [
        ("vocab", c_i32), ("hidden", c_i32), ("layers", c_i32), ("heads", c_i32), ("kv_heads", c_i32), ("head_dim", c_i32),
        ("ffn", c_i32), ("rope_theta", c_f32), ("rms_eps", c_f32), ("qk_norm", c_i32), ("pooling", c_i32),
        ("normalize", c_i32), ("head", c_i32), ("act", c_i32), ("norm_plus_one", c_i32), ("embed_scale", c_f32),
    ]


class VitConfig(ctypes.Structure):
    _fields_ = [
        ("image", c_i32), ("patch", c_i32), ("channels", c_i32), ("hidden", c_i32), ("layers", c_i32), ("heads", c_i32),
        ("ffn", c_i32), ("proj_dim", c_i32), ("act", c_i32), ("normalize", c_i32), ("ln_eps", c_f32),
    ]


class ClipTextConfig(ctypes.Structure):
    _fields_ = [
        ("vocab", c_i32), ("max_pos", c_i32), ("hidden", c_i32), ("layers", c_i32), ("heads", c_i32), ("ffn", c_i32),
        ("proj_dim", c_i32), ("act", c_i32), ("eos_token_id", c_i32), ("normalize", c_i32), ("ln_eps", c_f32),
    ]


class SearchStats(ctypes.Structure):
    _fields_ = [
        ("path", c_i64), ("n_queries", c_i64), ("candidates", c_i64), ("max_candidates", c_i64),
        ("uncertified", c_i64), ("overflowed", c_i64), ("exact_reruns", c_i64), ("wide_launches", c_i64), ("wide_queries", c_i64),
        ("aux_cus", c_i64), ("scans_overlap", c_i64), ("scan_kernel", c_i64), ("scan_image", c_i64), ("subset_rows", c_i64), ("subset_tiles", c_i64),
        ("reserved", c_i64 * 1),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


# every symbol include/veritasfi_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "vf_version": (ctypes.c_int, []),
    "vf_last_error": (ctypes.c_char_p, []),
    "vf_device_count": (ctypes.c_int, [p_i32]),
    "vf_index_create": (ctypes.c_int, [ctypes.POINTER(vp), vp, c_i64, c_i32, c_i32, c_i32, c_i64]),
    "vf_index_create_device": (ctypes.c_int, [ctypes.POINTER(vp), vp, c_i64, c_i32, c_i32, c_i32, c_i64]),
    "vf_index_create_sharded": (ctypes.c_int, [ctypes.POINTER(vp), vp, c_i64, c_i32, c_i32, p_i32, c_i32]),
    "vf_index_create_sharded_from_file": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_char_p, p_i32, c_i32]),
    "vf_index_group": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.POINTER(vp), c_i32]),
    "vf_index_shards": (ctypes.c_int, [vp, p_i32, p_i32, c_i32]),
    "vf_index_peer_access": (ctypes.c_int, [vp, p_i32, c_i32, p_i32]),
    "vf_corpus_file_info": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(c_i64), ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), ctypes.POINTER(c_i32)]),
    "vf_index_create_from_file": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_char_p, c_i64, c_i64, c_i32, c_i64]),
    "vf_index_search": (ctypes.c_int, [vp, vp, c_i32, c_i32, vp, vp]),
    "vf_index_search_device": (ctypes.c_int, [vp, vp, c_i32, c_i32, vp, vp, vp]),
    "vf_index_slots": (ctypes.c_int, [vp, p_i32]),
    "vf_index_search_begin": (ctypes.c_int, [vp, c_i32, vp, c_i32, c_i32, vp, vp, vp]),
    "vf_index_search_end": (ctypes.c_int, [vp, c_i32]),
    "vf_index_info": (ctypes.c_int, [vp, p_i64, p_i32, p_i32, p_i32]),
    "vf_index_stats": (ctypes.c_int, [vp, ctypes.POINTER(SearchStats)]),
    "vf_index_set_option": (ctypes.c_int, [vp, ctypes.c_char_p, c_i64]),
    "vf_index_profile": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double), p_i64, ctypes.POINTER(ctypes.c_double), p_i64]),
    "vf_index_profile_span": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double), p_i64]),
    "vf_index_debug_read": (ctypes.c_int, [vp, c_i32, vp, c_i64]),
    "vf_index_destroy": (ctypes.c_int, [vp]),
    "vf_cosine_matrix": (ctypes.c_int, [vp, c_i32, c_i32, vp, c_i32]),
    "vf_cosine_matrix_rows": (ctypes.c_int, [vp, vp, c_i32, vp]),
    "vf_cosine_matrix_rows_mixed": (ctypes.c_int, [vp, vp, c_i32, vp, c_i32, vp]),
    "vf_cosine_scores": (ctypes.c_int, [vp, c_i32, vp, c_i64, c_i32, vp, c_i32]),
    "vf_merge_topk_device": (ctypes.c_int, [vp, vp, c_i32, c_i32, c_i32, vp, vp, c_i32, vp]),
    "vf_merge_topk_packed_device": (ctypes.c_int, [vp, c_i32, c_i32, c_i32, vp, vp, c_i32, vp]),
    "vf_fuse_rank": (ctypes.c_int, [vp, vp, c_i32, vp, vp, c_i32]),
    "vf_encoder_weight_sizes": (ctypes.c_int, [ctypes.POINTER(EncoderConfig), p_i64, p_i64]),
    "vf_encoder_create": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.POINTER(EncoderConfig), vp, c_i64, vp, c_i64, c_i32]),
    "vf_encoder_forward": (ctypes.c_int, [vp, vp, vp, vp, c_i32, c_i32, c_i32, vp]),
    "vf_encoder_forward_pooled": (ctypes.c_int, [vp, vp, vp, vp, c_i32, c_i32, c_i32, c_i32, c_i32, vp]),
    "vf_encoder_forward_hidden": (ctypes.c_int, [vp, vp, vp, vp, c_i32, c_i32, vp]),
    "vf_encoder_info": (ctypes.c_int, [vp, ctypes.POINTER(EncoderConfig)]),
    "vf_encoder_destroy": (ctypes.c_int, [vp]),
    "vf_reranker_create": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.POINTER(EncoderConfig), vp, c_i64, vp, c_i64, c_i32]),
    "vf_reranker_score": (ctypes.c_int, [vp, vp, vp, vp, c_i32, c_i32, vp]),
    "vf_reranker_destroy": (ctypes.c_int, [vp]),
    "vf_decoder_weight_sizes": (ctypes.c_int, [vp, p_i64, p_i64]),
    "vf_decoder_create": (ctypes.c_int, [ctypes.POINTER(vp), vp, vp, c_i64, vp, c_i64, c_i32]),
    "vf_decoder_forward": (ctypes.c_int, [vp, vp, vp, c_i32, c_i32, c_i32, vp]),
    "vf_decoder_forward_pooled": (ctypes.c_int, [vp, vp, vp, c_i32, c_i32, c_i32, c_i32, vp]),
    "vf_decoder_forward_hidden": (ctypes.c_int, [vp, vp, vp, c_i32, c_i32, vp]),
    "vf_decoder_destroy": (ctypes.c_int, [vp]),
    "vf_vit_weight_sizes": (ctypes.c_int, [ctypes.POINTER(VitConfig), p_i64, p_i64]),
    "vf_vit_create": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.POINTER(VitConfig), vp, c_i64, vp, c_i64, c_i32]),
    "vf_vit_forward": (ctypes.c_int, [vp, vp, c_i32, vp]),
    "vf_vit_forward_u8": (ctypes.c_int, [vp, vp, vp, vp, c_i32, vp]),
    "vf_vit_destroy": (ctypes.c_int, [vp]),
    "vf_clip_text_weight_sizes": (ctypes.c_int, [ctypes.POINTER(ClipTextConfig), p_i64, p_i64]),
    "vf_clip_text_create": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.POINTER(ClipTextConfig), vp, c_i64, vp, c_i64, c_i32]),
    "vf_clip_text_forward": (ctypes.c_int, [vp, vp, vp, c_i32, c_i32, vp]),
    "vf_clip_text_destroy": (ctypes.c_int, [vp]),
    "vf_bm25_create": (ctypes.c_int, [p_i64, c_i64, p_i32, p_f32, c_i64, c_i64, c_i32, ctypes.POINTER(vp), p_i32]),
    "vf_bm25_search": (ctypes.c_int, [vp, p_i64, p_i32, c_i32, c_i32, p_i64, p_f32]),
}

_lib = None
_lock = threading.Lock()


def lib():
    """Load the HIP library (once).  Raises if it is not built -- there is no CPU path."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"{LIB_PATH} is missing: build it with `python -m veritasfi_amd.build` "
                        "(hipcc --offload-arch=gfx950). veritasfi_amd has no CPU fallback.")
                # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (same SONAME as
                # /opt/rocm's).  Load torch FIRST so our library binds to that copy; the other order
                # leaves torch unable to see the GPU, and device pointers / streams are shared anyway.
                try:
                    import torch  # noqa: F401
                except ImportError:
                    pass
                L = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(L, name)  # AttributeError if the ABI and this table drift apart
                    fn.restype = res
                    fn.argtypes = args
                _lib = L
    return _lib


def loaded() -> bool:
    """The library has been loaded in this process (an index, a model handle or a small dense op was created)."""
    return _lib is not None


def last_error() -> str:
    msg = lib().vf_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int, what: str = "") -> None:
    """Map a VF_E* code to RuntimeError(vf_last_error()), as SURVEY 8b prescribes."""
    if rc != VF_OK:
        raise RuntimeError(f"{what or 'veritasfi_hip'} failed (rc={rc}): {last_error()}")
