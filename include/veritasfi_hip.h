/*
 * veritasfi_hip.h -- C ABI of libveritasfi_hip.so (MI355X / gfx950, hand-written HIP).
 *
 * Drop-in boundary for VeritasFi's dense-retrieval hot path.  The
 * reference is pure Python and delegates this path to third-party objects; each entry point
 * below names the reference call it stands behind (paths relative to the reference root).
 * Plain pointers and sizes only -- no torch / numpy types cross this boundary.  The Python
 * classes in veritasfi_amd/ bind it with ctypes (INTEGRATION.md shows the reference-side stub).
 *
 * Conventions
 *   - every function returns VF_OK (0) or a negative VF_E* code; nothing aborts or throws across
 *     the ABI; vf_last_error() gives a thread-local message for the last failure.
 *   - "host" pointers are caller-owned host memory; "device" pointers (suffix _device / d_*) are
 *     HBM pointers on the index's GPU (e.g. torch tensor .data_ptr()); the library never frees them.
 *   - ranking contract: descending cosine, ties broken by LOWER id first; k > N pads ids with -1
 *     and scores with -FLT_MAX (faiss contract, src/utils/faissRetriever.py:37).
 *   - scores are the CANONICAL fp32 cosine (DESIGN.md "Canonical score"): bit-identical to the CPU
 *     oracle in oracle/vf_oracle.c, independent of sharding, batch size and kernel path.
 *   - zero-norm rows / queries score 0 (sklearn divides by 1: experiments/retriever/step3_mul.py:275).
 *   - a handle may be used from several threads (per-handle mutex); handles are per process.
 */
#ifndef VERITASFI_HIP_H
#define VERITASFI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VF_VERSION 100 /* 0.1.0 */

enum {
    VF_OK = 0,
    VF_EINVAL = -1,       /* bad argument */
    VF_ENOMEM = -2,       /* host or device allocation failed */
    VF_EHIP = -3,         /* a HIP runtime call failed (message has the HIP error string) */
    VF_EUNSUPPORTED = -4, /* valid request this build does not implement (e.g. > 2^32-1 rows per shard) */
    VF_EINTERNAL = -5
};

enum { VF_DTYPE_F32 = 0, VF_DTYPE_F16 = 1, VF_DTYPE_FP8_E4M3 = 2, VF_DTYPE_INT8 = 3 };
#define VF_INDEX_APPEND 0x100   /* or'ed into `dtype` of vf_index_create / vf_index_create_device: append to the handle in *out (below) */
#define VF_INDEX_REMOVE 0x200   /* as the whole `dtype` of vf_index_create: remove rows from the handle in *out (below) */

typedef struct vf_index vf_index;

/* counters of the last search on a handle (for tests / benches; not part of the reference surface) */
typedef struct vf_search_stats {
    int64_t path;            /* 0 = small-N exact dense, 1 = fused MFMA scan, 2 = chunked exact, 3 = subset scan (VF_SEARCH_SUBSET), 4 = a list per query (VF_SEARCH_SUBSETS) */
    int64_t n_queries;
    int64_t candidates;      /* total candidates appended by the fused scan (all queries) */
    int64_t max_candidates;  /* largest per-query candidate count */
    int64_t uncertified;     /* queries whose fused result failed the exactness certificate */
    int64_t overflowed;      /* queries whose candidate buffer overflowed */
    int64_t exact_reruns;    /* queries recomputed by the chunked exact path */
    int64_t wide_launches;   /* k_scan_wide main passes of the call (0: the 64-query HBM-bound scan served it) */
    int64_t wide_queries;    /* queries those passes served (up to 1024 per pass) */
    int64_t aux_cus;         /* CUs the main scan left to the small kernels of the other slots (0 = no CU split) */
    int64_t scans_overlap;   /* 1 = main scans of consecutive slots were not ordered against each other */
    int64_t scan_kernel;     /* main-scan kernel of the call: 1 k_scan (register loads), 2 k_scan2 (whole-line LDS-DMA), 3 k_scan_wide, 4 k_scan_wide8 (fp8 matrix instruction), 5 k_scan2r (k_scan2, half the query image in registers), 6 k_scan_ksplit (rows of 2560 to 4096 padded elements: option "wide_rows"), 7 k_scan_ksplit8 (the same for e4m3 rows) or its int8 form k_scan_ksplit8i (int8 rows report 7 as the int8 forms of k_scan and k_scan_wide report 1 and 3) */
    int64_t scan_image;      /* 1 = the main scan read the int8 row image (option "scan_image"), 0 = the rows as stored */
    int64_t subset_rows;     /* path 3: rows the list of a subset search named (VF_SEARCH_SUBSET); path 4: the sum over the queries of their own list's length */
    int64_t subset_tiles;    /* path 4 only: query tiles k_scan_subset_m scored: per pass, the sum over its lists of ceil(queries of the list / 4) */
    int64_t reserved[1];
} vf_search_stats;

int vf_version(void);
const char* vf_last_error(void);
int vf_device_count(int32_t* out);

/* ---- dense index: replaces faiss.IndexFlatIP + normalize_L2 ---------------------------------
 * src/utils/faissRetriever.py:11-26 (FaissRetriever.__init__): rows [n,d] row-major of `dtype`,
 * copied to device `device_id`.  Rows are stored as given (fp16 rows are the corpus; fp32 rows keep
 * an fp32 copy for exact scoring plus an fp16 scan copy); per-row norms are computed on the GPU.
 * VF_DTYPE_FP8_E4M3 rows (one byte per element, OCP e4m3: bias 7, no infinities, 0x7F / 0xFF = NaN) STAY fp8 in
 * HBM: the fused scan reads the bytes (half the traffic of fp16) and converts them to fp16 in registers -- exactly,
 * every e4m3 value is an fp16 value -- and the exact re-score decodes the same bytes.  A per-row scale of a
 * scaled-fp8 store cancels in the cosine, so none is taken.
 * VF_DTYPE_INT8 rows (one byte per element, two's complement, any of the 256 values) stay one byte per element in
 * HBM as well, and no scale is taken for the same reason: the score of a row is the canonical cosine of its integer
 * values (as fp32) with the query.  The index holds them with the top bit of every byte flipped (code + 128, the
 * form of the int8 row image of fp16 rows), so the rows are always COPIED, by every entry point; no fp16 or fp32
 * copy exists.  Every search path serves them; option scan_image picks the scan: 0 = bytes converted to fp16 in
 * registers (exact), 2 = the int8 matrix instruction on the bytes as they are wherever a shape exists (rows of 768
 * elements, k <= 128), 1 = auto.  Rows of 2560 to 4096 padded elements take the fused path from 32 768 rows (k_scan_ksplit8i: option
 * "wide_rows" below) and the chunked exact path below that count.
 * `id_offset` is added to every returned id (row-sharding across ranks). */
int vf_index_create(vf_index** out, const void* rows, int64_t n, int32_t d, int32_t dtype,
                    int32_t device_id, int64_t id_offset);

/* Same, rows already resident in HBM on `device_id`.  The index BORROWS d_rows (no copy for fp16
 * with d % 128 == 0); the caller keeps it alive until vf_index_destroy.  VF_DTYPE_INT8 rows are the exception:
 * they are copied (re-biased on the way), the index keeps no reference to d_rows and the caller may free it at once. */
int vf_index_create_device(vf_index** out, const void* d_rows, int64_t n, int32_t d, int32_t dtype,
                           int32_t device_id, int64_t id_offset);

/* ---- appending rows to a live index (IndexFlatIP.add, src/utils/faissRetriever.py:18-24; the ingest loop of src/load_data.py:98-128) ----
 * Both entry points above append when `dtype` carries VF_INDEX_APPEND: *out must hold a live handle on entry and holds the same handle
 * on return, whatever the result.  `rows` (host for vf_index_create, device memory of `device_id` for vf_index_create_device) are
 * [n, d] of dtype & 0xFF; d and that dtype must be the handle's, device_id the handle's device (a group's home device); id_offset
 * is ignored.  Row i of the call gets id = the handle's id_offset + its row count before the call + i; n == 0 succeeds and does
 * nothing.  Without the flag nothing changes (dtype 4 and above, 0x100 | 4 too, stay "unknown dtype").
 * Only the new rows are prepared (one kernel over them), so a call costs what its rows cost, whatever the index holds -- except when
 * the row arrays are full (they grow by half, device to device, the old ones freed after the new are complete: option "reserve_rows"
 * avoids it) and when the row count crosses a point at which a fresh build differs (16 384 rows: the scan copy replaces the cache of
 * normalised rows; the int8 row image's threshold).  Afterwards the handle is what vf_index_create over all the rows would have built:
 * same search paths, same kernels, same results.  An index that borrows the caller's device rows takes its own copy on the first
 * append (the caller's memory is never written and may be freed from then on).
 * VF_EINVAL "search pending" while any slot is between _begin and _end; VF_EUNSUPPORTED beyond 2^32-2 rows in a shard; on every
 * failure (VF_ENOMEM, VF_EHIP included) the handle is unchanged and still searchable.  Argument errors are reported before any HIP call.
 * A group handle (vf_index_create_sharded, vf_index_group) puts the rows into its LAST shard, so ids stay one contiguous range and
 * vf_index_shards is unchanged; that shard grows while the others do not, and nothing re-balances them: a group that is mostly
 * appended rows searches at the speed of its last shard.
 * vf_index_set_option(idx, "reserve_rows", total) makes room for `total` rows now (a borrowed index takes its copy now), so that
 * appends up to that count move nothing; a value at or below the row count does nothing, 2^32-1 and above per shard is VF_EUNSUPPORTED. */

/* ---- removing rows from a live index (faiss IndexFlat.remove_ids: later rows shift down, ids stay the positions) ----
 * vf_index_create(&h, ids, n_ids, d, VF_INDEX_REMOVE, device_id, 0): *out holds a live handle on entry and the same handle on return,
 * whatever the result; `rows` is const int64_t ids[n_ids] in HOST memory, global ids (id_offset .. id_offset + n - 1 of the handle);
 * d and device_id must be the handle's (a group's home device); id_offset is ignored.  The flag is honoured only when dtype is
 * VF_INDEX_REMOVE exactly: with any other bit (VF_INDEX_APPEND | VF_INDEX_REMOVE | x included) the value stays "unknown dtype", and
 * vf_index_create_device has no removal form (0x200 is "unknown dtype" there).
 * The listed rows leave and every later row moves down by the number removed before it, so the ids of the handle stay one range and a
 * host list indexed by id stays aligned after the same deletions.  Duplicates in the list count once; n_ids == 0 succeeds and does
 * nothing.  An id outside the handle's range is VF_EINVAL, names the offending position and removes nothing -- strict on purpose: a
 * stale row number after an earlier shift is the classic mistake.  VF_EINVAL "search pending" while any slot is between _begin and
 * _end.  Argument errors (null out, null handle, d or device mismatch, null ids with n_ids > 0, negative n_ids) are reported before
 * any HIP call.
 * Afterwards the handle is what vf_index_create over the remaining rows, in their order, would have built: same search paths, same
 * kernels, same image use, same result bits -- including the transitions a fresh build makes at a row count (at or below 16 384 rows
 * the cache of normalised rows replaces the scan copy; below the int8 row image's threshold the image goes; above it the image is
 * rebuilt, and an index that had refused its image over a row that is gone gets one).  The capacity does not shrink: a later append
 * uses the room.  Nothing below the first removed row is read or written, so a call costs what the rows behind it cost; removing the
 * last rows moves nothing.  The rows move in chunks through a staging buffer of up to 64 MB (option "compact_chunk_rows": destination
 * rows per chunk, 0 = auto).  An index that borrows the caller's device rows takes its own copy first (the caller's memory is never
 * written and may be freed from then on).  A plain handle may lose all its rows; it then behaves like a handle created empty.
 * A group handle removes each id in the shard that holds it, every shard on its own device, and lowers the id_offset of every later
 * shard, so ids stay one contiguous range.  A removal that would leave a shard of a group without rows is VF_EUNSUPPORTED and removes
 * nothing (nothing re-balances a group); all shards are checked before any is changed.
 * Failures: every allocation the call needs (the staging buffer, the owned copy of borrowed rows, a new cache of normalised rows, a
 * new image) is made before the first byte moves, so VF_ENOMEM leaves the handle exactly as it was.  A HIP runtime error AFTER the
 * first move cannot be undone in place: the call returns VF_EHIP and the handle is marked damaged -- every later search, append and
 * removal on it returns VF_EHIP with a message that says so, and so do vf_cosine_matrix_rows / _mixed and the options "reserve_rows"
 * and "scan_image", which read or rebuild the row arrays; vf_index_destroy still works.  The remaining calls (info, stats, the other
 * options) touch no row and answer as before. */

/* ---- ONE handle over several devices (single-process serving) -------------------------------------------------
 * The reference serves from one process (RAGManager singleton, src/utils/ragManager.py:17-30; it builds
 * EnsembleRetriever -> FaissRetriever(embeddings, fn) at src/utils/ensembleRetriever.py:39-43 and searches at :66,:139).
 * vf_index_create_sharded splits the rows into contiguous blocks of ceil(n / n_dev), one per listed
 * device (a device may be listed more than once), and returns a handle every vf_index_* entry point accepts: a search
 * peer-copies the queries from the home device (device_ids[0]) to every shard, runs the shard searches concurrently,
 * peer-copies each packed per-shard top-k back and merges them on the home device -- the result is bit-identical to
 * the single-device one (scores are canonical).  Device-buffer entry points take / return buffers on the HOME device.
 * vf_index_group adopts indexes the caller built itself (e.g. over device-resident shards); they must be contiguous
 * row blocks in ascending order (id_offset of each = id_offset + n of the previous) and the group then owns them. */
int vf_index_create_sharded(vf_index** out, const void* rows, int64_t n, int32_t d, int32_t dtype,
                            const int32_t* device_ids, int32_t n_dev);
int vf_index_create_sharded_from_file(vf_index** out, const char* path, const int32_t* device_ids, int32_t n_dev);
int vf_index_group(vf_index** out, vf_index** shards, int32_t n_shards);
/* number of shards of a handle (0 for a plain single-device index) and their devices (first `cap` of them) */
int vf_index_shards(vf_index* idx, int32_t* n_shards, int32_t* device_ids, int32_t cap);
/* peer (xGMI) access between the home device and every shard's device, as enabled when the group was formed:
 * ok[g] = 1 when both directions are on (or shard g lives on the home device), 0 when a direction could not be enabled
 * and the query / result copies of that shard are staged through the host; *n_missing counts the zeros.  The reference
 * has no counterpart (faiss-CPU index in one process, src/utils/faissRetriever.py:17-19 shows the abandoned GPU try). */
int vf_index_peer_access(vf_index* idx, int32_t* ok, int32_t cap, int32_t* n_missing);

/* Corpus file (.vfc): 64-byte header {char magic[8]="VFCORPUS"; u32 version=1; u32 dtype; u64 n; u32 d; u32 flags;
 * u8 reserved[32]} + n*d row-major elements (+ int64[n] external ids when flags bit 0 is set).  Stands where the
 * reference pulls every embedding out of Chroma into Python lists at start-up (src/utils/ensembleRetriever.py:39-43,
 * src/utils/faissRetriever.py:14): rows [row_lo, row_hi) are streamed from disk through pinned staging straight
 * into HBM (a rank loads only its shard).  veritasfi_amd/corpus_file.py writes the format. */
int vf_corpus_file_info(const char* path, int64_t* n, int32_t* d, int32_t* dtype, int32_t* has_ids);
int vf_index_create_from_file(vf_index** out, const char* path, int64_t row_lo, int64_t row_hi, int32_t device_id,
                              int64_t id_offset);

/* src/utils/faissRetriever.py:34-38 (FaissRetriever.invoke after embed_query): queries [nq,d] fp32,
 * NOT normalised (the library normalises, like faiss.normalize_L2 at :35); out_ids [nq,k] int64,
 * out_scores [nq,k] fp32, best first.  Synchronous; host buffers. */
int vf_index_search(vf_index* idx, const float* queries, int32_t nq, int32_t k, int64_t* out_ids,
                    float* out_scores);

/* Same with device buffers; work is enqueued on `stream` (a hipStream_t, NULL = default stream) and
 * the call returns after the results are final in d_ids / d_scores (it synchronises the stream once,
 * to read the 64-byte certificate word; see DESIGN.md "Exactness certificate"). */
int vf_index_search_device(vf_index* idx, const float* d_queries, int32_t nq, int32_t k,
                           int64_t* d_ids, float* d_scores, void* stream);

/* Pipelined form for throughput: _begin enqueues batch work into slot (0 <= slot < vf_index_slots)
 * and returns immediately; _end waits for that slot, certifies, repairs if needed.  Outputs are valid
 * after _end.  Slots run on internal streams ordered after `stream` at _begin time. */
int vf_index_slots(vf_index* idx, int32_t* out);
int vf_index_search_begin(vf_index* idx, int32_t slot, const float* d_queries, int32_t nq, int32_t k,
                          int64_t* d_ids, float* d_scores, void* stream);
int vf_index_search_end(vf_index* idx, int32_t slot);

/* ---- search a chosen subset of rows: exact filtered top-k ------------------------------------------------------------------
 * The reference promises metadata filtering ("compatible with LangChain that supports metadata filtering": FaissRetriever,
 * BM25Retriever) and does not deliver it: BM25Retriever.invoke(metadata_filters=...) raises NotImplementedError
 * (src/utils/bm25Retriever.py:54,70-72) and the sketch under its TODO (:91-132) ranks everything and masks on the host; in practice
 * it keeps one index per company.  Here ONE index answers "only these rows": `ids` [n_ids] are global ids (id_offset ..
 * id_offset + n - 1), STRICTLY ASCENDING, and the result is what vf_index_search over an index of those rows alone would return, ids
 * mapped back -- same canonical scores bit for bit, descending, ties to the lower id, a zero score reported as +0.0, k > n_ids padded
 * with (-1, -FLT_MAX).  Only the listed rows are read (k_scan_subset scores them as the index holds them: no copy of them is made),
 * so a call costs what its rows cost, whatever the index holds.
 * A list that is out of range, not ascending or repeats an id is VF_EINVAL and the message names the first offending position; the
 * host form checks before any HIP call, the device form by a small kernel whose word is read at the one synchronisation the call
 * makes (nothing has then been written to the output buffers).  A refused call changes nothing: the handle stays searchable.
 * n_ids == 0 returns all padding; n_ids == n is the ordinary search (vf_search_stats.path says which); every other call reports
 * path 3 and subset_rows = n_ids.  Limits: any k while n_ids <= 16 384; k <= 8192 beyond (VF_EUNSUPPORTED, the chunked exact path's own
 * limit); n_ids <= 2^32 - 2.  Synchronous, under the handle's mutex; the workspace is leased from the pool of the small dense entry
 * points (scores: up to 64 MB per launch, option "subset_super_rows" lowers the rows per launch), never from the search slots, so a
 * search pending between _begin and _end is not disturbed.  A damaged handle returns VF_EHIP.
 * Group handles take the host form only (the device form is VF_EUNSUPPORTED): the list is split at the shards' id ranges on the host,
 * the shards are searched one after another -- NOT overlapped -- and the parts are merged on the home device; shards * k > 16384 is
 * VF_EUNSUPPORTED as for every group search.
 * Not in scope: a pipelined _begin / _end form, overlapped shards, MixedModalIndex.  (The BM25 leg has its own row filter, inside its
 * kernels: VF_BM25_FILTER below.)
 * The call (no new entry point: like appends and removals it rides on calls that exist, so the exported surface stays as it is):
 *   vf_subset_query sq = {queries, ids, n_ids};
 *   vf_index_search(idx, (const float*)&sq, nq | VF_SEARCH_SUBSET, k, out_ids, out_scores);                        host buffers
 *   vf_index_search_device(idx, (const float*)&sq, nq | VF_SEARCH_SUBSET, k, d_out_ids, d_out_scores, stream);     device buffers
 * `sq` itself is always in host memory; in the device form its `queries` and `ids` are device pointers on the index's device (a filter
 * uploaded once serves every later call), work is enqueued on `stream` and the call returns after the results are final.  Without
 * the flag nothing about the two calls changes. */
#define VF_SEARCH_SUBSET 0x40000000   /* or'ed into `nq` of vf_index_search / vf_index_search_device: `queries` is a vf_subset_query */
typedef struct vf_subset_query {
    const float* queries;   /* [nq, d] fp32, not normalised */
    const int64_t* ids;     /* [n_ids] global ids, strictly ascending */
    int64_t n_ids;
} vf_subset_query;

/* ---- a list PER QUERY of a batch -----------------------------------------------------------------------------------------------
 * A server that batches the requests of many tenants has one list per query, not one per call.  With VF_SEARCH_SUBSETS row i of the
 * result is, ids and score bits, what the VF_SEARCH_SUBSET call returns for query i alone under lists[list_of[i]]: each query pads with
 * (-1, -FLT_MAX) from its own min(n_ids, k), ties go to the lower id, a zero score is +0.0.  Queries that name the same entry of
 * `lists` share one scan of its rows (four queries per tile); the number of launches does not depend on the number of lists.
 * This mode serves lists of at most 16 384 ids (the lists the one-list form ranks without a merge, at any k); a longer referenced list is
 * VF_EUNSUPPORTED, naming lists[j] and its length -- send its queries through VF_SEARCH_SUBSET.  n_ids[j] == 0 gives padding, n_ids[j] == n
 * is scanned like any list.  list_of[i] outside [0, n_lists) is VF_EINVAL naming the query; a referenced list that is out of range, not
 * ascending or repeats an id is VF_EINVAL naming lists[j], the position and the value (host form: before any HIP call; device form: by
 * one kernel over all referenced lists whose word is read at the call's one synchronisation, nothing having been written to the
 * outputs).  Lists no query names are not read.  A group handle is VF_EUNSUPPORTED in both forms, a damaged handle VF_EHIP, both flags
 * together VF_EINVAL.  Workspace (at most 16 MB of scores per pass of 256 queries) is one lease of the small entry points' pool, under
 * the handle's mutex: a search pending between _begin and _end is not disturbed, and a refused call changes nothing.
 * vf_search_stats: path 4, subset_rows = the sum over the queries of their list's length, subset_tiles.
 *   vf_subsets_query sq = {queries, lists, n_ids, n_lists, list_of};
 *   vf_index_search(idx, (const float*)&sq, nq | VF_SEARCH_SUBSETS, k, out_ids, out_scores);                       host buffers
 *   vf_index_search_device(idx, (const float*)&sq, nq | VF_SEARCH_SUBSETS, k, d_out_ids, d_out_scores, stream);    device buffers
 * `sq`, `lists`, `n_ids` and `list_of` are always host arrays; `queries` and every lists[j] are host pointers in the host form and
 * device pointers on the index's device in the device form. */
#define VF_SEARCH_SUBSETS 0x20000000  /* or'ed into `nq` of vf_index_search / vf_index_search_device: `queries` is a vf_subsets_query */
typedef struct vf_subsets_query {
    const float* queries;            /* [nq, d] fp32, not normalised */
    const int64_t* const* lists;     /* [n_lists] pointers to global ids, each list strictly ascending */
    const int64_t* n_ids;            /* [n_lists] */
    int32_t n_lists;
    const int32_t* list_of;          /* [nq]: each in [0, n_lists) */
} vf_subsets_query;

/* ---- a metadata filter evaluated on the device: range and boolean `where` -----------------------------------------------------------
 * Both filtered searches above start from a row set; this call MAKES one from a filter, on the device, per request.  The caller keeps
 * one int64 KEY COLUMN per metadata field on the index's device (order-preserving keys: an int is its own key, a float its bits
 * folded so that signed compare orders them, a string its rank among the sorted distinct values) with a validity bitmap for rows that
 * lack the field, and compiles the filter into a postfix PROGRAM (veritasfi_amd/where.py does both; csrc/vf_where.h is the program's
 * definition, checker and interpreter):
 *   leaves   kind 0: valid && lo <= key <= hi (lo > hi: passes nothing); kind 1: valid && key is one of the strictly ascending run
 *            set_values[lo .. lo + hi); kind 2: !valid
 *   ops      one byte each: a value below 0x80 pushes that leaf's verdict, 0x80 ands and 0x81 ors the two top values, 0x82 negates the top;
 *            the program leaves exactly one value
 *   limits   64 leaves, 128 ops, stack depth 32, 16 columns, 65 536 set values
 * The call writes d_bitmap -- uint32 words, bit r & 31 of word r >> 5 (VF_BM25_FILTER's layout), 2 * ceil(n / 64) words, zero at and past
 * n -- the number m of passing rows, and, when d_ids is not NULL, their global ids (id_offset + row) in ascending order: exactly the
 * list VF_SEARCH_SUBSET takes, already on the device.  Three launches (evaluate and ballot per 64 rows, prefix over the per-tile counts,
 * ids), one synchronisation, at which m is read.  k, d_ids and d_scores of the call itself are not read.
 * Checked before any device work, VF_EINVAL naming the position: n that is not the handle's row count (columns made before an append or
 * a removal are stale); a program the checker refuses (an op that is no leaf and no operator, a pop from an empty stack, values left
 * over, a leaf of unknown kind or naming no column, a run outside set_values or not strictly ascending); a null d_bitmap; ids_cap < n;
 * a tile_rows that is not 0 or a multiple of 64 in [64, 1024]; the flag together with VF_SEARCH_SUBSET / VF_SEARCH_SUBSETS; count bits
 * in nq; the flag on vf_index_search (the message names the device form).  VF_EUNSUPPORTED: a group handle, or a program over the
 * limits -- evaluate those on the host.  VF_EHIP: a damaged handle.  A refused call writes nothing.  n == 0 returns m = 0 without a
 * launch.  The call runs under the handle's mutex; its descriptor block and tile counts are one lease of the small entry points' pool,
 * so a search pending between _begin and _end is not disturbed; vf_index_stats is left alone.
 *   vf_where_query wq = {n, columns, n_columns, leaves, n_leaves, ops, n_ops, set_values, n_set_values, d_bitmap, d_ids, ids_cap, 0, 0};
 *   vf_index_search_device(idx, (const float*)&wq, VF_SEARCH_WHERE, 0, NULL, NULL, stream);       then wq.m rows pass
 * `wq`, `columns`, `leaves`, `ops` and `set_values` are host memory; the pointers inside `columns`, d_bitmap and d_ids are device
 * pointers on the index's device. */
#define VF_SEARCH_WHERE 0x10000000   /* or'ed into nq of vf_index_search_device: `d_queries` is a vf_where_query; the count bits are 0 */
typedef struct vf_where_column { const int64_t* keys; const uint32_t* valid; } vf_where_column;   /* device; valid NULL = every row has the field */
typedef struct vf_where_leaf { int32_t kind, column; int64_t lo, hi; } vf_where_leaf;
typedef struct vf_where_query {
    int64_t n;                                   /* rows the columns were made for: must equal the handle's row count */
    const vf_where_column* columns; int32_t n_columns;      /* host array of device pointers */
    const vf_where_leaf* leaves;   int32_t n_leaves;        /* host */
    const uint8_t* ops;            int32_t n_ops;           /* host, postfix */
    const int64_t* set_values;     int64_t n_set_values;    /* host */
    uint32_t* d_bitmap;                          /* device out, 2 * ceil(n / 64) words */
    int64_t*  d_ids; int64_t ids_cap;            /* device out, or NULL: ids_cap >= n */
    int64_t   m;                                 /* out: rows passing */
    int32_t   tile_rows;                         /* 0 = 1024; a multiple of 64 in [64, 1024]: tests lower it */
} vf_where_query;

int vf_index_info(vf_index* idx, int64_t* n, int32_t* d, int32_t* dtype, int32_t* device_id);
int vf_index_stats(vf_index* idx, vf_search_stats* out);
/* tuning knobs, by name: every name, its default and its accepted values are the table in veritasfi_amd/csrc/vf_options.h (tests use
 * "force_path" to exercise every path on the same data).  Unknown name or refused value -> VF_EINVAL; vf_last_error says what is accepted.
 * "wide_mfma": matrix instruction of the wide scan (batches of >= 129 queries) over e4m3 rows: -1 auto (= 1; = 0 for rows of 2560
 *   to 4096 padded elements, where the hi + lo query's wider bound costs repairs), 1 the fp8
 *   instruction on the row bytes as stored (k_scan_wide8: the query goes in as a hi + lo pair of e4m3 codes and its exactly
 *   known residual is the query's certificate bound), 0 the fp16 instruction on converted rows (k_scan_wide).  Results are
 *   identical bit for bit; vf_search_stats.scan_kernel says which one ran.
 * "sample_rows": rows per wave the sample pass scores to seed the thresholds: -1 auto (8 for shards of up to 1.5M rows while the
 *   sample still holds 16 k' rows, else 16), or 1..64.  A speed setting: a looser seed admits more candidates, results do not change.
 * "scan_impl": the narrow scan's kernel: 1 k_scan (register loads); 2 (default) k_scan2 (whole-line LDS-DMA loads) for fp16 rows, and
 *   its register-image form k_scan2r where it measured faster (fp16 rows of 384 / 512 / 768 / 1024 elements and e4m3 rows of 768 / 1024, above 1.1M rows); 3 k_scan2
 *   wherever it fits (e4m3 rows converted in registers); 4 k_scan2, never k_scan2r; 5 k_scan2r wherever a shape of it exists, at any
 *   row count.  Same results from each.
 * "sample_impl": the sample pass's kernel: -1 auto (k_scan2r's operand path where it exists and the CU split is on), 0 k_scan, 1 k_scan2r
 *   wherever it fits.  Same sample rows and slots either way; results do not change.
 * "wide_rows": the fused path for rows of 2433 to 4096 elements (padded to 2560 .. 4096: Qwen3-Embedding-4B / -8B,
 *   gte-Qwen2-7B), whose 32-query image does not fit the LDS: k_scan_ksplit splits the contraction over the workgroup's four waves and
 *   keeps the image in registers + LDS (up to 32 queries per pass; batches of 33 or more go to k_scan_wide).  0 never (such an index
 *   takes the chunked exact path at every size, and "force_path" = 1 is refused), 1 auto (default: from 131 072 rows), 2 wherever it
 *   is possible (more than 16 384 rows).  "force_path" = 1 takes the kernel at any of these sizes unless the option is 0.  e4m3 rows of
 *   these widths (padded to a multiple of 128) have a kernel of their own, k_scan_ksplit8 (a row is dp bytes, converted to fp16 in
 *   registers at the matrix instruction; vf_search_stats.scan_kernel = 7): auto from 32 768 rows, up to 64 queries in 32-query passes,
 *   batches of 65 or more on k_scan_wide where the padded width is a multiple of 256.  int8 rows of these widths take the same
 *   kernel with the int8 conversion (k_scan_ksplit8i, scan_kernel = 7 as well; the same batch rules, the wide pass being k_scan_wide's
 *   int8 form) from 32 768 rows, and for them that count is a floor at every setting: below it "wide_rows" = 2 and "force_path" = 1
 *   change nothing (chunked exact path; "force_path" = 1 refused), because 32 768 is the smallest row count at which the byte-row kernel
 *   has been measured and the behaviour of smaller int8 indexes is pinned by tests/test_gpu_int8_rows.py.  Same results bit for bit;
 *   vf_search_stats.scan_kernel = 6 where k_scan_ksplit ran. */
int vf_index_set_option(vf_index* idx, const char* name, int64_t value);
/* Live kernel timing with HIP events on the stream the kernels run on (bench.py roofline):
 * after vf_index_set_option(idx, "profile", 1) every fused search records events around its main
 * k_scan launch and around the whole per-batch pipeline; this returns the accumulated totals
 * (milliseconds, launches) since the option was set.  bytes_per_launch = algorithmic bytes the main
 * k_scan launch reads (rows scanned x (d*2 + 4)). */
int vf_index_profile(vf_index* idx, double* scan_ms_total, int64_t* scan_launches, double* pipeline_ms_total,
                     int64_t* scan_bytes_per_launch);
/* Makespan of the timed main scans since "profile" was set: the first launch's begin to the last launch's end (HIP events
 * on the streams the scans run on) and the number of launches.  Small shards run their scans OVERLAPPED (option
 * overlap_scans, vf_search_stats.scans_overlap): span / launches is then the launch interval the roofline is computed from. */
int vf_index_profile_span(vf_index* idx, double* span_ms, int64_t* launches);
/* Debug aid (not part of the reference surface): wall-clock stamps of the last main scan of `slot`
 * when option "debug" has bit 7 set; returns the number of 64-bit words copied (>= 0) or VF_E*. */
int vf_index_debug_read(vf_index* idx, int32_t slot, unsigned long long* out, int64_t n_words);
int vf_index_destroy(vf_index* idx);

/* ---- small dense cosine ------------------------------------------------------------------------
 * src/utils/ensembleRetriever.py:275-279 (compute_similarity_mtx after the embed loop):
 * x [n,d] fp32 host -> out [n,n] fp32 host, canonical cosine of every row pair. */
int vf_cosine_matrix(const float* x, int32_t n, int32_t d, float* out, int32_t device_id);
/* The same matrix for n rows ALREADY in the index, picked by global id (out [n,n] fp32 host, n <= 4096): what vf_cosine_matrix
 * returns for those rows' values, without re-embedding the chunk texts (ensembleRetriever.py:275 embeds each of the n
 * retrieved chunks again; their embeddings are rows of the HBM-resident corpus).  Valid when the embedder treats documents and
 * queries alike (the reference embeds both with embed_query, :275 and faissRetriever.py:33).  Single-device handles. */
int vf_cosine_matrix_rows(vf_index* idx, const int64_t* ids, int32_t n, float* out);
/* Mixed form: ids[i] >= 0 names a corpus row, ids[i] == -1 takes the NEXT vector of extra [n_extra, d] fp32 host (in order of
 * appearance; the count of -1 entries must equal n_extra) -- a chunk text the corpus does not hold, embedded by the caller.  This is
 * what serves the reference's own call, compute_similarity_mtx(chunk_texts) (src/utils/vllmManager.py:462 ->
 * src/utils/ensembleRetriever.py:265-281: texts only), from the rows in HBM: known texts by row, unknown ones embedded.  An
 * all-extra call returns vf_cosine_matrix's bits, an all-row call vf_cosine_matrix_rows's.  Single-device and sharded handles. */
int vf_cosine_matrix_rows_mixed(vf_index* idx, const int64_t* ids, int32_t n, const float* extra, int32_t n_extra, float* out);

/* experiments/retriever/step3_mul.py:275 (similarities_matrix = cosine_similarity(E, C)):
 * a [na,d], b [nb,d] fp32 host -> out [na,nb] fp32 host. */
int vf_cosine_scores(const float* a, int32_t na, const float* b, int64_t nb, int32_t d, float* out,
                     int32_t device_id);

/* ---- multi-GPU merge: after the RCCL all-gather of per-shard top-k -----------------
 * d_ids_parts / d_score_parts [nparts, nq, k] (global ids, -1 padded) on the current device ->
 * d_ids / d_scores [nq, k].  Asynchronous on `stream`. */
int vf_merge_topk_device(const int64_t* d_ids_parts, const float* d_score_parts, int32_t nparts,
                         int32_t nq, int32_t k, int64_t* d_ids, float* d_scores, int32_t device_id,
                         void* stream);

/* Same, from ONE all-gathered buffer: part g is the blob [ids nq*k int64][scores nq*k fp32][pad] at byte offset
 * g * S, S = nq*k*12 rounded up to a multiple of 16 (so every part's int64 ids stay aligned; a rank packs its result
 * that way so that a batch needs a single collective). */
int vf_merge_topk_packed_device(const void* d_parts, int32_t nparts, int32_t nq, int32_t k, int64_t* d_ids,
                                float* d_scores, int32_t device_id, void* stream);

/* src/utils/vllmManager.py:443-457 (rank_chunk score fusion): scores = rerank + time_score,
 * order = argsort descending (ties lower index first).  Host buffers, n <= 4096. */
int vf_fuse_rank(const float* rerank_scores, const float* time_scores, int32_t n, float* out_scores,
                 int64_t* out_order, int32_t device_id);

/* ---- encoder forward: embedding model and cross-encoder re-ranker -----------------------------
 * Stands where the reference calls third-party model objects:
 *   HuggingFaceEmbeddings(...).embed_query / embed_documents   src/utils/ragManager.py:50,
 *       src/utils/faissRetriever.py:33, src/load_data.py:99,124 (the embed loop)
 *   get_embeddings' model(**inputs) + pooling                   experiments/retriever/step3_mul.py:191-209,
 *       continuous_retrieval.py:127-152
 *   reranker.compute_score(pairs, batch_size=8)                  src/utils/vllmManager.py:450-452
 * BERT-family post-LN encoder (BERT / XLM-R), fp16 weights, fp32 accumulate.  Tokenisation stays in
 * Python (the reference's tokenizers are third-party too); this boundary takes token ids. */
typedef struct vf_encoder vf_encoder;
typedef struct vf_encoder_config {
    int32_t vocab, hidden, layers, heads, ffn, max_pos, type_vocab;
    int32_t roberta_pad_idx; /* -1: BERT positions 0..t-1; >= 0: cumsum(mask)*mask + pad_idx (RoBERTa / XLM-R) */
    int32_t pooling;         /* 0 CLS, 1 unmasked mean (continuous_retrieval.py:148), 2 last token (step3_mul.py:181-188),
                              * 3 masked mean (sentence-transformers pooling_mode_mean_tokens: src/utils/ragManager.py:50's
                              * HuggingFaceEmbeddings on a model whose 1_Pooling/config.json selects it) */
    int32_t normalize;       /* 1: L2-normalise the pooled vector (bge models) */
    int32_t head;            /* 0: embeddings [b, hidden]; 1: RobertaClassificationHead -> one logit per sequence */
    float ln_eps;
} vf_encoder_config;

/* Weight blobs (host), in this order.  fp16: word[vocab,H] pos[max_pos,H] type[type_vocab,H], then per
 * layer Wqkv[3H,H] (q rows, k rows, v rows) Wo[H,H] W1[F,H] W2[H,F], then (head==1) dense[H,H] out_proj[H].
 * fp32: emb_ln_gamma[H] emb_ln_beta[H], then per layer bqkv[3H] bo[H] ln1_gamma[H] ln1_beta[H] b1[F] b2[H]
 * ln2_gamma[H] ln2_beta[H], then (head==1) dense_bias[H] out_proj_bias[1].  nn.Linear layout [out,in]. */
int vf_encoder_weight_sizes(const vf_encoder_config* cfg, int64_t* n_fp16, int64_t* n_fp32);
int vf_encoder_create(vf_encoder** out, const vf_encoder_config* cfg, const void* w_fp16, int64_t n_fp16,
                      const float* w_fp32, int64_t n_fp32, int32_t device_id);
/* ids / mask / type_ids (may be NULL) [b, t] int32 host, t % 32 == 0, t <= 8192 and within the position table (pad with
 * mask 0; up to 512 tokens K / V stay resident in LDS, longer sequences -- bge-m3's 8192 -- stream them);
 * t_valid = columns the tokenizer produced (<= t; the rest is alignment padding the caller added: the
 * unmasked-mean and last-token poolings count only the first t_valid columns);
 * out [b, hidden] (head 0) or [b] (head 1) fp32 host. */
int vf_encoder_forward(vf_encoder* enc, const int32_t* ids, const int32_t* mask, const int32_t* type_ids,
                       int32_t b, int32_t t, int32_t t_valid, float* out);
/* Same, with pooling / normalize chosen for this call (-1 = the handle's setting); embedding handles only.
 * get_embeddings picks the pooling per call site on one loaded model (step3_mul.py:203-207 last token,
 * continuous_retrieval.py:146-149 unmasked mean). */
int vf_encoder_forward_pooled(vf_encoder* enc, const int32_t* ids, const int32_t* mask, const int32_t* type_ids,
                              int32_t b, int32_t t, int32_t t_valid, int32_t pooling, int32_t normalize, float* out);
/* last_hidden_state [b, t, hidden] fp32 host (callers that pool themselves: step3_mul.py:203-207) */
int vf_encoder_forward_hidden(vf_encoder* enc, const int32_t* ids, const int32_t* mask, const int32_t* type_ids,
                              int32_t b, int32_t t, float* out_hidden);
int vf_encoder_info(vf_encoder* enc, vf_encoder_config* out);
int vf_encoder_destroy(vf_encoder* enc);
/* ---- decoder-only models: the embedder / re-ranker family the reference configures by default ----------------
 * Qwen3-Embedding with last_token_pool -- get_embeddings in experiments/retriever/step3_mul.py:181-209 (model :384),
 * continuous_retrieval.py:127-152 -- and "Yes"-logit LLM re-rankers (experiments/profile/stress_test.py:197,212-225:
 * score = logits[:, -1, yes_loc]).  Pre-norm layer: x += Wo attn(rope(qnorm(q)), rope(knorm(k)), v) ; x += Wdown
 * (silu(Wgate n) * Wup n), n = RMSNorm(x); causal grouped-query attention; final RMSNorm.  fp16 weights and GEMM
 * operands; the RESIDUAL STREAM x is fp32 (the reference runs these models in the checkpoint's wider dtype,
 * step3_mul.py:62-64: a residual beyond the fp16 range must not overflow), fp32 accumulation / norms / softmax.
 * head_dim 64, 128 or 256 (gemma), t <= 4096 (the reference's truncation length, step3_mul.py:200). */
typedef struct vf_decoder vf_decoder;
typedef struct vf_decoder_config {
    int32_t vocab, hidden, layers, heads, kv_heads, head_dim, ffn;
    float rope_theta, rms_eps;
    int32_t qk_norm;    /* 1: RMSNorm over head_dim on q and k before RoPE (Qwen3) */
    int32_t pooling;    /* 0 first token, 1 unmasked mean, 2 last token (step3_mul.py:181-188) */
    int32_t normalize;  /* 1: L2-normalise the pooled vector */
    int32_t head;       /* 0: embeddings [b, hidden]; 2: one vocabulary token's logit at the last position -> [b] */
    int32_t act;            /* gated MLP activation: 0 SiLU (Qwen3), 1 tanh-GELU (gemma's gelu_pytorch_tanh) */
    int32_t norm_plus_one;  /* 1: RMSNorm gains are stored zero-centred, y = x_hat * (1 + w) (gemma) */
    float embed_scale;      /* token embeddings are multiplied by this (gemma: sqrt(hidden)); 0 or 1 = none */
} vf_decoder_config;
/* Weight blobs (host).  fp16: embed[vocab,H], then per layer Wqkv[(heads+2*kv_heads)*head_dim, H] (q rows, k rows,
 * v rows) Wo[H, heads*head_dim] Wgate_up[2*ffn, H] (gate rows, up rows) Wdown[H, ffn], then (head == 2) the lm_head
 * row of the scored token [H].  fp32: per layer input_norm[H] post_attention_norm[H] q_norm[head_dim] k_norm[head_dim],
 * then final_norm[H].  nn.Linear layout [out, in]. */
int vf_decoder_weight_sizes(const vf_decoder_config* cfg, int64_t* n_fp16, int64_t* n_fp32);
int vf_decoder_create(vf_decoder** out, const vf_decoder_config* cfg, const void* w_fp16, int64_t n_fp16,
                      const float* w_fp32, int64_t n_fp32, int32_t device_id);
/* ids / mask [b, t] int32 host, t % 32 == 0, t <= 4096 (left- or right-padded, mask 0); positions are column indices
 * (what HF does when no position_ids are passed); out [b, hidden] (head 0) or [b] (head 2) fp32 host. */
int vf_decoder_forward(vf_decoder* dec, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t, int32_t t_valid,
                       float* out);
/* vf_decoder_forward with the L2 normalisation of the pooled row chosen per call (normalize: -1 the handle's, 0, 1; ignored by the
 * token-logit head): HipDecoderEmbeddings -- last_token_pool + F.normalize (experiments/retriever/continuous_retrieval.py:55-60,
 * step3_mul.py:181-209) -- takes unit vectors from the pooling kernel whatever the handle was created with. */
int vf_decoder_forward_pooled(vf_decoder* dec, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t, int32_t t_valid,
                              int32_t normalize, float* out);
/* last_hidden_state [b, t, hidden] fp32 host (after the final RMSNorm), for callers that pool themselves -- the
 * reference's generic route outputs.last_hidden_state -> last_token_pool (experiments/retriever/step3_mul.py:203-207). */
int vf_decoder_forward_hidden(vf_decoder* dec, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t,
                              float* out_hidden);
int vf_decoder_destroy(vf_decoder* dec);

/* re-ranker = encoder with head == 1 */
int vf_reranker_create(vf_encoder** out, const vf_encoder_config* cfg, const void* w_fp16, int64_t n_fp16,
                       const float* w_fp32, int64_t n_fp32, int32_t device_id);
int vf_reranker_score(vf_encoder* rr, const int32_t* ids, const int32_t* mask, const int32_t* type_ids, int32_t b,
                      int32_t t, float* out_scores);
int vf_reranker_destroy(vf_encoder* rr);

/* ---- vision tower (CLIP-style ViT): the "figure encoder" of BASELINE configs[3] -------------------------------------------
 * The reference holds no image model; the contract is transformers' CLIPVisionModelWithProjection (the model family the
 * config names): image_embeds = visual_projection(post_layernorm(last_hidden_state[:, 0])).  Patch embedding without bias,
 * class token, learned positions, pre_layrnorm, PRE-LayerNorm layers, head dim 64 (ViT-B/32, B/16, L/14), at most 511
 * patches per image.  The caller's image processor has already resized and normalised the pixels. */
typedef struct vf_vit vf_vit;
typedef struct vf_vit_config {
    int32_t image, patch, channels; /* 224, 14, 3 */
    int32_t hidden, layers, heads, ffn;
    int32_t proj_dim;               /* width of the joint space (768 for ViT-L/14) */
    int32_t act;                    /* 0 erf-GELU, 1 quick-GELU x * sigmoid(1.702 x) (CLIP's default) */
    int32_t normalize;              /* 1: L2-normalise the projected vector */
    float ln_eps;
} vf_vit_config;
/* Weight blobs (host), in this order.  Kp = channels*patch*patch rounded up to 64.  fp16: patch[H,Kp] (Conv2d weight
 * flattened [H, c*p*p], zero-padded columns) class[H] pos[(P+1),H], then per layer Wqkv[3H,H] (q rows, k rows, v rows)
 * Wo[H,H] W1[F,H] W2[H,F], then proj[proj_dim,H].  fp32: pre_ln_gamma[H] pre_ln_beta[H], then per layer ln1_gamma[H]
 * ln1_beta[H] bqkv[3H] bo[H] ln2_gamma[H] ln2_beta[H] b1[F] b2[H], then post_ln_gamma[H] post_ln_beta[H]. */
int vf_vit_weight_sizes(const vf_vit_config* cfg, int64_t* n_fp16, int64_t* n_fp32);
int vf_vit_create(vf_vit** out, const vf_vit_config* cfg, const void* w_fp16, int64_t n_fp16, const float* w_fp32,
                  int64_t n_fp32, int32_t device_id);
/* pixels [b, channels, image, image] fp32 host -> out [b, proj_dim] fp32 host */
int vf_vit_forward(vf_vit* vit, const float* pixels, int32_t b, float* out);
/* the same on raw bytes: pixels [b, 3, image, image] uint8 host (resized / cropped by the caller), normalised on the device as
 * (x / 255 - mean[c]) / std[c] -- the image processor's rescale + normalize; a quarter of the PCIe bytes */
int vf_vit_forward_u8(vf_vit* vit, const unsigned char* pixels, const float* mean3, const float* std3, int32_t b, float* out);
int vf_vit_destroy(vf_vit* vit);

/* ---- CLIP text tower: the QUERY side of the figure leg (BASELINE configs[3]) ------------------------------------------------
 * Figure rows are CLIP image embeddings (vf_vit_*); a text query can only be compared with them after going through the same
 * model's text tower -- transformers' CLIPTextModelWithProjection: text_embeds = text_projection(final_layer_norm(h)[eos]).
 * Token + learned position embeddings, PRE-LayerNorm layers with CAUSAL attention plus the key-padding mask, head dim 64,
 * at most 512 positions (CLIP: 77).  The reference has no counterpart (its ingest embeds text only, src/load_data.py:98-128);
 * the embedder surface it would be injected through is the one of src/utils/ragManager.py:50 (embed_query / embed_documents). */
typedef struct vf_clip_text vf_clip_text;
typedef struct vf_clip_text_config {
    int32_t vocab, max_pos;         /* 49408, 77 */
    int32_t hidden, layers, heads, ffn; /* ViT-L/14's text tower: 768, 12, 12, 3072 */
    int32_t proj_dim;               /* width of the joint space (768 for ViT-L/14) */
    int32_t act;                    /* 0 erf-GELU, 1 quick-GELU */
    int32_t eos_token_id;           /* 2 (legacy configs of the published checkpoints): pool at argmax(ids); else at the first such id */
    int32_t normalize;              /* 1: L2-normalise the projected vector */
    float ln_eps;
} vf_clip_text_config;
/* Weight blobs (host), in this order.  fp16: token[vocab,H] pos[max_pos,H], then per layer Wqkv[3H,H] (q rows, k rows, v rows)
 * Wo[H,H] W1[F,H] W2[H,F], then proj[proj_dim,H].  fp32: per layer ln1_gamma[H] ln1_beta[H] bqkv[3H] bo[H] ln2_gamma[H]
 * ln2_beta[H] b1[F] b2[H], then final_ln_gamma[H] final_ln_beta[H]. */
int vf_clip_text_weight_sizes(const vf_clip_text_config* cfg, int64_t* n_fp16, int64_t* n_fp32);
int vf_clip_text_create(vf_clip_text** out, const vf_clip_text_config* cfg, const void* w_fp16, int64_t n_fp16, const float* w_fp32,
                        int64_t n_fp32, int32_t device_id);
/* ids [b, t] int32 host, right-padded, t <= max_pos; mask [b, t] (1 = token) or NULL (every position valid: what the HF
 * pipeline passes) -> out [b, proj_dim] fp32 host */
int vf_clip_text_forward(vf_clip_text* ct, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t, float* out);
int vf_clip_text_destroy(vf_clip_text* ct);

/* ---- BM25 leg: replaces bm25s.BM25.retrieve over the index src/utils/bm25Retriever.py:10-20 writes ----------------------------
 * The ensemble's third leg (src/utils/ensembleRetriever.py:188-190) scores every chunk and ranks all of them per request.  The
 * index is bm25s's CSC layout: column c (one per vocabulary token) holds postings indptr[c] .. indptr[c+1]: document rows
 * `indices` (strictly ascending within a column) and their precomputed float32 scores `data` (> 0: Lucene / Robertson-free
 * methods; bm25l / bm25+ are not served).  The arrays are copied to HBM once.
 * Scoring contract: score(doc) = fp32 sum of the doc's postings over the query's token columns, added left to right in query
 * order from 0.0f -- bit-equal to bm25s's numpy scorer (np.add.at per token) on the same token ids.  Ranking: score descending,
 * ties to the LOWER row, over all n_docs rows; untouched rows score 0 and follow the touched ones in ascending row order.
 * Per-query scratch on the device: n_docs * 4 B of scores + n_docs / 8 B of bitmap, up to 64 queries in flight (as many as
 * 3 GiB of it allows); k > 4096 also holds next_pow2(n_docs) * 8 B of sort keys and n_docs * 12 B of results. */
typedef struct vf_bm25 vf_bm25;
/* slots (may be NULL) = queries one device pass serves.  With indptr == NULL the call RELEASES the handle *out instead (all other
 * arguments ignored; *out is set to NULL) -- the exported surface stays two entry points. */
int vf_bm25_create(const int64_t* indptr, int64_t vocab, const int32_t* indices, const float* data, int64_t nnz,
                   int64_t n_docs, int32_t device_id, vf_bm25** out, int32_t* slots);

/* ---- a live BM25 index: documents are added and removed without a rebuild (no new entry point: the update rides on the create) ----
 * A posting's score depends on the document count and the mean document length, so one added or removed document changes every
 * score.  A live handle therefore keeps each posting's term frequency (int32) and each document's length beside the index, and an
 * update rewrites the whole index on the device: removed rows leave, later rows move down (ids stay the positions 0 .. n - 1), new
 * documents get the ids n .. n + m - 1, columns the vocabulary lacks are appended (columns never disappear), and every posting is
 * re-scored by the Lucene recipe in float64, rounded once: (idf*tf) / (tf + k1*((1.0-b) + (b*dl)/avgdl)).  The result is, bit for
 * bit, the index a build over the surviving documents followed by the new ones would be.
 * The call: vf_bm25_create((const int64_t*)&delta, 0, NULL, NULL, 0, 0, device_id | PHASE, &h, &slots), with exactly one PHASE flag.
 * An update is two calls, because idf needs a logarithm and the library takes none: idf[vocab] is the caller's, computed from the
 * counts the first call returns, by the very expression that built the index.
 *   VF_BM25_LIVE     stage: validates the delta (rows in range and strictly ascending per column, tf >= 1; every remove[i] in
 *                    0 .. n - 1 else VF_EINVAL naming i; duplicates count once; at least one document must remain), allocates
 *                    ALL the update needs, and fills counts[vocab] (postings per column after the update) and n_removed.  With
 *                    *out == NULL it starts a live handle from the delta alone; that handle serves nothing until its commit, and a
 *                    failed or discarded creation leaves *out NULL.  A stage discards an earlier stage that was not committed.
 *   VF_BM25_COMMIT   reads idf, avgdl, k1, b: writes the new arrays from the old ones and the delta and swaps them in last.
 *   VF_BM25_DISCARD  drops a staged update (release does too).
 *   VF_BM25_FETCH    copies the handle's arrays to the non-NULL out_* pointers (sized by the caller from the counts it was given).
 * Any failure leaves the handle exactly as it was: an update writes a SECOND set of arrays and never moves anything in place, so
 * between a stage and its commit the device holds the postings twice (12 B per posting each, plus the 4 B per document row map).
 * Searches are unchanged and may run between the two calls (they see the old index); each call holds the handle's lock.  After an
 * update that changes n_docs the per-query scratch is dropped and made again by the next search.  A handle created without
 * VF_BM25_LIVE keeps no term frequencies and refuses these calls; without a flag nothing about vf_bm25_create changes.
 * Only Lucene scoring is live.  `chunk` (0 = 2048, else 1 .. 2048) is the number of postings one workgroup rewrites: tests lower it. */
#define VF_BM25_LIVE 0x1000
#define VF_BM25_COMMIT 0x2000
#define VF_BM25_DISCARD 0x4000
#define VF_BM25_FETCH 0x8000
typedef struct vf_bm25_delta {
    int64_t vocab;            /* V' >= the handle's vocabulary: columns of the delta and of the index after the update */
    int64_t n_new;            /* documents added */
    const int64_t* indptr;    /* [vocab + 1] the new documents' CSC ... */
    const int32_t* rows;      /* ... rows 0 .. n_new - 1, strictly ascending per column */
    const int32_t* tf;        /* ... term frequencies >= 1 */
    const int64_t* remove;    /* [n_remove] ids that leave, any order (host) */
    int64_t n_remove;
    int64_t* counts;          /* out of the stage: [vocab] */
    int64_t n_removed;        /* out of the stage: distinct ids removed */
    const double* idf;        /* commit: [vocab] */
    double avgdl, k1, b;      /* commit: total tokens / n_docs after the update, and the index's parameters */
    int32_t chunk;
    int64_t* out_indptr; int32_t* out_indices; float* out_data; int32_t* out_tf; int32_t* out_doc_len;   /* fetch */
} vf_bm25_delta;
/* q_offsets [nq + 1] (q_offsets[0] = 0, non-decreasing), q_terms [q_offsets[nq]] token columns in query order (repeats count
 * again; a query with no token ranks every row at score 0), 1 <= k <= n_docs (else VF_EINVAL)
 * -> out_ids [nq, k] rows, out_scores [nq, k] (host) */
int vf_bm25_search(vf_bm25* h, const int64_t* q_offsets, const int32_t* q_terms, int32_t nq, int32_t k, int64_t* out_ids,
                   float* out_scores);

/* ---- a BM25 search restricted to a chosen set of rows (no new entry point: the filter rides on the search) -----------------------
 * The call: vf_bm25_filter_query fq = {q_offsets, allow, n_docs};
 *           vf_bm25_search(h, (const int64_t*)&fq, q_terms, nq | VF_BM25_FILTER, k, out_ids, out_scores);
 * `allow` is a bitmap of the rows that may be returned, ONE for all nq queries of the call.  Scores keep the whole corpus's
 * statistics (the postings' scores are what they are): the result is the first k entries of the unfiltered canonical ranking --
 * score descending, ties to the lower row, then the untouched rows at score 0 in ascending row order -- after the rows outside the
 * set are struck out.  Ids are the original rows and score bits those of the unfiltered call.  With m rows allowed and k > m the
 * ranks m .. k - 1 are padding, (-1, -FLT_MAX), as in the dense leg's subset search; k itself stays in [1, n_docs].
 * Checked under the handle's lock before any device work, VF_EINVAL each: a null `allow`; n_docs that is not the handle's document
 * count (a live handle may have changed since the bitmap was made); a bit set at or past n_docs (the message names the first such
 * row).  m == 0 returns all padding without a launch.  A refused call changes nothing.
 * The filter acts at the scatter: a posting whose row is outside the set is neither added nor marked, so the select and the sort see
 * allowed rows only, and the zero-score tail takes allowed untouched rows from every block of the bitmap.  The bitmap, n_docs / 8
 * bytes, is uploaded with every filtered call (no filter is kept on the device between calls); the handle allocates its device copy
 * and 4 B per 32 768 rows and query slot of tail scratch on the first filtered call.  Without the flag nothing about the call changes.
 * (Statistics over the set: VF_BM25_SUBSTATS below; a filter that stays on the device across calls, and a filter per query of a
 * batch: VF_BM25_PREPARED below.) */
#define VF_BM25_FILTER 0x40000000      /* or'ed into `nq` of vf_bm25_search: `q_offsets` is a vf_bm25_filter_query */
typedef struct vf_bm25_filter_query {
    const int64_t*  q_offsets;   /* what q_offsets was */
    const uint32_t* allow;       /* host, (n_docs + 31) / 32 words: bit (r & 31) of word r >> 5 set = row r may be returned */
    int64_t         n_docs;      /* the document count the bitmap was made for */
} vf_bm25_filter_query;

/* ---- a filtered BM25 search scored by the SUBSET's own statistics (no new entry point: the mode rides on the filtered search) --------
 * With VF_BM25_FILTER alone a filtered search keeps the whole corpus's N, df and mean length.  With VF_BM25_SUBSTATS or'ed in as well
 * the result is, bit for bit in ids and score bits, what a handle over the index built from the allowed documents ALONE returns
 * (Lucene scoring, the same vocabulary size, the allowed rows in ascending order, its row i mapped back to the i-th allowed row):
 * N = m, df[c] = the allowed postings of column c, avgdl = the allowed rows' tokens / m (1.0 when they hold none).  Ranking, padding
 * (m < k: ranks m .. k - 1 are (-1, -FLT_MAX)) and the one-filter-per-call rule are the filtered search's.  A query token without an
 * allowed posting adds nothing; a repeated token counts again.
 * A request is TWO calls with the caller's logarithm between them (the library takes none, as for a live update):
 *   vf_bm25_substats_query sq = {q_offsets, allow, n_docs, PHASE, ...};
 *   vf_bm25_search(h, (const int64_t*)&sq, q_terms, nq | VF_BM25_FILTER | VF_BM25_SUBSTATS, k, out_ids, out_scores);
 *   VF_BM25_SUBSTATS_STAGE   counts on the device and fills df [q_offsets[nq]] (one count per q_terms position), total_len (tokens of
 *                            the allowed rows), m (rows allowed) and generation (the handle's update generation).  k, out_ids and
 *                            out_scores are not read (with m == 0 and non-NULL outputs and k >= 1 they are filled with padding).
 *   the caller               idf[t] = log(1.0 + (m - df[t] + 0.5) / (df[t] + 0.5)) in float64, the expression that built the index;
 *                            avgdl = (double)total_len / m, or 1.0 when total_len == 0.
 *   VF_BM25_SUBSTATS_SEARCH  reads idf [q_offsets[nq]], avgdl, k1, b and generation, scores every allowed posting from its term
 *                            frequency -- float64, (idf*tf) / (tf + k1*((1.0-b) + (b*dl)/avgdl)), rounded once, the live update's own
 *                            arithmetic -- and ranks as the filtered search does.
 * Checked under the handle's lock before any device work, on top of the filtered search's checks: the handle must be live (it keeps
 * term frequencies and lengths), else VF_EUNSUPPORTED; a phase that is neither of the two, a null df (stage) or idf (search) with a
 * token in the batch, an idf that is not finite or is negative, avgdl <= 0, k1 < 0 or b outside [0, 1] are VF_EINVAL; so is a
 * generation that is no longer the handle's: the index was updated between the two calls (n_docs alone cannot tell: a removal plus an
 * addition keeps it), and what the stage counted is stale.  A refused call changes nothing, neither the outputs nor the struct.  m == 0
 * returns all padding without a launch.
 * The bitmap goes up once per request: the stage leaves its device copy for the search that follows, which uploads it again only if
 * its `allow` differs from the staged words or another filtered call came between.  The handle allocates 8 B per q_terms position and
 * 8 B per distinct column on the first such call; a handle that never uses the mode allocates nothing.  Without the flag nothing
 * about vf_bm25_search changes.  (Statistics kept on the device across requests, and a filter per query: VF_BM25_PREPARED below.) */
#define VF_BM25_SUBSTATS 0x20000000    /* or'ed into `nq` beside VF_BM25_FILTER: `q_offsets` is a vf_bm25_substats_query */
#define VF_BM25_SUBSTATS_STAGE 1
#define VF_BM25_SUBSTATS_SEARCH 2
typedef struct vf_bm25_substats_query {
    const int64_t*  q_offsets;   /* the three members of vf_bm25_filter_query ... */
    const uint32_t* allow;
    int64_t         n_docs;
    int32_t         phase;       /* ... and, read only under VF_BM25_SUBSTATS: VF_BM25_SUBSTATS_STAGE or VF_BM25_SUBSTATS_SEARCH */
    int64_t*        df;          /* out of the stage: [q_offsets[nq]] allowed postings of each q_terms position's column */
    int64_t         total_len;   /* out of the stage: tokens of the allowed rows */
    int64_t         m;           /* out of the stage: rows allowed */
    uint64_t        generation;  /* out of the stage, into the search: the handle's update generation */
    const double*   idf;         /* search: [q_offsets[nq]] */
    double          avgdl, k1, b;   /* search: the subset's mean length and the index's parameters */
} vf_bm25_substats_query;

/* ---- a PREPARED row filter: the bitmap and the subset's statistics kept on the device across calls (no new entry point) --------------
 * The same filter on thousands of consecutive requests (one index per tenant) need not be packed, checked, uploaded and counted per
 * request: the bitmap, m, the length sum and the subset's df -- hence its idf -- for every column of the vocabulary are properties of
 * (index generation, filter).  A prepared filter computes them once; after that a filtered request is ONE call that uploads nothing but
 * the query, in both statistics modes, and returns bit for bit what the unprepared call with the same rows and mode returns.
 *   vf_bm25_prepared_query pq = {q_offsets, allow, n_docs, PHASE, ...};
 *   vf_bm25_search(h, (const int64_t*)&pq, q_terms, nq | VF_BM25_PREPARED, k, out_ids, out_scores);
 * The handle owns any number of prepared filters, each named by a token the library hands out (never 0, never reused); memory is the
 * only bound.  A filter holds on the device its OWN bitmap (n_docs / 8 bytes, zero past n_docs, padded as the handle's own copy is; it
 * never aliases that copy, and unprepared filtered calls may run between prepared ones), and in subset mode idf [vocab] in float64.
 *   VF_BM25_PREPARED_PREPARE  reads allow, n_docs, mode (VF_BM25_PREPARED_CORPUS or VF_BM25_PREPARED_SUBSET) and chunk, under all of the
 *                             filtered search's checks; uploads the bitmap once; fills token, m, generation and bytes (device bytes the
 *                             filter holds).  Corpus mode computes nothing else.  Subset mode needs a live handle (else
 *                             VF_EUNSUPPORTED) and df [vocab] with vocab = the handle's vocabulary (else VF_EINVAL): it sums the
 *                             allowed rows' lengths and counts df for EVERY column in one pass over the flat posting array
 *                             (k_bm25_sub_df_all), and fills total_len and df.  m == 0 is allowed: such a filter searches to all
 *                             padding without a launch.  `chunk` (0 = 2048, else 1 .. 2048) is the number of postings one workgroup
 *                             of the count takes: tests lower it.  q_terms, nq's count, k and the outputs are not read.
 *   the caller                subset mode: idf[c] = log(1.0 + (m - df[c] + 0.5) / (df[c] + 0.5)) in float64 for every column, the
 *                             expression that built the index; avgdl = (double)total_len / m, or 1.0 when total_len == 0.
 *   VF_BM25_PREPARED_ARM      subset mode only: reads token, idf [vocab] (finite and >= 0, else VF_EINVAL naming the column), avgdl, k1
 *                             and b under VF_BM25_SUBSTATS_SEARCH's checks, and uploads idf to the filter's table.  A filter whose
 *                             generation is no longer the handle's is VF_EINVAL.  A subset-mode filter that was never armed refuses to
 *                             search.
 *   VF_BM25_PREPARED_SEARCH   reads token (or, per query, tokens: below) and q_offsets; q_terms, nq, k and the outputs are the search's
 *                             own.  Corpus mode runs the filtered scatter on the filter's bitmap; subset mode scores each allowed posting from its term frequency
 *                             with idf read per COLUMN from the filter's table.  Everything behind the scatter is the filtered
 *                             search's.  An unknown or released token is VF_EINVAL; so is a filter made before the handle's last
 *                             update (the message says to prepare again).
 *   VF_BM25_PREPARED_RELEASE  frees the filter `token` names.  Releasing the handle frees them all.
 * A committed live update invalidates every prepared filter of the handle and frees its device memory (rows have moved: no filter can
 * search with stale bits); the token stays known, so that a search or an arm with it is refused by its generation, until it is released.
 * An allocation failure is VF_ENOMEM and leaves the handle and every other filter as they were; a refused call changes nothing.
 * A filter PER QUERY of a batch (one index serves many tenants, and a server's batch holds requests of many): a search whose `mode` is
 * VF_BM25_PREPARED_PER_QUERY reads `tokens` [nq] in place of `token`; tokens[i] names the prepared filter of query i, 0 (the library
 * never hands it out) a query without one.  Row i of the result is, ids and score bits, what VF_BM25_PREPARED_SEARCH returns for query i
 * alone with the token tokens[i] -- or, for 0, what the unflagged call returns for it: corpus-mode, subset-mode and unfiltered queries
 * may stand side by side, at every k, with the padding of each query its own (ranks min(m_i, k) .. k - 1).  The call uploads 64 bytes
 * per query beside the query itself and nothing of any filter.  `tokens` is read ONLY in this mode: a caller compiled against the
 * struct without it passes mode 0 or 1 to a search, where `mode` was and is otherwise ignored.  Checked in query order under the
 * handle's lock before any device work, VF_EINVAL each and naming the position and the token: a null `tokens`; a token that is unknown or released;
 * a filter made before the handle's last update; a subset-mode filter that was never armed.  Corpus-mode tokens serve on any handle,
 * subset-mode ones exist only on live handles.  The same token on every query is served as any other batch of this mode.
 * Without the flag nothing about vf_bm25_search changes.  Not in scope: filters remapped across an update, a per-query filter that
 * was not prepared. */
#define VF_BM25_PREPARED 0x10000000    /* or'ed into `nq` of vf_bm25_search: `q_offsets` is a vf_bm25_prepared_query */
#define VF_BM25_PREPARED_PREPARE 1
#define VF_BM25_PREPARED_ARM 2
#define VF_BM25_PREPARED_SEARCH 3
#define VF_BM25_PREPARED_RELEASE 4
#define VF_BM25_PREPARED_CORPUS 0
#define VF_BM25_PREPARED_SUBSET 1
#define VF_BM25_PREPARED_PER_QUERY 2   /* `mode` of a VF_BM25_PREPARED_SEARCH: `tokens` [nq] names a filter per query */
typedef struct vf_bm25_prepared_query {
    const int64_t*  q_offsets;   /* search: what q_offsets was */
    const uint32_t* allow;       /* prepare: host, (n_docs + 31) / 32 words, as vf_bm25_filter_query's */
    int64_t         n_docs;      /* prepare: the document count the bitmap was made for */
    int32_t         phase;       /* one of the four VF_BM25_PREPARED_* phases */
    int32_t         mode;        /* prepare: VF_BM25_PREPARED_CORPUS or VF_BM25_PREPARED_SUBSET; search: VF_BM25_PREPARED_PER_QUERY or anything else */
    uint64_t        token;       /* out of prepare, into arm, search and release */
    int64_t         vocab;       /* prepare (subset mode) and arm: entries of df / idf, the handle's vocabulary */
    int64_t*        df;          /* out of prepare (subset mode): [vocab] allowed postings of every column */
    int64_t         total_len;   /* out of prepare (subset mode): tokens of the allowed rows */
    int64_t         m;           /* out of prepare: rows allowed */
    uint64_t        generation;  /* out of prepare: the handle's update generation */
    int64_t         bytes;       /* out of prepare: device bytes the filter holds */
    const double*   idf;         /* arm: [vocab] */
    double          avgdl, k1, b;   /* arm: the subset's mean length and the index's parameters */
    int32_t         chunk;       /* prepare (subset mode): 0 = 2048, else 1 .. 2048 postings per workgroup of the count */
    const uint64_t* tokens;      /* search in mode VF_BM25_PREPARED_PER_QUERY only: [nq], the filter of each query, 0 = none */
} vf_bm25_prepared_query;

#ifdef __cplusplus
}
#endif
#endif /* VERITASFI_HIP_H */
