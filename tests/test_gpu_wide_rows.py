"""Rows of 2560 to 4096 padded elements on the fused path (k_scan_ksplit, vf_search_stats.scan_kernel == 6; option "wide_rows").

Everything is compared with the CPU oracle (oracle/vf_oracle.c through the `oracle` fixture): ids and score BITS equal.  The
kernel only feeds the approximate scan; the canonical re-score, the certificate and the exact repair are the ones every other
width uses, so a wrong scan shows as a wrong id, as repairs that ordinary data does not need, or as an overflow."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_ranked

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_AUTO = 131_072         # the auto threshold (vf_api.hip: kWideRowsMinRows): from this many rows such an index takes the fused path


@pytest.fixture(scope="module")
def vf():
    import veritasfi_amd as m
    from veritasfi_amd import _ffi
    _ffi.lib()  # raises if the HIP library is missing: no fallback
    n = _ffi.c_i32(0)
    _ffi.check(_ffi.lib().vf_device_count(n), "vf_device_count")
    assert n.value >= 1, "no GPU visible"
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(want, got, what=""):
    (wi, ws), (gi, gs) = want, got
    bad = np.nonzero((wi != gi).any(axis=1))[0]
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:8].tolist()} (first: got {gi[bad[0]][:8]}, want {wi[bad[0]][:8]})"
    assert np.array_equal(_bits(ws), _bits(gs)), f"{what}: score bits differ, max |diff| = {float(np.max(np.abs(ws - gs)))}"
    for q in range(gi.shape[0]):
        assert_ranked(gi[q], gs[q])


def _data(seed, n, d, nq, dtype):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n, d)).astype(np.float32)
    if dtype == np.float16:
        c = c.astype(np.float16)
    q = np.random.default_rng(seed + 1).standard_normal((nq, d)).astype(np.float32)
    return c, q


NQS = (1, 3, 32, 33, 64, 65, 130)
KS = (1, 100, 2048)


# ---- 1 + 2: every width, both row types, every batch size and depth; the same bytes with the kernel switched off ----------------
@pytest.mark.parametrize("d", [2560, 3072, 4096, 2500, 3000])
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_wide_rows_search_on_the_fused_path_bit_equal_to_the_oracle(vf, oracle, d, dtype):
    c, q = _data(1000 + d, N_AUTO, d, max(NQS), dtype)
    full = oracle.search(c, q, max(KS))                    # (ranked by a total order: the best k of it are the result for k)
    want = {k: (np.ascontiguousarray(full[0][:, :k]), np.ascontiguousarray(full[1][:, :k])) for k in KS}
    with vf.DenseIndex(c) as ix:
        for k in KS:
            for nq in NQS:
                ids, sc = ix.search(q[:nq], k)
                st = ix.stats()
                print(f"d={d} {np.dtype(dtype).name} nq={nq} k={k}: path={st['path']} kernel={st['scan_kernel']} candidates={st['candidates']} "
                      f"max={st['max_candidates']} overflowed={st['overflowed']} uncertified={st['uncertified']} reruns={st['exact_reruns']}")
                _same((want[k][0][:nq], want[k][1][:nq]), (ids, sc), f"d={d} nq={nq} k={k}")
                assert st["path"] == 1, st
                # both sides of the dispatch boundary (vf_api.hip: kWideMinQueriesKsplit = 33): up to 32 queries k_scan_ksplit, from 33 k_scan_wide
                assert st["scan_kernel"] == (6 if nq <= 32 else 3), st
                assert st["overflowed"] == 0 and st["exact_reruns"] == 0, st
        # the same searches with the kernel switched off: path 2, the same bytes
        ix.set_option("wide_rows", 0)
        for k, nq in ((100, 3), (2048, 33), (1, 130)):
            ids, sc = ix.search(q[:nq], k)
            assert ix.stats()["path"] == 2
            _same((want[k][0][:nq], want[k][1][:nq]), (ids, sc), f"wide_rows=0 d={d} nq={nq} k={k}")
        with pytest.raises(Exception):                        # forcing the fused path with the kernel switched off is refused, as before
            ix.set_option("force_path", 1)
            ix.search(q[:2], 10)
        ix.set_option("force_path", -1)
        ix.set_option("wide_rows", 1)


def test_wide_rows_option_two_serves_a_small_corpus_and_auto_leaves_it_alone(vf, oracle):
    c, q = _data(32, 20_000, 2560, 30, np.float16)
    want = oracle.search(c, q, 50)
    with vf.DenseIndex(c) as ix:
        ids, sc = ix.search(q, 50)                            # auto: below the threshold, the chunked exact path as before
        assert ix.stats()["path"] == 2
        _same(want, (ids, sc), "auto, 20 000 rows")
        ix.set_option("wide_rows", 2)
        ids, sc = ix.search(q, 50)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_kernel"] == 6 and st["overflowed"] == 0, st
        _same(want, (ids, sc), "wide_rows = 2, 20 000 rows")
        ix.set_option("wide_rows", 1)
        ix.set_option("force_path", 1)                        # forced: the new kernel instead of "unsupported"
        ids, sc = ix.search(q[:4], 50)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_kernel"] == 6, st
        _same((want[0][:4], want[1][:4]), (ids, sc), "force_path = 1")
        with pytest.raises(Exception):
            ix.set_option("wide_rows", 3)


# ---- 3: the shape the existing suite documents stays on path 2 -------------------------------------------------------------------
def test_auto_keeps_17000_rows_of_2560_on_the_chunked_path(vf, oracle):
    c, q = _data(32, 17_000, 2560, 3, np.float16)
    with vf.DenseIndex(c) as ix:
        ids, sc = ix.search(q, 10)
        assert ix.stats()["path"] == 2
    _same(oracle.search(c, q, 10), (ids, sc))


# ---- 4a: the certificate-defeating construction of tests/adversarial.py, re-derived for d = 2560 --------------------------------
def halfway_query_2560(off=3e-5, seed=0):
    """Unit-norm query of 2560 entries beside fp16 half-way points: 1 / sqrt(2560) = 2^-6 * 1.2649, so the entries are
    2^-6 (1 + (2 m + 1) 2^-11) (1 -+ off) with m in {270, 271} (mantissas 1.26416 and 1.26514, squares 1.59810 and 1.60057) mixed so
    that the mean squared mantissa is 4096 / 2560 = 1.6; even entries sit just below their half-way point (round down), odd ones above."""
    d = 2560
    rng = np.random.default_rng(seed)
    mu = {m: 1.0 + (2 * m + 1) * 2.0 ** -11 for m in (270, 271)}
    frac = (4096.0 / d - mu[270] ** 2) / (mu[271] ** 2 - mu[270] ** 2)
    assert 0.0 < frac < 1.0
    n271 = int(round(frac * d))
    m = np.array([271] * n271 + [270] * (d - n271))
    rng.shuffle(m)
    sign = np.where(np.arange(d) % 2 == 0, -1.0, 1.0)
    t = 2.0 ** -6 * (1.0 + (2 * m + 1) * 2.0 ** -11) * (1.0 + sign * off)
    return (t * rng.choice([-1.0, 1.0], size=d)).astype(np.float32)


def build_hostile_case_2560(oracle, k=100, kprime=160, rho=0.2, n_background=40_000, seed=1):
    """tests/adversarial.py's build_case for d = 2560: one victim row whose approximate score understates its canonical score by
    ||delta|| sqrt(1 - rho^2) ~ 3.8e-4, k strong rows with canonical scores just below the victim's, fillers whose approximate scores
    sit just above the victim's.  The victim is the true best match and is outside the approximate top-k'."""
    from adversarial import approx_scores
    d = 2560
    rng = np.random.default_rng(seed)
    q = halfway_query_2560()
    qn = oracle.normalize(q[None, :])[0]
    delta = qn.astype(np.float16).astype(np.float64) - qn.astype(np.float64)
    assert np.linalg.norm(delta) > 3.0e-4, np.linalg.norm(delta)       # the entries do sit beside half-way points: ~2^-11 / sqrt(... )
    qd = qn.astype(np.float64)
    qd /= np.linalg.norm(qd)
    dh = delta - (delta @ qd) * qd
    dh /= np.linalg.norm(dh)

    def make(rho_t, alpha, count):
        z = rng.standard_normal((count, d))
        z -= np.outer(z @ qd, qd)
        z -= np.outer(z @ dh, dh)
        z /= np.linalg.norm(z, axis=1, keepdims=True)
        rho_t = np.broadcast_to(np.asarray(rho_t, dtype=np.float64), (count,))
        s = np.sqrt(1.0 - rho_t ** 2)
        v = rho_t[:, None] * qd + s[:, None] * (alpha * dh + np.sqrt(1.0 - alpha ** 2) * z)
        return v.astype(np.float16)

    victim = make(rho, -1.0, 1)
    can_v = float(oracle.cosine(q[None, :], victim.astype(np.float32))[0, 0])
    app_v = float(approx_scores(qn, victim)[0])
    assert can_v - app_v > 2.5e-4, (can_v, app_v)
    lo_s, hi_s = app_v + 6e-5, can_v - 4e-6                              # strong rows: canonical below the victim's, approximate well above its
    cand = make(rng.uniform(lo_s - 1e-5, hi_s + 1e-5, 3000), 0.0, 3000)
    can_c = oracle.cosine(q[None, :], cand.astype(np.float32))[0]
    app_c = approx_scores(qn, cand)
    ok = (can_c > lo_s) & (can_c < hi_s) & (np.abs(app_c - can_c) < 2e-5)
    strong = cand[ok][:k]
    assert strong.shape[0] == k, f"only {int(ok.sum())} strong rows met the window"
    fill = make(rng.uniform(app_v + 2e-6, app_v + 2.4e-5, 2500), 0.0, 2500)
    app_f = approx_scores(qn, fill)
    okf = (app_f > app_v + 6e-6) & (app_f < app_v + 1.6e-5)
    filler = fill[okf][: (kprime - k) + 12]
    assert filler.shape[0] >= kprime - k + 4, f"only {int(okf.sum())} fillers met the window"
    background = rng.standard_normal((n_background, d)).astype(np.float16)
    rows = np.concatenate([background, filler, strong, victim])
    perm = rng.permutation(rows.shape[0])
    rows = np.ascontiguousarray(rows[perm])
    victim_id = int(np.nonzero(perm == rows.shape[0] - 1)[0][0])
    app = approx_scores(qn, rows)
    can = oracle.cosine(q[None, :], rows.astype(np.float32))[0]
    by_app = np.argsort(-app, kind="stable")[:kprime]
    return {"corpus": rows, "query": q[None, :].copy(), "victim": victim_id, "victim_rescored": bool(victim_id in by_app),
            "true_best": int(np.argmax(can)), "victim_canonical": can_v, "victim_approx": app_v}


def test_hostile_query_beside_fp16_halfway_points_at_2560(vf, oracle):
    case = build_hostile_case_2560(oracle)
    assert case["true_best"] == case["victim"] and not case["victim_rescored"], case   # checked on the CPU: the scan alone would lose it
    c = case["corpus"]
    rng = np.random.default_rng(5)
    q = np.concatenate([case["query"], rng.standard_normal((4, 2560)).astype(np.float32), case["query"] * 3.0])
    want = oracle.search(c, q, 100)
    assert want[0][0, 0] == case["victim"]
    with vf.DenseIndex(c) as ix:
        ix.set_option("wide_rows", 2)                     # (40 173 rows: below the auto threshold)
        for nq in (1, 6):
            ids, sc = ix.search(q[:nq], 100)
            st = ix.stats()
            print("hostile 2560:", {x: st[x] for x in ("path", "scan_kernel", "uncertified", "overflowed", "exact_reruns")})
            assert st["path"] == 1 and st["scan_kernel"] == 6, st
            _same((want[0][:nq], want[1][:nq]), (ids, sc), f"hostile nq={nq}")
            assert ids[0, 0] == case["victim"]


# ---- 4b: the data kinds of tools/fuzz_search.py at d = 2560 ---------------------------------------------------------------------
@pytest.mark.parametrize("data,dtype", [("dupes", "f16"), ("clusters", "f16"), ("zeros", "f16"), ("lowrank", "f16"), ("sorted", "f16"),
                                        ("scaled", "f32"), ("ties", "f16")])
def test_hostile_data_kinds_at_2560_are_exact(vf, oracle, data, dtype):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_search
    n, d, nq, k = 36_000, 2560, 32, 64
    if data == "ties":                                    # exact ties: blocks of identical rows (ranked by id), a few distinct ones
        rng = np.random.default_rng(77)
        base = rng.standard_normal((9, d)).astype(np.float16)
        rows = base[rng.integers(0, 9, n)]
        rows[::1000] = rng.standard_normal((len(rows[::1000]), d)).astype(np.float16)
        q = rng.standard_normal((nq, d)).astype(np.float32)
        q[0] = base[3].astype(np.float32)
    else:
        case = dict(dtype=dtype, d=d, nq=nq, n=n, k=k, data=data, seed=4242)
        _, rows, q = fuzz_search.make_data(case)
        if data == "sorted":                              # ascending scores for query 0: its threshold rises all the way through the scan
            order = np.argsort(oracle.cosine(q[:1], rows.astype(np.float32))[0], kind="stable")
            rows = np.ascontiguousarray(rows[order])
    want = oracle.search(rows, q, k)
    with vf.DenseIndex(rows) as ix:
        ix.set_option("wide_rows", 2)                     # (36 000 rows: below the auto threshold)
        ids, sc = ix.search(q, k)
        st = ix.stats()
    print(f"{data}: ", {x: st[x] for x in ("path", "scan_kernel", "candidates", "max_candidates", "uncertified", "overflowed", "exact_reruns")})
    assert st["path"] == 1 and st["scan_kernel"] == 6, st
    _same(want, (ids, sc), data)


# ---- 5: the handle kinds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_handles_on_one_device(vf, oracle, shards):
    c, q = _data(50 + shards, 70_001, 2560, 29, np.float16)
    want = oracle.search(c, q, 100)
    with vf.DenseIndex(c, device_ids=[0] * shards) as ix:
        ix.set_option("wide_rows", 2)                     # (three shards of 23 333 rows are below the auto threshold)
        ids, sc = ix.search(q, 100)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_kernel"] == 6 and st["overflowed"] == 0, st
        _same(want, (ids, sc), f"{shards} shards")


def test_the_reference_deep_call_k_2048_with_one_to_four_queries(vf, oracle):
    c, q = _data(60, 140_000, 2560, 4, np.float32)
    want = oracle.search(c, q, 2048)
    with vf.DenseIndex(c) as ix:
        for nq in (1, 2, 4):
            ids, sc = ix.search(q[:nq], 2048)
            st = ix.stats()
            print(f"deep call nq={nq}:", {x: st[x] for x in ("path", "scan_kernel", "candidates", "max_candidates", "uncertified", "overflowed", "exact_reruns")})
            assert st["path"] == 1 and st["scan_kernel"] == 6 and st["overflowed"] == 0 and st["exact_reruns"] == 0, st
            _same((want[0][:nq], want[1][:nq]), (ids, sc), f"deep nq={nq}")


def test_begin_end_over_all_slots_file_index_and_borrowed_rows(vf, oracle, tmp_path):
    import torch
    from veritasfi_amd import corpus_file
    c, q = _data(70, 40_000, 3072, 48, np.float16)
    k = 20
    want = oracle.search(c, q, k)
    path = str(tmp_path / "wide.vfc")
    corpus_file.write(path, c)
    rows_dev = torch.from_numpy(c).cuda()
    for name, ix in (("host rows", vf.DenseIndex(c)), (".vfc file", vf.DenseIndex.from_file(path)), ("borrowed device rows", vf.DenseIndex(rows_dev))):
        with ix:
            ix.set_option("wide_rows", 2)                 # (40 000 rows: below the auto threshold)
            nslots = ix.slots
            assert nslots >= 2
            parts = np.array_split(np.arange(q.shape[0]), nslots)
            qd = [torch.from_numpy(q[p]).cuda() for p in parts]
            for rep in range(2):                          # every slot in flight at once, twice (buffers reused)
                outs = [ix.search_begin(s, qd[s], k) for s in range(nslots)]
                for s in range(nslots):
                    ix.search_end(s)
                    st = ix.stats()
                    assert st["path"] == 1 and st["scan_kernel"] == 6, (name, st)
                torch.cuda.synchronize()
                for s, p in enumerate(parts):
                    _same((want[0][p], want[1][p]), (outs[s][0].cpu().numpy(), outs[s][1].cpu().numpy()), f"{name}, slot {s}")


# ---- 6: one size that matters -------------------------------------------------------------------------------------------------------
def test_one_million_rows_of_2560_whole_corpus_oracle_check(vf, oracle):
    n, d, nq, k = 1_000_000, 2560, 64, 100
    rng = np.random.default_rng(2560)
    c = np.empty((n, d), np.float16)
    for lo in range(0, n, 50_000):                        # (in blocks: the fp32 draw of the whole corpus would be 10 GB)
        c[lo:lo + 50_000] = rng.standard_normal((50_000, d), dtype=np.float32).astype(np.float16)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        ids, sc = ix.search(q, k)                         # 64 queries: k_scan_wide
        st = ix.stats()
        ids32, sc32 = ix.search(q[:32], k)                # 32 queries: k_scan_ksplit
        st32 = ix.stats()
    for tag, s_ in (("64 queries", st), ("32 queries", st32)):
        print(f"1M x 2560, {tag}:", {x: s_[x] for x in ("path", "scan_kernel", "candidates", "max_candidates", "uncertified", "overflowed", "exact_reruns")})
    assert st["path"] == 1 and st["scan_kernel"] == 3 and st["overflowed"] == 0 and st["exact_reruns"] == 0, st
    assert st32["path"] == 1 and st32["scan_kernel"] == 6 and st32["overflowed"] == 0 and st32["exact_reruns"] == 0, st32
    want = oracle.search(c, q, k)
    _same(want, (ids, sc), "1M x 2560, 64 queries")
    _same((want[0][:32], want[1][:32]), (ids32, sc32), "1M x 2560, 32 queries")


# ---- 7: the same case forty times -----------------------------------------------------------------------------------------------------
def test_forty_repeats_are_bit_equal(vf, oracle):
    c, q = _data(90, 50_000, 4096, 32, np.float16)
    want = oracle.search(c, q, 100)
    with vf.DenseIndex(c) as ix:
        ix.set_option("wide_rows", 2)                     # (50 000 rows: below the auto threshold)
        first = None
        for rep in range(40):
            ids, sc = ix.search(q, 100)
            st = ix.stats()
            assert st["path"] == 1 and st["scan_kernel"] == 6, st
            if first is None:
                _same(want, (ids, sc), "repeat 0")
                first = (ids.copy(), _bits(sc).copy())
            else:
                assert np.array_equal(ids, first[0]) and np.array_equal(_bits(sc), first[1]), f"run {rep} differs from run 0"


# ---- the Python surface: a decoder embedder of hidden size 2560 feeding FaissRetriever.invoke ----------------------------------------
class _WordHashTokenizer:
    """Word-hash tokenizer with the HF methods HipDecoderEmbeddings calls (left padding, as decoder embedders use)."""
    bos_token_id, pad_token_id, padding_side = 2, 0, "left"

    def __call__(self, text, return_tensors=None, add_special_tokens=False, max_length=None, truncation=False, **_):
        ids = [5 + (sum(map(ord, w)) * 31 + len(w)) % 780 for w in text.split(" ") if w != ""]
        if truncation and max_length is not None:
            ids = ids[:max_length]
        return {"input_ids": ids}

    def pad(self, inputs, padding=True, max_length=None, pad_to_multiple_of=None, return_tensors=None):
        width = max(len(x["input_ids"]) for x in inputs)
        if pad_to_multiple_of:
            width = -(-width // pad_to_multiple_of) * pad_to_multiple_of
        ids = np.full((len(inputs), width), self.pad_token_id, np.int64)
        mask = np.zeros((len(inputs), width), np.int64)
        for i, x in enumerate(inputs):
            n = len(x["input_ids"])
            ids[i, width - n:], mask[i, width - n:] = x["input_ids"], 1
        return {"input_ids": ids, "attention_mask": mask}


def test_decoder_embedder_of_hidden_size_2560_through_faiss_retriever_invoke(vf, oracle, tmp_path):
    import torch
    from transformers import Qwen3Config, Qwen3Model
    torch.manual_seed(11)
    cfg = Qwen3Config(vocab_size=800, hidden_size=2560, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=32,
                      num_key_value_heads=8, head_dim=128, max_position_embeddings=512, rope_theta=1000000.0, tie_word_embeddings=False)
    model = Qwen3Model(cfg).eval()
    with torch.no_grad():
        for p_ in model.parameters():
            p_.copy_(p_.half().float())
    emb = vf.HipDecoderEmbeddings(_WordHashTokenizer(), vf.HipDecoder.from_hf(model, pooling=2, normalize=True), max_length=32, batch_size=128,
                                  query_instruction="query: ")
    words = ("revenue margin segment filing quarter fiscal cash flow guidance deliveries table figure europe asia energy storage "
             "automotive services debt equity dividend").split()
    rng = np.random.default_rng(3)
    docs = [" ".join(rng.choice(words, size=int(rng.integers(6, 14))).tolist()) + f" item {i}" for i in range(16_500)]
    # the project's own corpus route (load_data.py's embed loop -> corpus file -> index): fp16 rows, 128 texts per forward
    from veritasfi_amd import corpus_file
    path = str(tmp_path / "qwen2560.vfc")
    assert corpus_file.embed_to_file(path, docs, emb, batch_size=1100) == len(docs)
    vecs = np.asarray(corpus_file.rows_memmap(path))
    assert vecs.shape == (16_500, 2560) and vecs.dtype == np.float16 and np.isfinite(vecs.astype(np.float32)).all()
    fr = vf.FaissRetriever.from_index(vf.DenseIndex.from_file(path), emb, rows_as_given=False)
    fr.index.set_option("wide_rows", 2)                   # 16 500 rows: below the auto threshold
    queries = [docs[7], docs[9000], "cash flow of the energy storage segment"]
    I, D = fr.invoke(queries, 10)
    st = fr.index.stats()
    print("decoder 2560 -> FaissRetriever:", {x: st[x] for x in ("path", "scan_kernel", "uncertified", "overflowed", "exact_reruns")})
    assert st["path"] == 1 and st["scan_kernel"] == 6, st
    qv = np.asarray(emb.embed_queries(queries), np.float32)
    _same(oracle.search(vecs, qv, 10), (I, D), "FaissRetriever.invoke")
    fr.index.close()
    emb.decoder.close()
