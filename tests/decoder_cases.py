"""Inputs and plain NumPy float64 references for the decoder's kernels, one kernel at a time: the causal grouped-query attention
(k_attention_stream2<DH, true>), k_rope_table, k_qknorm_rope, k_rmsnorm, k_swiglu, k_gather_rows, k_token_logit and the last-token
branch of k_pool.  NumPy only: nothing here touches a GPU.  tests/test_decoder_cases_host.py checks the references against
transformers on the CPU and every planted case against its own conditions; tests/test_gpu_decoder_kernels.py runs the kernels.

Attention cases come in two families.

PEAKED-RANDOM: q, k, v ~ N(0, 1) rounded to fp16, q times a sharpness in {1, 3, 6}.  The reference is the float64 softmax; the bound
of a case is twice the error that ``attention_model_fp16`` (the kernel's roundings, in NumPy) has against float64 on that same case
(``MODEL_ERR``, computed on the CPU, never from a kernel's output).

PLANTED: every valid query i has ONE target key j(i) <= i that outscores every other key it may see by >= 25 nats (softmax weight
>= 1 - 1e-6), so the float64 output is V[j(i)]; and every key it must NOT see -- i + 1, the first key of the next key tile, any
padded key -- outscores the target by >= 25 nats, so one wrongly admitted key replaces the output by another row of V.  (Random
+-1 codes cannot hold a 25-nat margin at head dim 64: the cross-correlation of 32-element codes over thousands of keys reaches the
target's own score.  This construction is exact instead.)  The score of query i on key j, in nats:

    S(i, j) = 80 * chunk(j)  +  f_i(j mod 32)  +  bonus_i * [j in the class that query i selected]          chunk(j) = j // 32

  * f_i is -40 everywhere except: 0 at the target's slot when the target sits in the query's own 32-key chunk, +40 at slot
    (i mod 32) + 1 (key i + 1: the bait behind the diagonal).  32 one-hot dims carry it.
  * a target in an EARLIER chunk is reached through a class flag (first valid key, first key of a key tile, last key of a key tile,
    last key of a 32-key chunk) with bonus_i = 80 * (chunk(i) - chunk(j(i))) - f_i(slot of j(i)): the target then scores exactly
    80 * chunk(i), earlier members of the class 80 per chunk less, and a query only selects a class whose LATEST visible member is
    its target.
  * every later key scores >= 80 * (chunk(i) + 1) - 40, and a padded key carries chunk 128 and nothing else: both beat the target by
    >= 40 nats if admitted.  Scores stay below 10300 nats, far inside the kernel's additive -30000 mask.
  * targets cycle with (i + head) mod 5 through: the diagonal, the first valid key (key 0 of an unpadded row), i - 1, the last key
    of the previous key tile, the first key of the current key tile; a target that is padded falls back to the diagonal.
  * K is the same pattern for every kv head but rotated by 3 dims per kv head (q likewise), V is distinct per kv head: a wrong
    head-to-kv-head mapping lands on other scores and another row.
The key tile is 128 / 64 / 32 keys at head dim 64 / 128 / 256.
"""
import zlib

import numpy as np

KEY_TILE = {64: 128, 128: 64, 256: 32}             # AttnStream2Lds<DH>::KT
QK_TOKENS_PER_WG = {64: 64, 128: 32, 256: 16}      # k_qknorm_rope: 256 / (dh / 16)
MASKED = np.float32(-30000.0)
LOG2E = np.float32(1.4426950408889634)
PLANT_CHUNK, PLANT_U = 80.0, 40.0                  # nats per 32-key chunk; the slot bonus / penalty
PLANT_DIMS = 37                                    # 32 slots, chunk, four class flags
_CLS_FIRST, _CLS_TILE_START, _CLS_TILE_END, _CLS_CHUNK_END = 33, 34, 35, 36
_FLAG = 16.0                                       # a class flag's value in K (keeps the query's side inside fp16)


def row_mask(T, pad):
    """One row's key padding mask.  pad: 'none', 'right', 'left70', 'left_all' (a single valid key), 'hole', 'hole_late' or ('valid', n)."""
    m = np.ones(T, np.int32)
    if pad == "right":
        m[max(1, T - T // 3 - 5):] = 0
    elif pad == "left70":
        m[:min(70, T - 1)] = 0
    elif pad == "left_all":
        m[:T - 1] = 0
    elif pad == "hole":                      # interior holes over the 32- and 64-key boundaries, and over key 128
        m[30:min(70, T - 1)] = 0
        if T >= 160:
            m[120:135] = 0
    elif pad == "hole_late":                 # pads in the SECOND half of a 128-key tile only (head dim 64: the second staging wave's flag)
        assert T >= 288
        m[200:230] = 0
    elif isinstance(pad, tuple):
        m[pad[1]:] = 0
    else:
        assert pad == "none", pad
    return m


# ---- the case list ---------------------------------------------------------------------------------------------------------------
# (name, family, T, (heads, kv_heads), rows: pad kind per batch row | packed: valid length per sequence, sharpness)
# T 32: one active wave; 96: a partial key tile; 160: a second query block with one active wave; 288: three query blocks and the
# per-wave tile skip; 1024: many tiles through both LDS buffers; 4096 once.  'left70' at head dim 256: two fully masked tiles, then
# a partly masked one.  Packed: each sequence keeps ceil32(length) rows, valid tokens first.
ATTENTION_CASES = [
    ("planted-32", "planted", 32, (4, 1), ("none", "right", "left_all", "hole"), None),
    ("planted-96", "planted", 96, (4, 2), ("none", "right", "left70", "left_all", "hole"), None),
    ("planted-160", "planted", 160, (6, 3), ("none", "right", "left70", "left_all", "hole"), None),
    ("planted-288", "planted", 288, (2, 2), ("none", "right", "left70", "left_all", "hole"), None),
    ("planted-288-gqa", "planted", 288, (4, 2), ("none", "hole", "left70", "hole_late"), None),
    ("planted-1024", "planted", 1024, (4, 1), ("none", "left70", "hole", "hole_late"), None),
    ("planted-packed", "planted", 288, (4, 2), ("packed", 32, 96, 160, 288), None),
    ("planted-packed-longest-last", "planted", 288, (6, 3), ("packed", 70, 17, 288, 130), None),
    ("planted-4096", "planted", 4096, (2, 1), ("none",), None),
    ("random-32-s6", "random", 32, (4, 1), ("none", "right", "left_all", "hole"), 6.0),
    ("random-96-s3", "random", 96, (6, 3), ("none", "right", "left70", "left_all", "hole"), 3.0),
    ("random-160-s6", "random", 160, (4, 2), ("none", "right", "left70", "hole"), 6.0),
    ("random-288-s1", "random", 288, (4, 2), ("none", "right", "left70", "left_all", "hole"), 1.0),
    ("random-288-s3", "random", 288, (2, 2), ("none", "left70"), 3.0),
    ("random-288-s6", "random", 288, (4, 1), ("none", "hole", "hole_late"), 6.0),
    ("random-1024-s3", "random", 1024, (2, 2), ("none", "left70"), 3.0),
    ("random-packed-s1", "random", 288, (4, 2), ("packed", 32, 96, 160, 288), 1.0),
    ("random-packed-longest-last-s3", "random", 288, (6, 3), ("packed", 70, 17, 288, 130), 3.0),
]
HEAD_DIMS = (64, 128, 256)

# max |attention_model_fp16 - float64| over the valid query rows of each peaked-random case, in units of max |v|, computed on the
# CPU by tests/test_decoder_cases_host.py::test_fp16_model_error_is_the_recorded_one (which prints and re-checks them).  The GPU
# test's bound for a case is TWICE its entry.
MODEL_ERR = {
    "random-32-s6-dh64": 2.797e-04,
    "random-32-s6-dh128": 9.240e-04,
    "random-32-s6-dh256": 2.430e-04,
    "random-96-s3-dh64": 2.787e-04,
    "random-96-s3-dh128": 6.034e-04,
    "random-96-s3-dh256": 2.523e-04,
    "random-160-s6-dh64": 2.562e-04,
    "random-160-s6-dh128": 1.206e-03,
    "random-160-s6-dh256": 3.752e-04,
    "random-288-s1-dh64": 1.914e-04,
    "random-288-s1-dh128": 3.068e-04,
    "random-288-s1-dh256": 2.231e-04,
    "random-288-s3-dh64": 2.321e-04,
    "random-288-s3-dh128": 5.146e-04,
    "random-288-s3-dh256": 2.098e-04,
    "random-288-s6-dh64": 2.267e-04,
    "random-288-s6-dh128": 1.471e-03,
    "random-288-s6-dh256": 3.336e-04,
    "random-1024-s3-dh64": 1.976e-04,
    "random-1024-s3-dh128": 4.627e-04,
    "random-1024-s3-dh256": 3.582e-04,
    "random-packed-s1-dh64": 2.231e-04,
    "random-packed-s1-dh128": 2.576e-04,
    "random-packed-s1-dh256": 2.121e-04,
    "random-packed-longest-last-s3-dh64": 2.461e-04,
    "random-packed-longest-last-s3-dh128": 5.026e-04,
    "random-packed-longest-last-s3-dh256": 2.219e-04,
}


class AttentionCase:
    """qkv [rows][(heads + 2 kv_heads) * dh] fp16, mask [rows] int32, seq_off [B + 1] int32 or None (then row b * T + t),
    target [rows][heads]: the planted key's absolute row (-1: padded query, or a peaked-random case)."""

    def __init__(self, name, family, dh, T, heads, kv_heads, B, qkv, mask, seq_off, target, sharp):
        self.name, self.family, self.dh, self.T, self.heads, self.kv_heads, self.B = name, family, dh, T, heads, kv_heads, B
        self.qkv, self.mask, self.seq_off, self.target, self.sharp = qkv, mask, seq_off, target, sharp
        self.scale = np.float32(1.0) / np.sqrt(np.float32(dh))
        self.ld = (heads + 2 * kv_heads) * dh
        self.rows = qkv.shape[0]

    def sequences(self):
        if self.seq_off is None:
            return [(b * self.T, self.T) for b in range(self.B)]
        return [(int(self.seq_off[b]), int(self.seq_off[b + 1] - self.seq_off[b])) for b in range(self.B)]

    def v_rows(self):
        """V as [rows][kv_heads][dh] (a view)."""
        return self.qkv[:, (self.heads + self.kv_heads) * self.dh:].reshape(self.rows, self.kv_heads, self.dh)

    def vmax(self):
        return float(np.abs(self.v_rows().astype(np.float64)).max())


def _planted_sequence(T, m, dh, heads, kv_heads):
    """q [T][heads][dh], k [T][kv_heads][dh] (float64, exactly representable up to the fp16 rounding of q) and target [T][heads]."""
    KT, inv = KEY_TILE[dh], np.sqrt(float(dh))
    j = np.arange(T)
    valid = m != 0
    r, c = j % 32, j // 32
    f0 = int(np.argmax(valid))
    K = np.zeros((T, dh))
    K[j, r] = 1.0
    K[:, 32] = c
    K[f0, _CLS_FIRST] = _FLAG
    K[j % KT == 0, _CLS_TILE_START] = _FLAG
    K[j % KT == KT - 1, _CLS_TILE_END] = _FLAG
    K[r == 31, _CLS_CHUNK_END] = _FLAG
    K[~valid] = 0.0
    K[~valid, 32] = 128.0
    q = np.zeros((T, heads, dh))
    target = np.full((T, heads), -1, np.int64)
    group = heads // kv_heads
    for hd in range(heads):
        kind = (j + hd) % 5
        tgt = j.copy()
        tgt[kind == 1] = f0
        tgt[(kind == 2) & (j >= 1)] = j[(kind == 2) & (j >= 1)] - 1
        prev_tile = (kind == 3) & (j >= KT) & (j % KT != KT - 1)     # (a query that is itself a tile's last key keeps the diagonal)
        tgt[prev_tile] = (j[prev_tile] // KT) * KT - 1
        tgt[kind == 4] = (j[kind == 4] // KT) * KT
        tgt = np.where(valid[tgt] & (tgt <= j), tgt, j)
        F = np.full((T, 32), -PLANT_U)
        bait = r < 31
        F[j[bait], r[bait] + 1] = PLANT_U
        near = c[tgt] == c
        F[j[near], r[tgt[near]]] = 0.0
        Q = np.zeros((T, dh))
        Q[:, :32] = F * inv
        Q[:, 32] = PLANT_CHUNK * inv
        far = ~near
        cls = np.select([kind == 1, kind == 2, kind == 3, kind == 4], [_CLS_FIRST, _CLS_CHUNK_END, _CLS_TILE_END, _CLS_TILE_START], 0)
        assert np.all(cls[far] > 0)
        bonus = PLANT_CHUNK * (c - c[tgt]) - F[j, r[tgt]]
        Q[j[far], cls[far]] = bonus[far] * inv / _FLAG
        Q[~valid] = 0.0
        q[:, hd] = np.roll(Q, 3 * (hd // group), axis=1)
        target[:, hd] = np.where(valid, tgt, -1)
    k = np.stack([np.roll(K, 3 * hk, axis=1) for hk in range(kv_heads)], axis=1)
    return q, k, target


def build_attention_case(spec, dh, seed=0):
    name, family, T, (heads, kv_heads), rows_spec, sharp = spec
    rng = np.random.default_rng([seed, dh, zlib.crc32(name.encode())])
    if rows_spec[0] == "packed":
        lens = list(rows_spec[1:])
        l32 = [(n + 31) // 32 * 32 for n in lens]
        assert max(l32) == T
        seq_off = np.concatenate([[0], np.cumsum(l32)]).astype(np.int32)
        masks = [row_mask(L, ("valid", n)) for L, n in zip(l32, lens)]
    else:
        seq_off = None
        masks = [row_mask(T, pad) for pad in rows_spec]
    B = len(masks)
    mask = np.concatenate(masks).astype(np.int32)
    rows = mask.size
    qd, kd = heads * dh, kv_heads * dh
    qkv = rng.standard_normal((rows, qd + 2 * kd)).astype(np.float16)
    target = np.full((rows, heads), -1, np.int64)
    if family == "planted":
        row0 = 0
        for m in masks:
            L = m.size
            q, k, tgt = _planted_sequence(L, m, dh, heads, kv_heads)
            qkv[row0:row0 + L, :qd] = q.reshape(L, qd).astype(np.float16)
            qkv[row0:row0 + L, qd:qd + kd] = k.reshape(L, kd).astype(np.float16)
            target[row0:row0 + L] = np.where(tgt >= 0, tgt + row0, -1)
            row0 += L
    else:
        qkv[:, :qd] = (qkv[:, :qd].astype(np.float32) * np.float32(sharp)).astype(np.float16)
    return AttentionCase(f"{name}-dh{dh}", family, dh, T, heads, kv_heads, B, qkv, mask, seq_off, target, sharp)


_case_cache = {}


def attention_case(name, dh):
    """The case of that name (built once per process; treat it as read-only)."""
    key = (name, dh)
    if key not in _case_cache:
        spec = next(s for s in ATTENTION_CASES if s[0] == name)
        _case_cache[key] = build_attention_case(spec, dh)
    return _case_cache[key]


# ---- float64 reference -----------------------------------------------------------------------------------------------------------
def attention_reference(case, causal_shift=0, ignore_mask=False, kv_map="div", target_weight=False):
    """Causal grouped-query attention in float64 over the fp16 inputs: true -inf masking, key padding mask, optional packing.
    Returns out [rows][heads * dh] (NaN rows where a query sees no key), and with target_weight the softmax weight of the planted key.
    The three keyword switches build the MUTANT references of the host test: causal_shift=1 admits key i + 1, ignore_mask drops the
    padding mask, kv_map='mod' maps head hd to kv head hd % kv_heads instead of hd // (heads / kv_heads)."""
    dh, heads, kv_heads = case.dh, case.heads, case.kv_heads
    qd, kd, group = heads * dh, kv_heads * dh, heads // kv_heads
    out = np.full((case.rows, qd), np.nan)
    tw = np.full((case.rows, heads), np.nan)
    scale = float(case.scale)
    for row0, T in case.sequences():
        blk = case.qkv[row0:row0 + T].astype(np.float64)
        m = case.mask[row0:row0 + T] != 0
        jj = np.arange(T)
        for hd in range(heads):
            hk = hd // group if kv_map == "div" else hd % kv_heads
            q = blk[:, hd * dh:(hd + 1) * dh]
            k = blk[:, qd + hk * dh:qd + (hk + 1) * dh]
            v = blk[:, qd + kd + hk * dh:qd + kd + (hk + 1) * dh]
            for i0 in range(0, T, 512):
                i1 = min(T, i0 + 512)
                s = (q[i0:i1] @ k.T) * scale
                vis = jj[None, :] <= (jj[i0:i1, None] + causal_shift)
                if not ignore_mask:
                    vis = vis & m[None, :]
                s = np.where(vis, s, -np.inf)
                with np.errstate(invalid="ignore"):
                    p = np.exp(s - s.max(axis=1, keepdims=True))
                    z = p.sum(axis=1, keepdims=True)
                    out[row0 + i0:row0 + i1, hd * dh:(hd + 1) * dh] = (p @ v) / z
                    if target_weight:
                        t = case.target[row0 + i0:row0 + i1, hd]
                        ok = t >= 0
                        tw[row0 + i0:row0 + i1, hd][ok] = (p / z)[np.nonzero(ok)[0], t[ok] - row0]
    return (out, tw) if target_weight else out


def planted_expected(case):
    """V[j(i)] for every (row, head): [rows][heads * dh] float64, NaN where the query is padded."""
    v = case.v_rows().astype(np.float64)
    group = case.heads // case.kv_heads
    out = np.full((case.rows, case.heads, case.dh), np.nan)
    for hd in range(case.heads):
        t = case.target[:, hd]
        ok = t >= 0
        out[ok, hd] = v[t[ok], hd // group]
    return out.reshape(case.rows, case.heads * case.dh)


# ---- the kernel's arithmetic, in NumPy -------------------------------------------------------------------------------------------
def attention_model_fp16(case):
    """k_attention_stream2<DH, true>'s roundings: q * scale rounded to fp16, fp32 scores, additive -30000 padding mask and -30000 on
    the keys past the diagonal, online softmax per key tile with exp2 and the log2(e) fold, probabilities rounded to fp16 for the PV
    product (their fp32 values summed for the normaliser), output rounded to fp16.  Accumulation order inside a product, the device's
    exp2 and the fused multiply-adds are NOT reproduced: the GPU bound doubles this model's error for them."""
    dh, heads, kv_heads = case.dh, case.heads, case.kv_heads
    qd, kd, group, KT = heads * dh, kv_heads * dh, heads // kv_heads, KEY_TILE[dh]
    out = np.zeros((case.rows, qd), np.float16)
    f32 = np.float32
    for row0, T in case.sequences():
        blk = case.qkv[row0:row0 + T]
        madd = np.where(case.mask[row0:row0 + T] != 0, f32(0), MASKED).astype(f32)
        jj = np.arange(T)
        for hd in range(heads):
            hk = hd // group
            qs = (blk[:, hd * dh:(hd + 1) * dh].astype(f32) * case.scale).astype(np.float16).astype(f32)
            k = blk[:, qd + hk * dh:qd + (hk + 1) * dh].astype(f32)
            v = blk[:, qd + kd + hk * dh:qd + kd + (hk + 1) * dh].astype(f32)
            m_run = np.full(T, -1e30, f32)
            l_run = np.zeros(T, f32)
            o = np.zeros((T, dh), f32)
            for kt in range(0, T, KT):
                ke = min(T, kt + KT)
                live = jj >= kt                                   # queries that can see a key of this tile
                s = qs[live] @ k[kt:ke].T + madd[None, kt:ke]
                s = np.where(jj[None, kt:ke] > jj[live, None], MASKED, s).astype(f32)
                m_new = np.maximum(m_run[live], s.max(axis=1))
                alpha = np.exp2((m_run[live] - m_new) * LOG2E).astype(f32)
                p = np.exp2(s * LOG2E - (m_new * LOG2E)[:, None]).astype(f32)
                l_run[live] = l_run[live] * alpha + p.sum(axis=1, dtype=f32)
                o[live] = o[live] * alpha[:, None] + p.astype(np.float16).astype(f32) @ v[kt:ke]
                m_run[live] = m_new
            out[row0:row0 + T, hd * dh:(hd + 1) * dh] = (o / l_run[:, None]).astype(np.float16)
    return out


def valid_rows(case):
    return case.mask != 0


# ---- the small kernels -----------------------------------------------------------------------------------------------------------
def rope_table_reference(theta, T, dh):
    """cos / sin of pos * theta^(-2 j / dh) in float64: ([T][dh / 2] cos, sin, angle)."""
    j = np.arange(dh // 2, dtype=np.float64)
    inv_freq = np.float64(np.float32(theta)) ** (-2.0 * j / dh)
    ang = np.arange(T, dtype=np.float64)[:, None] * inv_freq[None, :]
    return np.cos(ang), np.sin(ang), ang


def rope_table_bound(angle):
    """|device - float64|: powf within two ulps (2^-22 relative on the frequency), the fp32 product pos * inv_freq (2^-24 relative),
    both scaled by the angle since |d cos| , |d sin| <= |d angle|; plus sincosf's own result (2^-23: under two ulps near 1)."""
    return angle * (2.0 ** -22 + 2.0 ** -24) + 2.0 ** -23


def _h(x):
    """Round to fp16, back in float64."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def qknorm_rope_reference(qkv, T, heads, kv_heads, dh, qw, kw, eps, qk_norm, cos, sin, pos_ids=None, round16=True):
    """Per-head RMSNorm over head_dim (optional) and rotate-half RoPE on the q and k parts of qkv [M][(heads + 2 kv_heads) * dh], in
    float64 with HF's fp16 rounding points: after the normalisation, after the weight multiply, and the result.  V is copied.
    Returns (out float64 holding fp16 values, bound): bound[m][e] is what one flipped ulp at each rounding point allows (below).
    round16=False drops the three roundings (the comparison with transformers in fp32)."""
    rnd = _h if round16 else (lambda a: a)
    M = qkv.shape[0]
    x = qkv.astype(np.float64)
    out = x.copy()
    bound = np.zeros_like(x)
    pos = np.asarray(pos_ids) if pos_ids is not None else np.arange(M) % T
    c, s = cos[pos], sin[pos]                                   # [M][dh / 2]
    half = dh // 2
    for hh in range(heads + kv_heads):
        w = np.asarray(qw if hh < heads else kw, np.float64)
        v = x[:, hh * dh:(hh + 1) * dh]
        if qk_norm:
            r = 1.0 / np.sqrt((v * v).mean(axis=1, keepdims=True) + float(eps))
            v = rnd(rnd(v * r) * w[None, :])
        x1, x2 = v[:, :half], v[:, half:]
        out[:, hh * dh:hh * dh + half] = rnd(x1 * c - x2 * s)
        out[:, hh * dh + half:(hh + 1) * dh] = rnd(x2 * c + x1 * s)
        # One fp16 ulp of a value y is at most 2^-10 |y|.  A flip at the normalisation moves x by <= 2^-10 |x| (the weight multiplies
        # the value and its error alike), a flip after the weight multiply by another 2^-10 |x|; the rotation is orthogonal, so
        # (dx1, dx2) of length <= 2 * 2^-10 hypot(x1, x2) moves either output by at most that; the output's own flip adds
        # 2^-10 |out| <= 2^-10 hypot(x1, x2).  x1, x2 are the rotation's inputs, i.e. AFTER the weight: max(1, |w|) is not needed.
        # Without qk_norm only the last rounding exists.
        hyp = np.hypot(x1, x2) * ((3 if qk_norm else 1) * 2.0 ** -10)
        bound[:, hh * dh:hh * dh + half] = hyp
        bound[:, hh * dh + half:(hh + 1) * dh] = hyp
    return out, bound


def rmsnorm_reference(x, w, woff, eps):
    """y = x * rsqrt(mean(x^2) + eps) * (w + woff) in float64 over the fp32 inputs."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    return x / np.sqrt((x * x).mean(axis=1, keepdims=True) + float(eps)) * (w[None, :] + float(woff))


RSQRT_REL = 2.0 ** -23                # an fp32 1 / sqrt(x) from two correctly rounded operations: half an ulp each (host test)


def silu_reference(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def gelu_tanh_reference(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def swiglu_reference(gu, F, act_kind):
    """act(gate) * up in float64 over gu [M][2 F] fp16 (gate | up)."""
    g, u = gu[:, :F].astype(np.float64), gu[:, F:].astype(np.float64)
    return (gelu_tanh_reference(g) if act_kind == 1 else silu_reference(g)) * u


GELU_TANH_FIT_BOUND = 5.4e-6          # stated beside gelu_tanh in csrc/vf_transformer.hip (tools/fit_gelu.py --tanh)
FP16_SUBNORMAL_QUANTUM = 2.0 ** -24


def swiglu_bound(gu, F, act_kind, ref):
    """One fp16 rounding of the result (2^-11 |ref|, or the subnormal quantum below the normal range) plus the activation's own error
    times |up|: the fit bound of gelu_tanh, or for SiLU 2^-22 |x| (__expf scales its argument in fp32: 2^-24 |x| relative on the
    exponential, the add and the division within another 2^-23)."""
    g, u = np.abs(gu[:, :F].astype(np.float64)), np.abs(gu[:, F:].astype(np.float64))
    act_err = GELU_TANH_FIT_BOUND if act_kind == 1 else 2.0 ** -22 * g
    return 2.0 ** -11 * np.abs(ref) + act_err * u + FP16_SUBNORMAL_QUANTUM


def all_finite_fp16():
    """Every finite fp16 value, both signs (63488 of them), padded with zeros to a multiple of 8."""
    bits = np.arange(1 << 16, dtype=np.uint16)
    vals = bits.view(np.float16)
    vals = vals[np.isfinite(vals)]
    return np.concatenate([vals, np.zeros(-vals.size % 8, np.float16)])


def gather_reference(ids, table, scale):
    """fp32(fp16 row) * scale: one fp32 multiply per element, so the kernel must match bit for bit."""
    return table[np.asarray(ids)].astype(np.float32) * np.float32(scale)


def last_token_index(mask, B, T, Tv, seq_off=None):
    """Row (absolute) that last-token pooling selects for each sequence.  Padded rows [B][T]: column Tv - 1 if EVERY row's bit Tv - 1
    is set, else sum(mask[:Tv]) - 1, and 0 for a row with no token.  Packed: the count of the sequence's rows minus one."""
    mask = np.asarray(mask)
    if seq_off is not None:
        out = []
        for b in range(B):
            r0, r1 = int(seq_off[b]), int(seq_off[b + 1])
            n = int((mask[r0:r1] != 0).sum())
            out.append(r0 + (n - 1 if n > 0 else 0))
        return np.asarray(out, np.int64), 0
    m = mask.reshape(B, T)[:, :Tv] != 0
    all_last = bool(m[:, Tv - 1].all())
    if all_last:
        return np.arange(B, dtype=np.int64) * T + (Tv - 1), 1
    n = m.sum(axis=1)
    return np.arange(B, dtype=np.int64) * T + np.where(n > 0, n - 1, 0), 0
