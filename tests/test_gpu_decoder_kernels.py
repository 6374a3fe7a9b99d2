"""The decoder's kernels ONE BY ONE against the float64 references of tests/decoder_cases.py, through the vf_debug_dec_* hooks
(csrc/vf_transformer.hip), which launch each kernel with the grid arithmetic of the forward itself (dec_launch_*).

Every output buffer is filled with NaN first and what lies outside the case must still be NaN afterwards.  Every bound is derived
where it is used (number formats and the reference's own error, never a kernel's output) and every measured value is printed and
recorded next to
its bound through the decoder tests' own record (test_gpu_encoder._measured)."""
import ctypes

import numpy as np
import pytest
import torch

import decoder_cases as DC
from test_gpu_encoder import _measured
from veritasfi_amd import _ffi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_I, _F, _P = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
_SIGNATURES = {
    "vf_debug_dec_attention": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _I, _P],
    "vf_debug_dec_rope_table": [_F, _I, _I, _P, _P],
    "vf_debug_dec_qknorm_rope": [_P, _I, _I, _I, _I, _I, _P, _P, _F, _I, _P, _P, _P],
    "vf_debug_dec_rmsnorm": [_P, _P, _F, _F, _I, _I, _P, _I, _P],
    "vf_debug_dec_swiglu": [_P, _I, _I, _I, _P, _P],
    "vf_debug_dec_gather_rows": [_P, _P, _I, _I, _F, _P, _P],
    "vf_debug_dec_token_logit": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
    "vf_debug_dec_pool_last": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P],
}


def _hook(name):
    fn = getattr(_ffi.lib(), name)
    fn.restype, fn.argtypes = _I, _SIGNATURES[name]
    return fn


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ---- causal grouped-query attention: k_attention_stream2<64 / 128 / 256, true> ---------------------------------------------------
def _run_attention(case, pad_cols):
    """ctx [rows + 8][heads * dh + pad_cols] fp16 after one launch; the 8 extra rows and the pad columns must stay NaN."""
    qd = case.heads * case.dh
    qkv, mask = _dev(case.qkv), _dev(case.mask)
    seq_off = None if case.seq_off is None else _dev(case.seq_off)
    ctx = _nan((case.rows + 8, qd + pad_cols), torch.float16)
    rc = _hook("vf_debug_dec_attention")(qkv.data_ptr(), mask.data_ptr(), _ptr(seq_off), case.B, case.T, case.heads, case.kv_heads,
                                         case.dh, float(case.scale), ctx.data_ptr(), qd + pad_cols, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = ctx.cpu().numpy()
    assert np.isnan(got[case.rows:]).all(), "rows past the case were written"
    assert np.isnan(got[:, qd:]).all(), "columns past heads * head_dim were written"
    return got[:case.rows, :qd].astype(np.float64)


@pytest.mark.parametrize("dh", DC.HEAD_DIMS)
@pytest.mark.parametrize("name", [s[0] for s in DC.ATTENTION_CASES if s[1] == "planted"])
def test_causal_attention_planted(name, dh):
    """Every valid query row of every head returns V[j(i)], the one key the float64 softmax leaves (weight >= 1 - 1e-6, checked on
    the CPU).  Bound 2^-10 max|v|: one fp16 rounding of the output (2^-11) plus one of the winning probability (2^-11).  A key
    admitted past the diagonal, through the padding mask or from another kv head costs >= 0.5 max|v| (a condition of the case, see
    tests/test_decoder_cases_host.py), so the bound is a yes / no, not a measurement."""
    case = DC.attention_case(name, dh)
    got = _run_attention(case, 64 if "packed" in name or "288" in name else 0)
    valid = DC.valid_rows(case)
    want = DC.planted_expected(case)
    assert np.isfinite(got[valid]).all()
    err = np.abs(got[valid] - want[valid])
    vmax = case.vmax()
    _measured(f"attention_planted[{case.name}]", err_over_vmax=err.max() / vmax, bound_over_vmax=2.0 ** -10,
              rows_off=int((err.max(axis=1) > 2.0 ** -10 * vmax).sum()), rows=int(valid.sum()))
    bad = np.argwhere(err > 2.0 ** -10 * vmax)
    assert bad.size == 0, f"{case.name}: {len(bad)} elements off, first (valid row #, column) {bad[0].tolist()}, " \
                          f"row {np.nonzero(valid)[0][bad[0][0]]}, worst {err.max() / vmax:.3g} max|v|"


@pytest.mark.parametrize("dh", DC.HEAD_DIMS)
@pytest.mark.parametrize("name", [s[0] for s in DC.ATTENTION_CASES if s[1] == "random"])
def test_causal_attention_peaked_random(name, dh):
    """Against the float64 softmax.  Bound: TWICE the error of the fp16-faithful NumPy model on this very case (decoder_cases.MODEL_ERR,
    computed on the CPU); the factor two is for accumulation order, the device's exp2 and the fp32 rescaling steps the model does not
    reproduce one by one."""
    case = DC.attention_case(name, dh)
    got = _run_attention(case, 64 if "packed" in name else 0)
    valid = DC.valid_rows(case)
    ref = DC.attention_reference(case)
    assert np.isfinite(got[valid]).all()
    vmax = case.vmax()
    err = float(np.abs(got[valid] - ref[valid]).max() / vmax)
    bound = 2.0 * DC.MODEL_ERR[case.name]
    _measured(f"attention_random[{case.name}]", err_over_vmax=err, bound_over_vmax=bound)
    assert err <= bound, (case.name, err, bound)


def test_attention_hook_refuses_before_launching():
    """T % 32 != 0, T > 4096, heads % kv_heads != 0 and another head dim return -2 and leave ctx untouched."""
    hook = _hook("vf_debug_dec_attention")
    for T, heads, kvh, dh in ((48, 2, 1, 64), (4128, 2, 1, 64), (64, 3, 2, 64), (64, 2, 1, 96), (64, 2, 1, 32)):
        rows = 64          # (never read: the refusal comes first)
        qkv = torch.zeros(rows, (heads + 2 * kvh) * dh, dtype=torch.float16, device=DEV)
        mask = torch.ones(rows, dtype=torch.int32, device=DEV)
        ctx = _nan((rows, heads * dh), torch.float16)
        rc = hook(qkv.data_ptr(), mask.data_ptr(), None, 1, T, heads, kvh, dh, 0.125, ctx.data_ptr(), heads * dh, _stream())
        torch.cuda.synchronize()
        assert rc == -2, (T, heads, kvh, dh, rc)
        assert bool(torch.isnan(ctx).all())


# ---- k_rope_table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", DC.HEAD_DIMS)
@pytest.mark.parametrize("theta", [1e4, 1e6])
def test_rope_table(theta, dh):
    """The whole table, positions 0..4095.  |d| <= angle * (2^-22 + 2^-24) + 2^-23 (decoder_cases.rope_table_bound): it also shows
    that sincosf reduces arguments up to ~4095 rad correctly."""
    T = 4096
    tab = _nan((T + 1, dh // 2, 2), torch.float32)
    assert _hook("vf_debug_dec_rope_table")(theta, T, dh, tab.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = tab.cpu().numpy().astype(np.float64)
    assert np.isnan(got[T]).all()
    cos, sin, ang = DC.rope_table_reference(theta, T, dh)
    bound = DC.rope_table_bound(ang)
    ec, es = np.abs(got[:T, :, 0] - cos), np.abs(got[:T, :, 1] - sin)
    _measured(f"rope_table[{theta:g},{dh}]", max_err=max(ec.max(), es.max()), worst_ratio_to_bound=max((ec / bound).max(), (es / bound).max()),
              bound_at_worst_angle=bound.max())
    assert np.all(ec <= bound) and np.all(es <= bound)


# ---- k_qknorm_rope ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", DC.HEAD_DIMS)
def test_qknorm_rope(dh):
    """heads {1, 3, 4} (1: the first q part is EMPTY) x kv_heads {1, 2} x M {1, tokens per workgroup + 1} x qk_norm x positions from
    tok % T (T = 48 < M wraps) or from pos_ids holding 0 and 4095.  The kernel reads the float64 table rounded to fp32, so only
    its own arithmetic is measured.  Bound per element: decoder_cases.qknorm_rope_reference (one flipped fp16 ulp at each of HF's
    three rounding points; one without qk_norm).  The V part and the rows past M keep their bits."""
    hook = _hook("vf_debug_dec_qknorm_rope")
    rng = np.random.default_rng(dh)
    T, eps = 48, 1e-6
    cos, sin, _ = DC.rope_table_reference(1e6, 4096, dh)
    tab = _dev(np.stack([cos, sin], axis=-1).astype(np.float32))
    worst, beyond, total = 0.0, 0, 0
    for heads in (1, 3, 4):
        for kvh in (1, 2):
            for M in (1, DC.QK_TOKENS_PER_WG[dh] + 1):
                for qk_norm in (1, 0):
                    for use_pos in (False, True):
                        ld = (heads + 2 * kvh) * dh
                        x = (rng.standard_normal((M + 3, ld)) * rng.choice([0.05, 1.0, 20.0], size=(M + 3, 1))).astype(np.float16)
                        x[M:] = np.float16("nan")
                        qw = (1 + 0.3 * rng.standard_normal(dh)).astype(np.float32)
                        kw = (1 + 0.3 * rng.standard_normal(dh)).astype(np.float32)
                        pos = None
                        if use_pos:
                            pos = rng.integers(0, 4096, size=M).astype(np.int32)
                            pos[0] = 4095
                            pos[-1] = 0 if M > 1 else 4095
                        want, bound = DC.qknorm_rope_reference(x[:M], T, heads, kvh, dh, qw, kw, eps, qk_norm, cos, sin, pos_ids=pos)
                        buf, dq, dk = _dev(x), _dev(qw), _dev(kw)
                        dpos = None if pos is None else _dev(pos)
                        assert hook(buf.data_ptr(), M, T, heads, kvh, dh, dq.data_ptr(), dk.data_ptr(), eps, qk_norm, tab.data_ptr(),
                                    _ptr(dpos), _stream()) == 0
                        torch.cuda.synchronize()
                        got = buf.cpu().numpy()
                        what = (heads, kvh, M, qk_norm, use_pos)
                        assert np.array_equal(got[M:].view(np.uint16), x[M:].view(np.uint16)), (what, "rows past M were written")
                        vcol = (heads + kvh) * dh
                        assert np.array_equal(got[:M, vcol:].view(np.uint16), x[:M, vcol:].view(np.uint16)), (what, "V was written")
                        err = np.abs(got[:M, :vcol].astype(np.float64) - want[:, :vcol])
                        ratio = err / bound[:, :vcol]
                        assert np.all(err <= bound[:, :vcol]), (what, float(ratio.max()), np.argwhere(err > bound[:, :vcol])[0].tolist())
                        worst = max(worst, float(ratio.max()))
                        ulp = np.spacing(np.abs(want[:, :vcol]).astype(np.float16)).astype(np.float64)
                        beyond += int((err > ulp).sum())
                        total += err.size
    _measured(f"qknorm_rope[{dh}]", worst_ratio_to_bound=worst, share_beyond_one_output_ulp=beyond / total)


# ---- k_rmsnorm -------------------------------------------------------------------------------------------------------------------
# The roundings on an output element besides the reciprocal square root: w + woff, x * r, the product with the gain, and the
# statistics (mean of squares, + eps) whose error the square root halves -- 4 * 2^-24 relative in all.  For rsqrtf itself no
# vendor table is at hand, so its term is the error of an fp32 reciprocal square root built from two correctly rounded operations
# (decoder_cases.RSQRT_REL = 2^-23, measured against float64 in tests/test_decoder_cases_host.py).
RMS_FP32_REL = 4 * 2.0 ** -24 + DC.RSQRT_REL


@pytest.mark.parametrize("out_fp32", [1, 0])
@pytest.mark.parametrize("H", [32, 136, 1024, 2560])
def test_rmsnorm(H, out_fp32):
    """H 32 (8 chunks: most lanes idle), 136 (34 chunks: a second trip for two lanes), 1024, 2560; M in {1, 7, 8, 9} around the eight
    rows of a workgroup; woff 0 / 1; rows of magnitude 1e-20 (squares underflow: eps alone), 1 and 3e4.  fp32 output: RMS_FP32_REL
    relative; fp16 output: that plus one fp16 rounding, 2^-11 relative or half the subnormal spacing (2^-25) below the normal range."""
    hook = _hook("vf_debug_dec_rmsnorm")
    rng = np.random.default_rng(H)
    worst = 0.0
    for M in (1, 7, 8, 9):
        for woff in (0.0, 1.0):
            x = (rng.standard_normal((M, H)) * np.resize([1e-20, 1.0, 3e4], M)[:, None]).astype(np.float32)
            w = (0.3 * rng.standard_normal(H) + (0.0 if woff else 1.0)).astype(np.float32)
            want = DC.rmsnorm_reference(x, w, woff, 1e-6)
            y = _nan((M + 2, H), torch.float32 if out_fp32 else torch.float16)
            dx, dw = _dev(x), _dev(w)
            assert hook(dx.data_ptr(), dw.data_ptr(), woff, 1e-6, M, H, y.data_ptr(), out_fp32, _stream()) == 0
            torch.cuda.synchronize()
            got = y.cpu().numpy().astype(np.float64)
            assert np.isnan(got[M:]).all(), (M, woff, "rows past M were written")
            bound = RMS_FP32_REL * np.abs(want)
            if not out_fp32:
                bound = bound + np.maximum(2.0 ** -11 * np.abs(want), 2.0 ** -25)
            err = np.abs(got[:M] - want)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound), (M, woff, float((err / np.maximum(bound, 1e-300)).max()), np.argwhere(err > bound)[0].tolist())
    _measured(f"rmsnorm[{H},{'fp32' if out_fp32 else 'fp16'}]", worst_ratio_to_bound=worst, fp32_rel_bound=RMS_FP32_REL)


# ---- k_swiglu --------------------------------------------------------------------------------------------------------------------
def _run_swiglu(gu, F, act_kind):
    M = gu.shape[0]
    out = _nan((M + 1, F), torch.float16)
    dgu = _dev(gu)
    assert _hook("vf_debug_dec_swiglu")(dgu.data_ptr(), M, F, act_kind, out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[M]).all(), "the row past M was written"
    return got[:M].astype(np.float64)


@pytest.mark.parametrize("act_kind", [0, 1])
def test_swiglu_every_finite_fp16_gate(act_kind):
    """act(x) * 1 for every finite fp16 x, with the device's exp2 / __expf.  Bound (decoder_cases.swiglu_bound): 2^-11 |ref| + the fp16
    subnormal quantum + the activation's own error -- 5.4e-6 for the degree-5 tanh-GELU fit (stated at gelu_tanh), 2^-22 |x| for SiLU."""
    g = DC.all_finite_fp16()
    F = g.size
    gu = np.concatenate([g, np.ones(F, np.float16)])[None, :]
    ref = DC.swiglu_reference(gu, F, act_kind)
    bound = DC.swiglu_bound(gu, F, act_kind, ref)
    got = _run_swiglu(gu, F, act_kind)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    k = int(np.argmax(err / bound))
    _measured(f"swiglu_all_fp16[{'gelu_tanh' if act_kind else 'silu'}]", worst_ratio_to_bound=(err / bound).max(), at_gate=float(g[k]),
              max_abs_err_below_8=float(err[0][np.abs(g.astype(np.float64)) < 8].max()))
    assert np.all(err <= bound), (float(g[k]), float(err[0, k]), float(bound[0, k]))


@pytest.mark.parametrize("act_kind", [0, 1])
def test_swiglu_tail_and_row_stride(act_kind):
    """F = 2056: F / 8 = 257 chunks, one past a 256-thread block.  M = 32769 with F = 8: the grid holds 32768 rows, row 32768 is the
    second trip of block 0's row loop."""
    rng = np.random.default_rng(act_kind)
    worst = 0.0
    for M, F in ((5, 2056), (32769, 8)):
        gu = (rng.standard_normal((M, 2 * F)) * 3).astype(np.float16)
        ref = DC.swiglu_reference(gu, F, act_kind)
        bound = DC.swiglu_bound(gu, F, act_kind, ref)
        err = np.abs(_run_swiglu(gu, F, act_kind) - ref)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (M, F, np.argwhere(err > bound)[0].tolist(), float((err / bound).max()))
    _measured(f"swiglu_shapes[{'gelu_tanh' if act_kind else 'silu'}]", worst_ratio_to_bound=worst)


# ---- k_gather_rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 2560])
def test_gather_rows(H):
    """Bit-equal to fp32(fp16 row) * scale; ids hold 0 and vocab - 1; M 1 and 9 (a second workgroup); scale 1 and sqrt(H)."""
    hook = _hook("vf_debug_dec_gather_rows")
    rng = np.random.default_rng(H)
    vocab = 37
    table = rng.standard_normal((vocab, H)).astype(np.float16)
    dt = _dev(table)
    for M in (1, 9):
        for scale in (1.0, float(np.sqrt(np.float32(H)))):
            ids = rng.integers(0, vocab, size=M).astype(np.int32)
            ids[0] = vocab - 1
            ids[-1] = 0 if M > 1 else vocab - 1
            out = _nan((M + 2, H), torch.float32)
            di = _dev(ids)
            assert hook(di.data_ptr(), dt.data_ptr(), M, H, scale, out.data_ptr(), _stream()) == 0
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.isnan(got[M:]).all()
            assert np.array_equal(got[:M].view(np.uint32), DC.gather_reference(ids, table, scale).view(np.uint32)), (M, scale)


# ---- last-token selection: k_token_logit and k_pool (pooling 2) ------------------------------------------------------------------------
def _last_token_layouts():
    """(name, mask [rows], B, T, Tv, seq_off)"""
    T = 64
    right = np.stack([DC.row_mask(T, ("valid", n)) for n in (64, 10, 33, 1, 0)])             # the last row holds NO token
    left = np.zeros((4, T), np.int32)                                                        # t_valid = 50 < t = 64
    for b, n in enumerate((50, 3, 1, 20)):
        left[b, 50 - n:50] = 1
    mixed = left.copy()
    mixed[1] = DC.row_mask(T, ("valid", 7))                                                  # one right-padded row: the count decides
    lens = (70, 17, 96, 1)
    l32 = [(n + 31) // 32 * 32 for n in lens]
    packed = np.concatenate([DC.row_mask(L, ("valid", n)) for L, n in zip(l32, lens)])
    seq_off = np.concatenate([[0], np.cumsum(l32)]).astype(np.int32)
    return [("right", right.reshape(-1), 5, T, T, None), ("left", left.reshape(-1), 4, T, 50, None),
            ("mixed", mixed.reshape(-1), 4, T, 50, None), ("packed", packed, 4, 96, 96, seq_off)]


@pytest.mark.parametrize("H", [136, 2560])
def test_last_token_pool_and_logit(H):
    """Right-padded rows, left-padded rows with t_valid < t (every row's bit t_valid - 1 set: column t_valid - 1), a row without any
    token (row 0 of its sequence), packed rows.  The pooled row is bit-equal to fp32 of the selected input row; the logit matches the
    float64 dot within H * 2^-24 * sum |x_j w_j| (fp32 accumulation of H exact products in any order)."""
    rng = np.random.default_rng(H)
    for name, mask, B, T, Tv, seq_off in _last_token_layouts():
        rows = mask.size
        x = rng.standard_normal((rows, H)).astype(np.float16)
        w = rng.standard_normal(H).astype(np.float16)
        tok, all_last = DC.last_token_index(mask, B, T, Tv, seq_off)
        assert all_last == (1 if name == "left" else 0)
        dx, dm, dw = _dev(x), _dev(mask.astype(np.int32)), _dev(w)
        ds = None if seq_off is None else _dev(seq_off)
        pooled = _nan((B + 1, H), torch.float32)
        logit = _nan((B + 1,), torch.float32)
        assert _hook("vf_debug_dec_pool_last")(dx.data_ptr(), dm.data_ptr(), _ptr(ds), B, T, Tv, H, all_last, 0, pooled.data_ptr(), _stream()) == 0
        assert _hook("vf_debug_dec_token_logit")(dx.data_ptr(), dm.data_ptr(), _ptr(ds), B, T, Tv, H, all_last, dw.data_ptr(),
                                                 logit.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        gp, gl = pooled.cpu().numpy(), logit.cpu().numpy()
        assert np.isnan(gp[B]).all() and np.isnan(gl[B])
        assert np.array_equal(gp[:B].view(np.uint32), x[tok].astype(np.float32).view(np.uint32)), (name, tok.tolist())
        prod = x[tok].astype(np.float64) * w.astype(np.float64)[None, :]
        err = np.abs(gl[:B].astype(np.float64) - prod.sum(axis=1))
        bound = H * 2.0 ** -24 * np.abs(prod).sum(axis=1)
        _measured(f"token_logit[{name},{H}]", worst_ratio_to_bound=(err / bound).max())
        assert np.all(err <= bound), (name, err.tolist(), bound.tolist())
