"""CPU checks of tests/decoder_cases.py: the NumPy references against transformers' own modules in fp32, every planted attention
case against the conditions that make it a test (in float64, on the inputs alone), and the fp16-faithful model's error per
peaked-random case against the numbers recorded in decoder_cases.MODEL_ERR (which size the GPU test's bound)."""
import types

import numpy as np
import pytest

import decoder_cases as DC

PLANTED = [s[0] for s in DC.ATTENTION_CASES if s[1] == "planted"]
RANDOM = [s[0] for s in DC.ATTENTION_CASES if s[1] == "random"]


# ---- the references agree with transformers (fp32, CPU) --------------------------------------------------------------------------
@pytest.mark.parametrize("dh,heads,kv_heads", [(64, 4, 2), (128, 3, 1), (256, 1, 1)])
def test_qknorm_rope_reference_matches_qwen3(dh, heads, kv_heads):
    """q_norm / k_norm (Qwen3RMSNorm over head_dim) then apply_rotary_pos_emb, against the reference without its fp16 roundings."""
    import torch
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm, apply_rotary_pos_emb
    rng = np.random.default_rng(dh)
    M, T, eps = 40, 4096, 1e-6
    qkv = rng.standard_normal((M, (heads + 2 * kv_heads) * dh)).astype(np.float16)
    qw = (1 + 0.3 * rng.standard_normal(dh)).astype(np.float32)
    kw = (1 + 0.3 * rng.standard_normal(dh)).astype(np.float32)
    pos = rng.integers(0, 4096, size=M)
    pos[0], pos[1] = 0, 4095
    cos, sin, _ = DC.rope_table_reference(1e6, T, dh)
    got, _ = DC.qknorm_rope_reference(qkv, T, heads, kv_heads, dh, qw, kw, eps, 1, cos, sin, pos_ids=pos, round16=False)
    x = torch.from_numpy(qkv.astype(np.float32))
    qn, kn = Qwen3RMSNorm(dh, eps=eps), Qwen3RMSNorm(dh, eps=eps)
    with torch.no_grad():
        qn.weight.copy_(torch.from_numpy(qw))
        kn.weight.copy_(torch.from_numpy(kw))
        q = qn(x[:, :heads * dh].view(1, M, heads, dh)).transpose(1, 2)
        k = kn(x[:, heads * dh:(heads + kv_heads) * dh].view(1, M, kv_heads, dh)).transpose(1, 2)
        c = torch.from_numpy(np.concatenate([cos[pos], cos[pos]], axis=1).astype(np.float32))[None]
        s = torch.from_numpy(np.concatenate([sin[pos], sin[pos]], axis=1).astype(np.float32))[None]
        q, k = apply_rotary_pos_emb(q, k, c, s)
    want = np.concatenate([q.transpose(1, 2).reshape(M, heads * dh).numpy(), k.transpose(1, 2).reshape(M, kv_heads * dh).numpy()], axis=1)
    err = np.abs(got[:, :(heads + kv_heads) * dh] - want).max()
    # fp32 on HF's side: ~dh roundings in the mean, a handful after it, on values of magnitude <= ~6
    assert err <= 32 * 2.0 ** -24 * max(1.0, np.abs(want).max()), err
    assert np.array_equal(got[:, (heads + kv_heads) * dh:], qkv[:, (heads + kv_heads) * dh:].astype(np.float64))   # V is copied


@pytest.mark.parametrize("H,woff", [(136, 0.0), (1024, 0.0), (1024, 1.0)])
def test_rmsnorm_reference_matches_transformers(H, woff):
    import torch
    from transformers.models.gemma.modeling_gemma import GemmaRMSNorm
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm
    rng = np.random.default_rng(H)
    x = (rng.standard_normal((9, H)) * np.array([1e-3, 1, 30, 1, 1, 1, 1, 1, 300])[:, None]).astype(np.float32)
    w = (0.2 * rng.standard_normal(H) + (0.0 if woff else 1.0)).astype(np.float32)
    mod = (GemmaRMSNorm if woff else Qwen3RMSNorm)(H, eps=1e-6)
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(w))
        want = mod(torch.from_numpy(x)).numpy()
    got = DC.rmsnorm_reference(x, w, woff, 1e-6)
    rel = np.abs(got - want) / np.maximum(np.abs(got), 1e-30)
    assert rel.max() <= (H / 8 + 8) * 2.0 ** -24, rel.max()     # torch sums the mean in fp32 (vectorised, a few partial sums)


@pytest.mark.parametrize("name,dh", [("random-96-s3", 64), ("random-288-s1", 128), ("random-160-s6", 256), ("random-packed-s1", 64)])
def test_attention_reference_matches_transformers_eager(name, dh):
    """eager_attention_forward with repeat_kv and an additive causal-plus-padding mask, fp32, sequence by sequence."""
    import torch
    from transformers.models.qwen3.modeling_qwen3 import eager_attention_forward
    case = DC.attention_case(name, dh)
    ref = DC.attention_reference(case)
    heads, kvh, qd, kd = case.heads, case.kv_heads, case.heads * dh, case.kv_heads * dh
    mod = types.SimpleNamespace(num_key_value_groups=heads // kvh, training=False)
    worst = 0.0
    for row0, T in case.sequences():
        blk = torch.from_numpy(case.qkv[row0:row0 + T].astype(np.float32))
        m = case.mask[row0:row0 + T] != 0
        q = blk[:, :qd].view(1, T, heads, dh).transpose(1, 2)
        k = blk[:, qd:qd + kd].view(1, T, kvh, dh).transpose(1, 2)
        v = blk[:, qd + kd:].view(1, T, kvh, dh).transpose(1, 2)
        vis = np.tril(np.ones((T, T), bool)) & m[None, :]
        add = torch.from_numpy(np.where(vis, 0.0, np.finfo(np.float32).min).astype(np.float32))[None, None]
        with torch.no_grad():
            out, _ = eager_attention_forward(mod, q, k, v, add, scaling=float(case.scale))
        got = out.reshape(T, qd).numpy()
        worst = max(worst, float(np.abs(got[m] - ref[row0:row0 + T][m]).max()))
    # fp32 scores: dh products of magnitude <= max|q| max|k| scale each, so exp() moves by that relative amount; twice for the sum
    q64 = np.abs(case.qkv[:, :qd].astype(np.float64)).max()
    k64 = np.abs(case.qkv[:, qd:qd + kd].astype(np.float64)).max()
    score_err = dh * 2.0 ** -24 * dh * q64 * k64 * float(case.scale)
    assert worst <= (2 * score_err + case.T * 2.0 ** -24) * case.vmax(), (worst, score_err)


def test_rsqrt_term_of_the_rmsnorm_bound():
    """The host's fp32 model of rsqrt (1 / sqrt(x), both correctly rounded) against float64 over 22 decades: within RSQRT_REL."""
    x = np.exp(np.random.default_rng(0).uniform(np.log(1e-12), np.log(1e10), 200000)).astype(np.float32)
    r32 = (np.float32(1.0) / np.sqrt(x)).astype(np.float64)
    r64 = 1.0 / np.sqrt(x.astype(np.float64))
    rel = float((np.abs(r32 - r64) / r64).max())
    print("fp32 1/sqrt relative error", rel, "bound", DC.RSQRT_REL)
    assert rel <= DC.RSQRT_REL


def test_last_token_index():
    m = np.array([[1, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 0]], np.int32)
    tok, all_last = DC.last_token_index(m.reshape(-1), 3, 4, 4)
    assert tok.tolist() == [2, 5, 8] and all_last == 0
    m = np.array([[0, 1, 1, 0], [1, 1, 1, 0]], np.int32)                 # left padding judged at t_valid = 3, not at t = 4
    tok, all_last = DC.last_token_index(m.reshape(-1), 2, 4, 3)
    assert tok.tolist() == [2, 6] and all_last == 1
    tok, all_last = DC.last_token_index(np.array([1, 1, 0, 1, 0, 0, 0], np.int32), 3, 4, 4, seq_off=np.array([0, 3, 5, 7]))
    assert tok.tolist() == [1, 3, 5] and all_last == 0


def test_activation_references():
    import torch
    x = DC.all_finite_fp16().astype(np.float64)
    t = torch.from_numpy(x)
    assert np.abs(DC.silu_reference(x) - torch.nn.functional.silu(t).numpy()).max() <= 1e-9 * 65504
    assert np.abs(DC.gelu_tanh_reference(x) - torch.nn.functional.gelu(t, approximate="tanh").numpy()).max() <= 1e-9 * 65504


# ---- the planted cases are what they claim to be -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", DC.HEAD_DIMS)
@pytest.mark.parametrize("name", PLANTED)
def test_planted_case_meets_its_conditions(name, dh):
    """On the inputs alone, in float64: the target's weight is >= 1 - 1e-6 and the output is V[j(i)] to 1e-9 max|v|; a reference that
    admits key i + 1, one that ignores the padding mask and one that maps head hd to kv head hd % kv_heads each move the output by more
    than 0.5 max|v| (where the case can tell them apart: a padded key in front of a valid query / a head whose two mappings differ).  The
    fp16-faithful model (q * scale rounded to fp16 as the kernel does) must land on V[j(i)] too, within the GPU test's bound."""
    case = DC.attention_case(name, dh)
    valid = DC.valid_rows(case)
    vmax = case.vmax()
    want = DC.planted_expected(case)
    ref, tw = DC.attention_reference(case, target_weight=True)
    assert np.all(case.target[valid] >= 0) and np.all(case.target[~valid] < 0)
    assert np.nanmin(tw[valid]) >= 1 - 1e-6, float(np.nanmin(tw[valid]))
    assert np.abs(ref[valid] - want[valid]).max() <= 1e-9 * vmax
    # the targets straddle the key tile: each of the five kinds occurs, and some target sits in an earlier tile than its query
    KT = DC.KEY_TILE[dh]
    rows = np.nonzero(valid)[0]
    if case.T > KT:
        seq0 = np.zeros(case.rows, np.int64)
        for row0, T in case.sequences():
            seq0[row0:row0 + T] = row0
        qt = (rows - seq0[rows]) // KT
        kt = (case.target[rows, 0] - seq0[rows]) // KT
        assert np.any(kt < qt) and np.any(kt == qt)
    moved = {}
    moved["causal+1"] = float(np.nanmax(np.abs(DC.attention_reference(case, causal_shift=1)[valid] - want[valid])))
    # (right padding alone is hidden from every valid query by the causal mask too: only a padded key in FRONT of a valid query tells)
    if any(np.any(case.mask[r0:r0 + int(np.nonzero(case.mask[r0:r0 + T])[0].max())] == 0) for r0, T in case.sequences()):
        moved["no-padding-mask"] = float(np.nanmax(np.abs(DC.attention_reference(case, ignore_mask=True)[valid] - want[valid])))
    group = case.heads // case.kv_heads
    if any(hd // group != hd % case.kv_heads for hd in range(case.heads)):
        moved["hd%kv_heads"] = float(np.nanmax(np.abs(DC.attention_reference(case, kv_map="mod")[valid] - want[valid])))
    print("planted", case.name, {k: round(v / vmax, 3) for k, v in moved.items()}, "min target weight", float(np.nanmin(tw[valid])))
    for k, v in moved.items():
        assert v > 0.5 * vmax, (k, v, vmax)
    model = DC.attention_model_fp16(case).astype(np.float64)
    assert np.abs(model[valid] - want[valid]).max() <= 2.0 ** -10 * vmax


def test_every_planted_case_set_covers_every_mutant():
    """No condition above is vacuous over the whole list: some case has padding, some has a mapping that hd % kv_heads changes."""
    specs = [s for s in DC.ATTENTION_CASES if s[1] == "planted"]
    assert any(s[4][0] != "packed" and any(p in ("left70", "left_all", "hole", "hole_late") for p in s[4]) for s in specs)
    assert any(any(hd // (h // kv) != hd % kv for hd in range(h)) for _, _, _, (h, kv), _, _ in specs)


# ---- the fp16-faithful model's error, per peaked-random case -------------------------------------------------------------------------
@pytest.mark.parametrize("dh", DC.HEAD_DIMS)
@pytest.mark.parametrize("name", RANDOM)
def test_fp16_model_error_is_the_recorded_one(name, dh):
    """max |model - float64| over the valid query rows, in units of max|v|: printed, and equal to decoder_cases.MODEL_ERR's entry up
    to the summation order of the host's BLAS (the GPU test doubles the RECORDED number, so it must not drift from what the model
    gives)."""
    case = DC.attention_case(name, dh)
    valid = DC.valid_rows(case)
    ref = DC.attention_reference(case)
    model = DC.attention_model_fp16(case).astype(np.float64)
    err = float(np.abs(model[valid] - ref[valid]).max() / case.vmax())
    print(f'    "{case.name}": {err:.3e},')
    assert case.name in DC.MODEL_ERR, f"record {case.name}: {err:.3e}"
    rec = DC.MODEL_ERR[case.name]
    assert 0.8 * rec <= err <= 1.25 * rec, (err, rec)
