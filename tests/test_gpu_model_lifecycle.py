"""The life of a model handle (encoder, decoder, vision tower, CLIP text tower), which the four share (ModelBase, DevPool and
model_upload / model_release in csrc/vf_transformer.hip): create, a workspace that grows, forwards that do not depend on the growth,
close -- and the caller's current device, which no entry point may leave changed (DeviceGuard, csrc/vf_internal.h).

Every handle has the smallest configuration its create accepts, with seeded random weights: nothing here is compared with a
reference model (tests/test_gpu_encoder.py, test_vision.py and test_pretrained.py do that), only a handle with itself."""
import ctypes
import threading

import numpy as np
import pytest

KINDS = ("encoder", "decoder", "vit", "clip_text")


def _blobs(n16, n32, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 0.05, n16).astype(np.float16), rng.normal(0.5, 0.2, n32).astype(np.float32)


def _sizes(fn, cfg_struct):
    from veritasfi_amd import _ffi
    n16, n32 = _ffi.c_i64(0), _ffi.c_i64(0)
    _ffi.check(fn(ctypes.byref(cfg_struct), ctypes.byref(n16), ctypes.byref(n32)), "weight_sizes")
    return n16.value, n32.value


def _open(kind, device_id=0):
    """(handle, forward) of the smallest legal model of `kind`; forward(b) runs the seeded batch of b rows."""
    from veritasfi_amd import _ffi
    from veritasfi_amd.encoder import HipDecoder, HipEncoder
    from veritasfi_amd.vision import HipClipTextEncoder, HipVisionEncoder
    L = _ffi.lib()
    rng = np.random.default_rng(7)
    if kind == "encoder":
        cfg = dict(vocab=100, hidden=128, layers=1, heads=2, ffn=256, max_pos=64, type_vocab=2, roberta_pad_idx=-1, pooling=0,
                   normalize=1, head=0, ln_eps=1e-5)
        h = HipEncoder(cfg, *_blobs(*_sizes(L.vf_encoder_weight_sizes, _ffi.EncoderConfig(**cfg)), seed=1), device_id=device_id)
        ids = rng.integers(0, 100, (5, 32))
        mask = np.ones((5, 32), np.int32)
        mask[1, 20:] = 0
        return h, lambda b: h.forward(ids[:b], mask[:b])
    if kind == "decoder":
        cfg = dict(vocab=100, hidden=128, layers=1, heads=2, kv_heads=1, head_dim=64, ffn=128, rope_theta=10000.0, rms_eps=1e-6,
                   qk_norm=1, pooling=2, normalize=0, head=0, act=0, norm_plus_one=0, embed_scale=1.0)
        h = HipDecoder(cfg, *_blobs(*_sizes(L.vf_decoder_weight_sizes, _ffi.DecoderConfig(**cfg)), seed=2), device_id=device_id)
        ids = rng.integers(0, 100, (5, 32))
        mask = np.ones((5, 32), np.int32)
        mask[1, 20:] = 0
        return h, lambda b: h.forward(ids[:b], mask[:b])
    if kind == "vit":
        cfg = dict(image=32, patch=8, channels=3, hidden=128, layers=1, heads=2, ffn=256, proj_dim=64, act=1, normalize=0, ln_eps=1e-5)
        h = HipVisionEncoder(cfg, *_blobs(*_sizes(L.vf_vit_weight_sizes, _ffi.VitConfig(**cfg)), seed=3), device_id=device_id)
        px = rng.standard_normal((5, 3, 32, 32)).astype(np.float32)
        return h, lambda b: h.forward(px[:b])
    assert kind == "clip_text"
    cfg = dict(vocab=100, max_pos=40, hidden=128, layers=1, heads=2, ffn=256, proj_dim=64, act=1, eos_token_id=2, normalize=0, ln_eps=1e-5)
    h = HipClipTextEncoder(cfg, *_blobs(*_sizes(L.vf_clip_text_weight_sizes, _ffi.ClipTextConfig(**cfg)), seed=4), device_id=device_id)
    ids = rng.integers(0, 100, (5, 40))
    return h, lambda b: h.forward(ids[:b])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_workspace_regrowth_leaves_the_forward_unchanged(kind):
    """A batch of 2, a batch of 5 (more sequences than the workspace holds: it is freed and grown), the batch of 2 again: same
    shapes, same kernels, so the same bits.  Then close: a forward on the closed handle raises."""
    h, forward = _open(kind)
    try:
        first = forward(2).copy()
        grown = forward(5).copy()
        again = forward(2).copy()
    finally:
        h.close()
    assert first.shape[0] == 2 and grown.shape[0] == 5
    assert np.isfinite(grown).all()
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), float(np.abs(first - again).max())
    with pytest.raises(RuntimeError):
        forward(2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_create_and_close_without_a_forward(kind):
    """Twenty handles opened and closed unused: the release meets no stream and an empty workspace pool."""
    for _ in range(20):
        h, _forward = _open(kind)
        h.close()
    h, forward = _open(kind)   # ... and the device is still good for a forward afterwards
    try:
        assert np.isfinite(forward(2)).all()
    finally:
        h.close()


def _hip_runtime():
    """The HIP runtime object the library is bound to: the one libamdhip64 mapped into this process once the library is loaded
    (PyTorch-ROCm ships a copy with the system's SONAME; _ffi.lib() loads torch first so that both bind to it).  Opening that very
    file again hands back the same object, so hipGetDevice / hipSetDevice here read and write the per-thread state the library sees."""
    from veritasfi_amd import _ffi
    _ffi.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert len(paths) == 1, f"expected one HIP runtime in the process, found {paths}"
    rt = ctypes.CDLL(paths[0])
    rt.hipGetDevice.argtypes, rt.hipGetDevice.restype = [ctypes.POINTER(ctypes.c_int)], ctypes.c_int
    rt.hipSetDevice.argtypes, rt.hipSetDevice.restype = [ctypes.c_int], ctypes.c_int
    rt.hipGetDeviceCount.argtypes, rt.hipGetDeviceCount.restype = [ctypes.POINTER(ctypes.c_int)], ctypes.c_int
    return rt


@pytest.mark.gpu
def test_entry_points_leave_the_callers_device_alone():
    """From a thread whose current device is 1: create, forward and destroy each kind of handle on device 0.  After every call the
    thread's current device is still 1 (hipSetDevice is per-thread state: the rule of csrc/vf_internal.h)."""
    rt = _hip_runtime()
    n = ctypes.c_int(0)
    assert rt.hipGetDeviceCount(ctypes.byref(n)) == 0
    if n.value < 2:
        pytest.skip("needs two visible devices")
    seen, errors = [], []

    def current():
        d = ctypes.c_int(-1)
        assert rt.hipGetDevice(ctypes.byref(d)) == 0
        return d.value

    def body():
        try:
            assert rt.hipSetDevice(1) == 0 and current() == 1
            for kind in KINDS:
                h, forward = _open(kind, device_id=0)
                seen.append((kind, "create", current()))
                out = forward(2)
                seen.append((kind, "forward", current()))
                h.close()
                seen.append((kind, "destroy", current()))
                assert np.isfinite(out).all()
        except BaseException as e:  # noqa: BLE001 -- handed to the test's thread
            errors.append(e)

    t = threading.Thread(target=body)
    t.start()
    t.join()
    assert not errors, errors
    print(seen)
    assert len(seen) == 3 * len(KINDS)
    moved = [s for s in seen if s[2] != 1]
    assert not moved, moved
