"""The VAE's two ends without a GPU: the C ABI carries the new entries, the coefficient tables reproduce Pillow's default resize at every
size the device test uses, and the two arithmetic statements the kernels spell out (fp16(fp32(u) / 127.5f - 1) and the rounded steps of
_to_uint8_device) are what torch evaluates on the host.  Every comparison is for equality."""
import ctypes

import numpy as np
import pytest
import torch

import vae_ingest_ref as ref


def test_the_library_exports_and_binds_the_new_entries():
    from invertible_cd_amd import _lib
    lib = _lib.load()
    for name in ("icd_vae_ingest", "icd_image_to_u8"):
        assert name in _lib.SIGNATURES, f"{name} has no ctypes prototype"
        fn = getattr(lib, name)                                # AttributeError: the built library does not export it
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]


def test_bad_arguments_are_refused_before_anything_is_launched():
    """No GPU here: a call that got past its checks would fail with ICD_ERR_HIP, not ICD_ERR_INVALID_ARG."""
    from invertible_cd_amd import _lib, resample
    lib = _lib.load()
    invalid = -1                                               # ICD_ERR_INVALID_ARG
    assert lib.icd_vae_ingest(None, 1, 8, 8, 8, *([None, None, None, 5] * 2), None, None, None, None) == invalid
    buf = (ctypes.c_int32 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    k = resample.tap_width(16, 16)
    call = lambda B, H, W, S, ht, vt: lib.icd_vae_ingest(p, B, H, W, S, p, p, p, ht, p, p, p, vt, p, p, None, None)
    assert call(0, 16, 16, 16, k, k) == invalid                # B = 0
    assert call(1, 16, 16, 12, k, k) == invalid                # S not a multiple of 8
    assert b"multiple of 8" in lib.icd_last_error()
    assert call(1, 64, 16, 16, k, k) == invalid                # tables built for other sizes (64 -> 16 has wider rows)
    assert b"tables do not match" in lib.icd_last_error()
    assert lib.icd_image_to_u8(None, 0, 1, 8, 8, p, None) == invalid
    assert lib.icd_image_to_u8(p, 0, 0, 8, 8, p, None) == invalid
    assert lib.icd_image_to_u8(p, 1, 1, 8, 0, p, None) == invalid


@pytest.mark.parametrize("H,W,S", ref.SIZES)
def test_the_tables_reproduce_pillows_default_resize(H, W, S):
    from invertible_cd_amd import resample
    imgs = ref.images(3, H, W)
    want = ref.pil_resize(imgs, S)
    for b in range(3):
        assert np.array_equal(resample.resize_emulated(imgs[b], S, S), want[b])
    # the device kernels run a pass whose size does not change: its table is the identity
    assert np.array_equal(resample.resize_emulated(imgs[0], S, S, skip_identity=False), want[0])


def test_every_byte_through_the_spelled_out_ingest_arithmetic_is_torchs_host_route():
    u = np.arange(256, dtype=np.uint8)
    mine = (u.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).astype(np.float16)       # division, subtraction, ONE rounding
    host = ref.host_route(u.reshape(1, 16, 16, 1).repeat(3, axis=3)).to(torch.float16)[0, 0].flatten()
    assert np.array_equal(mine.view(np.uint16), host.numpy().view(np.uint16))
    assert mine[0] == -1.0 and mine[255] == 1.0


def test_the_rounded_steps_are_torchs_chain_on_every_fp16_value():
    x, want = ref.all_fp16_sample()
    assert want.shape == (1, 148, 144, 3) and torch.isinf(x).sum() >= 2
    assert torch.equal(ref.to_u8_torch(x), want)
    assert int(want.min()) == 0 and int(want.max()) == 255
    x32 = ref.fp32_sample(2, 37, 41, seed=5)
    assert torch.equal(ref.to_u8_torch(x32), ref.to_u8_steps(x32))
