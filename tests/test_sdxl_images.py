"""The SDXL image rules without a GPU: the numpy restatements of tests/sdxl_images_ref.py are what pipelines._ImageProcessor (diffusers'
VaeImageProcessor) evaluates on the host, the new arguments of the SDXL samplers refuse what they cannot take before any GPU work, and the
C ABI carries the two new entries.  Every comparison is for equality."""
import ctypes
import types

import numpy as np
import pytest
import torch

import sdxl_images_ref as ref
import stubs


# ------------------------------------------------------------------------------------------------ 1. the ingest rule
def test_every_byte_through_the_reference_is_preprocess_of_a_pil_image():
    from PIL import Image
    from invertible_cd_amd.pipelines import _ImageProcessor
    u = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    u[..., 1] = u[::-1, :, 1]                                  # the channels differ: a channel mix-up shows
    u[..., 2] = u[:, ::-1, 2]
    x = _ImageProcessor().preprocess(Image.fromarray(u))       # 16 x 16: no resize
    assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3, 16, 16)
    want = x[0].permute(1, 2, 0).numpy()
    got = ref.ingest_values(u)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0, 0, 0] == -1.0 and got[15, 15, 0] == 1.0


def test_the_split_halves_are_ops_definition_on_every_byte():
    """hi = fp16(v), lo = fp16(v - hi): ops.split_weight's expression (the host statement of the split operand) on torch tensors"""
    v = ref.ingest_values(np.arange(256, dtype=np.uint8))
    hi, lo = ref.split(v)
    t = torch.from_numpy(v)
    thi = t.to(torch.float16)
    tlo = (t - thi.float()).to(torch.float16)
    assert np.array_equal(hi.view(np.uint16), thi.numpy().view(np.uint16)) and np.array_equal(lo.view(np.uint16), tlo.numpy().view(np.uint16))
    assert np.count_nonzero(lo) > 128                          # fp32 values that fp16 cannot hold: the lo half carries something
    # hi + lo gives v back to within half an fp16 ulp of lo: the split loses less than 2^-22 on [-1, 1]
    assert float(np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v.astype(np.float64)).max()) < 2.0 ** -22
    op = ref.split3_operand(np.arange(192, dtype=np.uint8).reshape(1, 8, 8, 3))
    assert op.shape == (64, 24) and op.dtype == np.float16
    assert np.array_equal(op[:, 0:3], op[:, 16:19]) and not op[:, 3:8].any() and not op[:, 11:16].any() and not op[:, 19:24].any()
    assert np.array_equal(op[:, 0:3].reshape(-1).view(np.uint16), hi[:192].view(np.uint16))
    assert np.array_equal(op[:, 8:11].reshape(-1).view(np.uint16), lo[:192].view(np.uint16))


# ------------------------------------------------------------------------------------------------ 2. the output rule
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_the_reference_gives_the_bytes_of_postprocess_on_every_rounding_tie(dtype):
    from invertible_cd_amd.pipelines import _ImageProcessor
    ip = _ImageProcessor()
    samples = ref.tie_samples(dtype)
    assert all(s.shape == (2, 3, 3, 5) and s.dtype == np.dtype(dtype) for s in samples)
    flat = np.concatenate([s.reshape(-1) for s in samples])
    assert np.isinf(flat).sum() >= 2 and flat.min() < -1 and flat.max() > 1 and (flat == 0).sum() >= 2 and (np.abs(flat) == 1).sum() >= 2
    ties, seen = 0, set()
    for s in samples:
        pil = ip.postprocess(torch.from_numpy(s.copy()), output_type="pil")
        assert len(pil) == 2 and pil[0].size == (5, 3)          # PIL's (width, height)
        want = np.stack([np.array(im) for im in pil])
        got = ref.to_u8_round(s)
        assert got.dtype == np.uint8 and got.shape == (2, 3, 5, 3)
        assert np.array_equal(got, want)
        y = np.clip(s / s.dtype.type(2) + s.dtype.type(0.5), 0, 1).astype(np.float32) * np.float32(255)
        ties += int((y - np.floor(y) == 0.5).sum())
        seen.update(got.reshape(-1).tolist())
    assert seen == set(range(256))                             # both sides of every tie are there
    if dtype == "float32":
        assert ties >= 255                                     # the fp32 product lands exactly on k + 0.5: half to even decides
    # the rule differs from the SD1.5 one (truncation) on these values: the two entries are not interchangeable
    s = samples[0]
    trunc = (np.clip(s / s.dtype.type(2) + s.dtype.type(0.5), 0, 1).transpose(0, 2, 3, 1) * s.dtype.type(255)).astype(np.uint8)
    assert not np.array_equal(trunc, ref.to_u8_round(s))


def test_half_to_even_at_the_exact_ties():
    x = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, 127.5 / 255], dtype=np.float64) * 2 - 1
    x = np.resize(x.astype(np.float32), 90).reshape(ref.TIE_SHAPE)
    y = (x / np.float32(2) + np.float32(0.5)) * np.float32(255)
    got = ref.to_u8_round(x)[0, 0, :4, 0]                      # channel 0 of the first four pixels of row 0
    for g, v in zip(got, y[0, 0, 0, :4]):
        assert g == int(np.rint(v))
    assert ref.to_u8_round(np.full(ref.TIE_SHAPE, 0.0, np.float16))[0, 0, 0, 0] == 128      # 127.5 -> 128 (even)


# ------------------------------------------------------------------------------------------------ 3. argument handling (stub pipes)
def test_sample_deterministic_refuses_an_unknown_output_type_before_any_work():
    from invertible_cd_amd import generation_sdxl as X
    p = stubs.StubPipe()
    with pytest.raises(ValueError, match="output_type"):
        X.sample_deterministic(p, ["aa", "bb"], num_inference_steps=2, guidance_scale=7.0, is_sdxl=True,
                               compute_embeddings_fn=stubs.sdxl_emb_fn, output_type="bogus")
    assert p.unet.calls == []
    # the default and the explicit 'pil' are the same call, and the stub's postprocess sees the type that was asked for
    seen = []
    p.image_processor = types.SimpleNamespace(postprocess=lambda im, output_type, do_denormalize: (seen.append(output_type), im)[1])
    kw = dict(latents=torch.zeros(2, 4, 2, 2), num_inference_steps=2, guidance_scale=7.0, is_sdxl=True, compute_embeddings_fn=stubs.sdxl_emb_fn)
    X.sample_deterministic(p, ["aa", "bb"], **kw)
    X.sample_deterministic(p, ["aa", "bb"], output_type="uint8_device", **kw)
    assert seen == ["pil", "uint8_device"]


def _img2img_pipe():
    from invertible_cd_amd.pipelines import StableDiffusionXLImg2ImgPipeline
    calls = []
    vae = types.SimpleNamespace(to=lambda *a, **k: None, config=types.SimpleNamespace(scaling_factor=0.13025),
                                encode=lambda *a, **k: calls.append("encode"), encode_images=lambda *a, **k: calls.append("encode_images"))
    return StableDiffusionXLImg2ImgPipeline(stubs.StubUNet(), stubs.StubScheduler(), vae=vae, device="cpu"), calls


def test_prepare_latents_refuses_uint8_images_it_cannot_take():
    pipe, calls = _img2img_pipe()
    args = (torch.tensor([19]), 1, 1, torch.float32, "cpu")
    square = torch.zeros((1, 64, 64, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="on the device only"):
        pipe.prepare_latents(square, *args)
    with pytest.raises(ValueError, match="on the device only"):
        pipe.prepare_latents([square[0]], *args, resize_to=64)
    with pytest.raises(ValueError, match="square images of one size"):
        pipe.prepare_latents(torch.zeros((1, 40, 56, 3), dtype=torch.uint8), *args)
    with pytest.raises(ValueError, match="square images of one size"):
        pipe.prepare_latents([square[0], torch.zeros((32, 32, 3), dtype=torch.uint8)], *args)
    with pytest.raises(ValueError, match="multiple of 8"):
        pipe.prepare_latents(square, *args, resize_to=60)
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        pipe.prepare_latents(torch.zeros((1, 3, 64, 64), dtype=torch.uint8), *args)
    with pytest.raises(ValueError, match="resize_to applies to uint8"):
        pipe.prepare_latents(torch.zeros((1, 3, 64, 64)), *args, resize_to=64)
    assert calls == []                                         # nothing reached the VAE


def test_inverse_sample_deterministic_passes_resize_to_through():
    from invertible_cd_amd import generation_sdxl as X
    p = stubs.StubPipe()
    seen = []
    orig = p.prepare_latents
    p.prepare_latents = lambda *a, **k: (seen.append(k.get("resize_to", "absent")), orig(*a, **k))[1]
    kw = dict(num_inference_steps=2, guidance_scale=0.0, is_sdxl=True, compute_embeddings_fn=stubs.sdxl_emb_fn)
    X.inverse_sample_deterministic(p, torch.zeros(2, 4, 2, 2), ["aa", "bb"], **kw)
    X.inverse_sample_deterministic(p, torch.zeros(2, 4, 2, 2), ["aa", "bb"], resize_to=1024, **kw)
    assert seen == ["absent", 1024]                            # the default call is the call it has always been


def test_encode_images_image_processor_rule_needs_the_fp32_mode():
    from invertible_cd_amd import synthetic, vae
    cfg = vae.SDXL_VAE.scaled((32, 64, 64, 64))
    m = vae.AutoencoderKL(cfg, synthetic.synthetic_vae_state_dict(cfg, seed=3), device="cpu")
    assert m.dtype == torch.float16
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="fp32-fidelity"):
        m.encode_images(img, 8, rule="image_processor")
    with pytest.raises(ValueError, match="rule must be"):
        m.to(torch.float32).encode_images(img, 8, rule="load_1024")


def test_postprocess_uint8_device_refuses_a_host_tensor():
    from invertible_cd_amd.pipelines import _ImageProcessor
    with pytest.raises(ValueError, match="on the device"):
        _ImageProcessor().postprocess(torch.zeros(1, 3, 8, 8), output_type="uint8_device")


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def test_the_library_exports_and_binds_the_two_entries():
    from invertible_cd_amd import _lib
    lib = _lib.load()
    for name in ("icd_vae_ingest_f32", "icd_image_to_u8_round"):
        assert name in _lib.SIGNATURES, f"{name} has no ctypes prototype"
        fn = getattr(lib, name)                                # AttributeError: the built library does not export it
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["icd_vae_ingest_f32"] == _lib.SIGNATURES["icd_vae_ingest"]          # the same table arguments
    assert _lib.SIGNATURES["icd_image_to_u8_round"] == _lib.SIGNATURES["icd_image_to_u8"]


def test_bad_arguments_are_refused_before_anything_is_launched():
    """No GPU here: a call that got past its checks would fail with ICD_ERR_HIP, not ICD_ERR_INVALID_ARG."""
    from invertible_cd_amd import _lib, resample
    lib = _lib.load()
    invalid = -1                                               # ICD_ERR_INVALID_ARG
    assert lib.icd_vae_ingest_f32(None, 1, 8, 8, 8, *([None, None, None, 5] * 2), None, None, None, None) == invalid
    buf = (ctypes.c_int32 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    k = resample.tap_width(16, 16)
    call = lambda B, H, W, S, ht, vt: lib.icd_vae_ingest_f32(p, B, H, W, S, p, p, p, ht, p, p, p, vt, p, p, None, None)
    assert call(0, 16, 16, 16, k, k) == invalid                # B = 0
    assert call(1, 16, 16, 12, k, k) == invalid                # S not a multiple of 8
    assert b"icd_vae_ingest_f32" in lib.icd_last_error() and b"multiple of 8" in lib.icd_last_error()
    assert call(1, 64, 16, 16, k, k) == invalid                # tables built for other sizes (64 -> 16 has wider rows)
    assert b"tables do not match" in lib.icd_last_error()
    assert call(1, 16, 5000, 16, k, k) == invalid              # W > 4096
    assert lib.icd_image_to_u8_round(None, 0, 1, 8, 8, p, None) == invalid
    assert b"icd_image_to_u8_round" in lib.icd_last_error()
    assert lib.icd_image_to_u8_round(p, 0, 0, 8, 8, p, None) == invalid
    assert lib.icd_image_to_u8_round(p, 1, 1, 8, 0, p, None) == invalid
