"""SDXL edits on the device: uint8 images into the fp32-fidelity VAE encoder (icd_vae_ingest_f32) and uint8 images out of the sampler
(icd_image_to_u8_round), against the host route - Pillow's resize, pipelines._ImageProcessor (diffusers' VaeImageProcessor), vae._pack32
- and its numpy restatement (tests/sdxl_images_ref.py).

Bars.  Every comparison is for equality: the resample is integer arithmetic, the ingest value is a division, a doubling and a subtraction
in fp32 followed by the split's two roundings, the output kernel makes torch's and numpy's roundings one by one, and the encoder sees the
same operand bits on both routes."""
import ctypes

import numpy as np
import pytest
import torch

import sdxl_images_ref as ref

pytestmark = pytest.mark.gpu

INVALID = -1                                                   # ICD_ERR_INVALID_ARG
POISON = 0x7B7B                                                # fp16 bit pattern the outputs are filled with before a call


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ingest_cabi(dev, S, want_bytes):
    """icd_vae_ingest_f32 through ctypes -> (status, out [B * S * S, 24] fp16, the byte buffer [B, S, S, 3]), both poisoned before"""
    from invertible_cd_amd import _lib, ops
    B, H, W = dev.shape[:3]
    tmp = torch.empty((B * H, S, 3), device="cuda", dtype=torch.uint8)
    out = torch.full((B * S * S, 24), POISON, device="cuda", dtype=torch.int16).view(torch.float16)
    byt = torch.full((B, S, S, 3), 0xA5, device="cuda", dtype=torch.uint8)
    rc = _lib.load().icd_vae_ingest_f32(_vp(dev), B, H, W, S, *ops._table_args(W, S, H, S, dev.device), _vp(tmp), _vp(out),
                                        _vp(byt) if want_bytes else None, _stream())
    torch.cuda.synchronize()
    return rc, out, byt


def _host_operand(resized_u8):
    """Pillow's bytes -> _ImageProcessor.preprocess -> vae._pack32: the first operand of the fp32-fidelity encoder, host route"""
    from PIL import Image
    from invertible_cd_amd import vae
    from invertible_cd_amd.pipelines import _ImageProcessor
    x = _ImageProcessor().preprocess([Image.fromarray(a) for a in resized_u8])
    assert x.dtype == torch.float32 and tuple(x.shape) == (resized_u8.shape[0], 3) + resized_u8.shape[1:3]
    return vae._pack32(x, torch.device("cuda"))


def _all_values_image():
    u = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    u[..., 1] = u[::-1, :, 1]
    u[..., 2] = u[:, ::-1, 2]
    return u[None].copy()


INGEST_CASES = {
    "down_20x12_to_8": lambda: (ref.images(1, 20, 12), 8),              # 20 -> 8 and 12 -> 8: the tap count differs per axis
    "up_5x7_to_16": lambda: (ref.images(1, 5, 7), 16),
    "identity_8x8": lambda: (ref.images(3, 8, 8), 8),
    "all_256_values": lambda: (_all_values_image(), 16),
    "odd_byte_slice_b2": lambda: (ref.images(2, 20, 12, seed=5), 8),
}


# ------------------------------------------------------------------------------------------------ 1. icd_vae_ingest_f32
@pytest.mark.parametrize("case", list(INGEST_CASES))
def test_ingest_f32_equals_pillow_preprocess_and_pack32_bit_for_bit(case):
    from invertible_cd_amd import ops
    imgs, S = INGEST_CASES[case]()
    B, H, W = imgs.shape[:3]
    if case == "odd_byte_slice_b2":                            # B = 2 as a slice of a larger buffer, starting at an odd byte
        flat = torch.zeros(3 + imgs.size + 5, dtype=torch.uint8, device="cuda")
        flat[3:3 + imgs.size] = torch.from_numpy(imgs).cuda().flatten()
        dev = flat[3:3 + imgs.size].view(B, H, W, 3)
        assert dev.data_ptr() % 2 == 1
    else:
        dev = torch.from_numpy(imgs).cuda()
    want_u8 = ref.pil_resize(imgs, S)
    if H == S and W == S:
        assert np.array_equal(want_u8, imgs)                    # identity taps: the input bytes
    want = _host_operand(want_u8)
    assert tuple(want.shape) == (B * S * S, 24) and want.dtype == torch.float16
    assert np.array_equal(want.cpu().numpy().view(np.uint16), ref.split3_operand(want_u8).view(np.uint16))      # the restatement agrees
    rc, out, byt = _ingest_cabi(dev, S, True)
    assert rc == 0
    diff = int((byt.cpu() != torch.from_numpy(want_u8)).sum())
    assert diff == 0, f"{diff} resized bytes differ from Pillow"
    diff = int((out.view(torch.int16) != want.view(torch.int16)).sum())
    assert diff == 0, f"{diff} operand halves differ from split_cast(_pack32(preprocess(...)))"
    pads = torch.cat([out[:, 3:8], out[:, 11:16], out[:, 19:24]], dim=1).view(torch.int16)
    assert int(pads.count_nonzero()) == 0                      # the pad columns of [hi | lo | hi]: +0 although `out` was poisoned
    if case == "all_256_values":
        assert torch.equal(byt.cpu(), torch.from_numpy(imgs)) and sorted(set(byt.cpu().flatten().tolist())) == list(range(256))
    rc, out2, byt2 = _ingest_cabi(dev, S, False)                # bytes = NULL: the same operand, the byte buffer left alone
    assert rc == 0 and torch.equal(out2.view(torch.int16), want.view(torch.int16)) and int((byt2 != 0xA5).sum()) == 0
    o3, b3 = ops.vae_ingest_f32(dev, S, want_bytes=True)        # the operator wrapper is the same call
    assert torch.equal(o3.view(torch.int16), want.view(torch.int16)) and torch.equal(b3, byt) and ops.vae_ingest_f32(dev, S)[1] is None


# ------------------------------------------------------------------------------------------------ 2. icd_image_to_u8_round
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_image_to_u8_round_equals_the_cpu_reference_on_every_rounding_tie(dtype):
    from invertible_cd_amd import _lib, ops
    from invertible_cd_amd.pipelines import _ImageProcessor
    wrong = 0
    for s in ref.tie_samples(dtype):
        dev = torch.from_numpy(s.copy()).cuda()
        got = ops.image_to_u8_round(dev)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, 5, 3)
        wrong += int((got.cpu().numpy() != ref.to_u8_round(s)).sum())
        assert torch.equal(_ImageProcessor().postprocess(dev, output_type="uint8_device"), got)
    assert wrong == 0, f"{wrong} bytes differ from postprocess's"
    # nothing past the last pixel is written (30 pixels, 90 bytes: the last thread stores bytes)
    s = ref.tie_samples(dtype)[0]
    dev = torch.from_numpy(s.copy()).cuda()
    pad = torch.full((90 + 64,), 0xA5, device="cuda", dtype=torch.uint8)
    rc = _lib.load().icd_image_to_u8_round(_vp(dev), int(dtype == "float32"), 2, 3, 5, _vp(pad), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(pad[:90].cpu().numpy().reshape(2, 3, 5, 3), ref.to_u8_round(s)) and bool((pad[90:] == 0xA5).all())


# ------------------------------------------------------------------------------------------------ 3. refused arguments
def test_refused_arguments_leave_the_poisoned_outputs_untouched():
    from invertible_cd_amd import _lib, ops
    lib = _lib.load()
    dev = torch.from_numpy(ref.images(1, 24, 40)).cuda()

    def call(S, tables, images=dev, null_out=False):
        tmp = torch.full((24 * 64 * 3,), 0x5A, device="cuda", dtype=torch.uint8)
        out = torch.full((64 * 64, 24), POISON, device="cuda", dtype=torch.int16)
        byt = torch.full((64 * 64 * 3,), 0xA5, device="cuda", dtype=torch.uint8)
        rc = lib.icd_vae_ingest_f32(None if images is None else _vp(images), 1, 24, 40, S, *tables, _vp(tmp), None if null_out else _vp(out),
                                    _vp(byt), _stream())
        torch.cuda.synchronize()
        assert bool((tmp == 0x5A).all()) and bool((out == POISON).all()) and bool((byt == 0xA5).all()), "a refused call wrote something"
        return rc

    good = ops._table_args(40, 32, 24, 32, dev.device)
    assert call(36, ops._table_args(40, 36, 24, 36, dev.device)) == INVALID      # S not a multiple of 8
    assert call(32, ops._table_args(40, 64, 24, 64, dev.device)) == INVALID      # tables built for 64, S = 32: other row lengths
    assert call(32, ops._table_args(80, 32, 24, 32, dev.device)) == INVALID      # tables built for another width
    assert call(32, good, images=None) == INVALID                                # null pointers
    assert call(32, good, null_out=True) == INVALID
    assert call(32, (None,) + tuple(good[1:])) == INVALID
    x = torch.zeros((1, 3, 3, 5), device="cuda")
    out = torch.full((64,), 0xA5, device="cuda", dtype=torch.uint8)
    assert lib.icd_image_to_u8_round(None, 1, 1, 3, 5, _vp(out), _stream()) == INVALID
    assert lib.icd_image_to_u8_round(_vp(x), 1, 1, 3, 5, None, _stream()) == INVALID
    assert lib.icd_image_to_u8_round(_vp(x), 1, 0, 3, 5, _vp(out), _stream()) == INVALID
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


# ------------------------------------------------------------------------------------------------ 4, 5. end to end (reduced width)
@pytest.fixture(scope="module")
def sdxl_small():
    """Reduced-width synthetic SDXL UNet and VAE on one img2img pipeline; 64 x 64 images, 8 x 8 latents, two prompts"""
    from invertible_cd_amd import synthetic, unet, vae
    from invertible_cd_amd.pipelines import StableDiffusionXLImg2ImgPipeline
    from invertible_cd_amd.schedulers import DDIMScheduler
    from invertible_cd_amd.unet_config import SDXL
    cfg = SDXL.scaled((64, 128, 256), cross_dim=128, heads=(2, 4, 8))
    u = unet.UNet2DConditionModel(cfg, synthetic.synthetic_state_dict(cfg, seed=4), dtype=torch.float16)
    vcfg = vae.SDXL_VAE.scaled((32, 64, 64, 64))
    v = vae.AutoencoderKL(vcfg, synthetic.synthetic_vae_state_dict(vcfg, seed=3))
    pipe = StableDiffusionXLImg2ImgPipeline(u, DDIMScheduler.sdxl(), vae=v)
    inp = synthetic.synthetic_inputs(cfg, 2, 8, 8, seed=9)
    emb = lambda p, o, c: {"prompt_embeds": inp["context"].cuda().half(), "text_embeds": inp["text_embeds"].cuda().half(),
                           "time_ids": inp["time_ids"].cuda()}
    return pipe, v, emb


def test_inversion_and_edit_from_device_images_equal_the_host_route(sdxl_small):
    from PIL import Image
    from invertible_cd_amd import generation_sdxl as G
    from invertible_cd_amd import metrics
    pipe, v, emb = sdxl_small
    S = 64
    src = ref.images(2, 40, 56)
    resized = ref.pil_resize(src, S)
    pils = [Image.fromarray(a) for a in resized]
    kw = dict(num_inference_steps=3, timesteps=[19, 339, 699], guidance_scale=0.0, is_sdxl=True, compute_embeddings_fn=emb, seed=5,
              return_start_latent=True)
    lat_h, start_h = G.inverse_sample_deterministic(pipe, pils, ["a", "b"], **kw)
    lat_d, start_d = G.inverse_sample_deterministic(pipe, torch.from_numpy(src).cuda(), ["a", "b"], resize_to=S, **kw)
    assert tuple(start_d.shape) == (2, 4, 8, 8) and start_d.dtype == torch.float16 and bool(torch.isfinite(lat_d).all())
    assert torch.equal(start_d, start_h) and torch.equal(lat_d, lat_h)
    assert float(start_d.float().std()) > 0 and not torch.equal(start_d[0], start_d[1])
    # images already at their size: resize_to=None is the same call
    lat_n, start_n = G.inverse_sample_deterministic(pipe, torch.from_numpy(resized).cuda(), ["a", "b"], **kw)
    assert torch.equal(start_n, start_h) and torch.equal(lat_n, lat_h)
    # the way back: the bytes of the PIL images, left on the device
    rkw = dict(latents=lat_d, num_inference_steps=3, timesteps=[339, 699, 999], guidance_scale=7.0, is_sdxl=True, compute_embeddings_fn=emb)
    pil_out = G.sample_deterministic(pipe, ["a", "b"], **rkw)
    dev_out = G.sample_deterministic(pipe, ["a", "b"], output_type="uint8_device", **rkw)
    host = np.stack([np.array(im) for im in pil_out])
    assert dev_out.is_cuda and dev_out.dtype == torch.uint8 and tuple(dev_out.shape) == (2, S, S, 3)
    assert np.array_equal(dev_out.cpu().numpy(), host)
    assert host.std() > 0 and not np.array_equal(host[0], host[1])
    # metrics.py takes the tensor as it is
    got = metrics.calculate_psnr(dev_out, torch.from_numpy(resized).cuda(), "cuda")
    want = metrics.calculate_psnr([a for a in host], [a for a in resized], "cuda")
    assert got == want and len(got) == 2 and all(np.isfinite(g) for g in got)


def test_a_list_of_two_sizes_equals_each_image_alone_and_the_host_batch(sdxl_small):
    from PIL import Image
    pipe, v, emb = sdxl_small
    S = 64
    a, b = ref.images(1, 40, 56, seed=1), ref.images(1, 72, 64, seed=2)
    both = [torch.from_numpy(a[0]).cuda(), torch.from_numpy(b).cuda()]           # [H, W, 3] and [1, H, W, 3]
    resized = np.concatenate([ref.pil_resize(a, S), ref.pil_resize(b, S)])
    chunk = v.max_chunk
    v.to(torch.float32)
    try:
        out = v.encode_images(both, S, want_bytes=True, rule="image_processor")
        d = out["latent_dist"]
        assert tuple(d.mean.shape) == (2, 4, 8, 8) and d.mean.dtype == torch.float32
        assert torch.equal(out["images"].cpu(), torch.from_numpy(resized))
        assert "images" not in v.encode_images(both, S, rule="image_processor")
        host = v.encode(pipe.image_processor.preprocess([Image.fromarray(r) for r in resized]))["latent_dist"]
        assert torch.equal(d.mean, host.mean) and torch.equal(d.logvar, host.logvar)
        # a pipeline that runs in fp16 rounds the image to fp16 in front of the upcast (prepare_latents): image_dtype says so
        x16 = pipe.image_processor.preprocess([Image.fromarray(r) for r in resized]).half().float()
        host16, d16 = v.encode(x16)["latent_dist"], v.encode_images(both, S, rule="image_processor", image_dtype=torch.float16)["latent_dist"]
        assert torch.equal(d16.mean, host16.mean) and torch.equal(d16.logvar, host16.logvar) and not torch.equal(d16.mean, d.mean)
        v.max_chunk = 1                                         # one image per encoder pass, in a list or alone: the same launches
        d1 = v.encode_images(both, S, rule="image_processor")["latent_dist"]
        for i, one in enumerate(both):
            alone = v.encode_images(one, S, rule="image_processor")["latent_dist"]
            assert torch.equal(d1.mean[i:i + 1], alone.mean) and torch.equal(d1.logvar[i:i + 1], alone.logvar)
        assert not torch.equal(d1.mean[0], d1.mean[1])
    finally:
        v.max_chunk = chunk
        v.to(torch.float16)
    # through the pipeline: the list against the host route on the resized PIL images, both draws from one generator
    args = (torch.tensor([19]), 2, 1, torch.float16, "cuda")
    got = pipe.prepare_latents(both, *args, generator=torch.Generator().manual_seed(7), resize_to=S)
    want = pipe.prepare_latents([Image.fromarray(r) for r in resized], *args, generator=torch.Generator().manual_seed(7))
    assert got.dtype == torch.float16 and tuple(got.shape) == (2, 4, 8, 8) and torch.equal(got, want)
    with pytest.raises(ValueError, match="square images of one size"):
        pipe.prepare_latents(both, *args)
