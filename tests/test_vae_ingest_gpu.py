"""Real images into the VAE and uint8 images out of it, on the device, against the host route (tests/vae_ingest_ref.py): Pillow's resize,
image2latent's `float() / 127.5 - 1`, `encode`, and the torch expression of _to_uint8_device.

Bars.  Every comparison is for equality: the resample is integer arithmetic, the ingest value is one division, one subtraction and one
rounding to fp16, the output kernel makes torch's roundings one by one, and the encoder sees the same bits on both routes."""
import ctypes

import numpy as np
import pytest
import torch

import vae_ingest_ref as ref

pytestmark = pytest.mark.gpu

INVALID = -1                                                   # ICD_ERR_INVALID_ARG


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _ingest_cabi(dev, S, want_bytes, sentinel=0xA5):
    """icd_vae_ingest through ctypes -> (status, out [B * S * S, 8] fp16, the byte buffer [B, S, S, 3], pre-filled with `sentinel`)"""
    from invertible_cd_amd import _lib, ops
    B, H, W = dev.shape[:3]
    tmp = torch.empty((B * H, S, 3), device="cuda", dtype=torch.uint8)
    out = torch.full((B * S * S, 8), 7.0, device="cuda", dtype=torch.float16)
    byt = torch.full((B, S, S, 3), sentinel, device="cuda", dtype=torch.uint8)
    rc = _lib.load().icd_vae_ingest(_vp(dev), B, H, W, S, *ops._table_args(W, S, H, S, dev.device), _vp(tmp), _vp(out),
                                    _vp(byt) if want_bytes else None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out, byt


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W,S", ref.SIZES)
def test_ingest_equals_pillow_and_the_host_routes_encoder_tensor_bit_for_bit(H, W, S, B):
    """B = 3 carries a constant-255 and a constant-0 image (clip8 at both ends); 17 x 23 at B = 3 is a batch slice that starts at an odd
    byte.  The byte-less call must leave a sentinel-filled buffer alone and give the same encoder tensor."""
    from invertible_cd_amd import ops
    imgs = ref.images(B, H, W)
    if (H, W, B) == (17, 23, 3):
        flat = torch.zeros(1 + imgs.size, dtype=torch.uint8, device="cuda")
        flat[1:] = torch.from_numpy(imgs).cuda().flatten()
        dev = flat[1:].view(B, H, W, 3)
        assert dev.data_ptr() % 2 == 1
    else:
        dev = torch.from_numpy(imgs).cuda()
    want_u8 = ref.pil_resize(imgs, S)
    if H == S and W == S:
        assert np.array_equal(want_u8, imgs)                    # identity taps: the input bytes
    want_x = ops.pack_nchw(ref.host_route(want_u8).to("cuda", dtype=torch.float16).contiguous())
    rc, out, byt = _ingest_cabi(dev, S, True)
    assert rc == 0
    diff = int((byt.cpu() != torch.from_numpy(want_u8)).sum())
    assert diff == 0, f"{diff} resized bytes differ from Pillow"
    assert torch.equal(out.view(torch.int16), want_x.view(torch.int16))
    assert int(out[:, 3:].view(torch.int16).count_nonzero()) == 0       # pad channels: +0, not -0
    rc, out2, byt2 = _ingest_cabi(dev, S, False)
    assert rc == 0 and torch.equal(out2.view(torch.int16), want_x.view(torch.int16))
    assert int((byt2 != 0xA5).sum()) == 0
    if B == 3:                                                 # the operator wrapper is the same call
        o3, b3 = ops.vae_ingest(dev, S, want_bytes=True)
        assert torch.equal(o3, out) and torch.equal(b3, byt) and ops.vae_ingest(dev, S)[1] is None


def test_ingest_refuses_bad_arguments_and_launches_nothing():
    from invertible_cd_amd import _lib, ops
    lib = _lib.load()
    dev = torch.from_numpy(ref.images(1, 24, 40)).cuda()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(B, S, tables):
        tmp = torch.full((24 * 64 * 3,), 0x5A, device="cuda", dtype=torch.uint8)
        out = torch.full((64 * 64, 8), 7.0, device="cuda", dtype=torch.float16)
        byt = torch.full((64 * 64 * 3,), 0xA5, device="cuda", dtype=torch.uint8)
        rc = lib.icd_vae_ingest(_vp(dev), B, 24, 40, S, *tables, _vp(tmp), _vp(out), _vp(byt), st)
        torch.cuda.synchronize()
        assert bool((tmp == 0x5A).all()) and bool((out == 7.0).all()) and bool((byt == 0xA5).all()), "a refused call wrote something"
        return rc

    good = ops._table_args(40, 32, 24, 32, dev.device)
    assert call(1, 36, ops._table_args(40, 36, 24, 36, dev.device)) == INVALID      # S not a multiple of 8
    assert call(1, 32, ops._table_args(40, 64, 24, 64, dev.device)) == INVALID      # tables built for 64, S = 32: other row lengths
    assert call(1, 32, ops._table_args(80, 32, 24, 32, dev.device)) == INVALID      # tables built for another width
    assert call(0, 32, good) == INVALID
    assert lib.icd_image_to_u8(_vp(dev), 0, 0, 24, 40, _vp(dev), st) == INVALID


# ------------------------------------------------------------------------------------------------ image_to_u8
def test_image_to_u8_on_every_fp16_value_is_the_rounded_chain_and_torchs_expression():
    from invertible_cd_amd import ops
    x, want = ref.all_fp16_sample()
    dev = x.cuda()
    got = ops.image_to_u8(dev)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 148, 144, 3)
    diff = int((got.cpu() != want).sum())
    assert diff == 0, f"{diff} bytes differ from the CPU restatement"
    assert torch.equal(got, ref.to_u8_torch(dev))


@pytest.mark.parametrize("B,H,W", [(1, 3, 5), (2, 3, 5), (2, 37, 41), (1, 64, 64)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_image_to_u8_equals_the_torch_expression_at_odd_shapes(B, H, W, dtype):
    """3 x 5: fewer pixels than a block and H W % 4 != 0 (a thread's four pixels straddle two samples at B = 2, the last thread stores
    bytes); 37 x 41: several blocks, a ragged last one.  The fp32 values hold +-1, 0 and k / 127.5 - 1 for the bytes k that fit."""
    from invertible_cd_amd import generation, ops
    x = ref.fp32_sample(B, H, W, seed=H * W + B).to(dtype)
    dev = x.cuda()
    pad = torch.full((B * H * W * 3 + 64,), 0xA5, device="cuda", dtype=torch.uint8)          # nothing past the last pixel is written
    got = ops.image_to_u8(dev)
    want = ref.to_u8_torch(dev)
    assert torch.equal(got, want)
    assert torch.equal(got.cpu(), ref.to_u8_steps(x))
    assert torch.equal(generation._to_uint8_device(dev), want)
    assert torch.equal(generation._to_uint8_device(dev.permute(0, 1, 3, 2)), ref.to_u8_torch(dev.permute(0, 1, 3, 2)))    # not contiguous: torch
    from invertible_cd_amd import _lib
    rc = _lib.load().icd_image_to_u8(_vp(dev), int(dtype == torch.float32), B, H, W, _vp(pad),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(pad[:B * H * W * 3].view(B, H, W, 3), want) and bool((pad[B * H * W * 3:] == 0xA5).all())


def test_image_to_u8_fp32_on_all_256_ingest_values():
    from invertible_cd_amd import ops
    k = torch.arange(256, dtype=torch.float32) / 127.5 - 1
    x = k.repeat(3).reshape(1, 3, 16, 16).contiguous().cuda()
    assert torch.equal(ops.image_to_u8(x), ref.to_u8_torch(x))
    assert torch.equal(ops.image_to_u8(x).cpu(), ref.to_u8_steps(x.cpu()))


# ------------------------------------------------------------------------------------------------ encode_images against encode
def _vae(dtype, max_chunk):
    from invertible_cd_amd import synthetic, vae
    cfg = vae.SD_VAE.scaled((32, 64, 64, 64))
    sd = synthetic.synthetic_vae_state_dict(cfg, seed=21)
    m = vae.AutoencoderKL(cfg, sd, max_chunk=max_chunk)
    return m.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_encode_images_gives_the_bits_of_encode_on_the_host_routes_tensor(dtype):
    """B = 3 with max_chunk = 2: the chunk seam.  Mixed sizes in one list: ingested size by size, encoded in the caller's order."""
    m = _vae(dtype, max_chunk=2)
    S = 64
    imgs = ref.images(3, 50, 70)
    want_u8 = ref.pil_resize(imgs, S)
    x = ref.host_route(want_u8).to("cuda", dtype=dtype)
    want = m.encode(x)["latent_dist"]
    out = m.encode_images(torch.from_numpy(imgs).cuda(), S, want_bytes=True)
    got = out["latent_dist"]
    assert got.mean.dtype == dtype and tuple(got.mean.shape) == (3, 4, 8, 8)
    assert torch.equal(got.mean, want.mean) and torch.equal(got.logvar, want.logvar)
    assert torch.equal(out["images"].cpu(), torch.from_numpy(want_u8))
    assert "images" not in m.encode_images(torch.from_numpy(imgs).cuda(), S)
    # a list of three sizes, the middle one already S x S
    other = [ref.images(1, 90, 40)[0], ref.images(1, S, S)[0], imgs[2]]
    want_u8 = np.stack([ref.pil_resize(o[None], S)[0] for o in other])
    want = m.encode(ref.host_route(want_u8).to("cuda", dtype=dtype))["latent_dist"]
    out = m.encode_images([torch.from_numpy(o).cuda() for o in other], S, want_bytes=True)
    assert torch.equal(out["latent_dist"].mean, want.mean) and torch.equal(out["latent_dist"].logvar, want.logvar)
    assert torch.equal(out["images"].cpu(), torch.from_numpy(want_u8))
    # size=None: the images' own size
    own = m.encode_images(torch.from_numpy(want_u8).cuda())["latent_dist"]
    assert torch.equal(own.mean, want.mean)
    with pytest.raises(ValueError):
        m.encode_images(torch.from_numpy(imgs).cuda())          # 50 x 70 is no size of its own
    with pytest.raises(ValueError):
        m.encode_images(torch.from_numpy(imgs).cuda(), 60)
    with pytest.raises(ValueError):
        m.encode_images(torch.from_numpy(imgs).cuda().float(), S)


# ------------------------------------------------------------------------------------------------ end to end
def test_invert_with_device_images_returns_the_host_routes_latents_and_bytes(tmp_path):
    from PIL import Image
    from invertible_cd_amd import clip, generation, inversion, synthetic, vae
    from invertible_cd_amd.loading import load_models
    from invertible_cd_amd.schedulers import DDIMScheduler
    rng = np.random.default_rng(0)
    paths = [str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    Image.fromarray(rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)).save(paths[0])
    Image.fromarray(rng.integers(0, 256, (640, 520, 3), dtype=np.uint8)).save(paths[1])
    comp = {"vae_state_dict": synthetic.synthetic_vae_state_dict(vae.SD_VAE, seed=0, device="cuda", dtype=torch.float16),
            "text_encoder_state_dict": synthetic.synthetic_clip_state_dict(clip.CLIP_VIT_L, seed=0)}
    ldm, rev, fwd = load_models("synthetic:sd15", "cuda", reverse_checkpoint="synthetic:1", forward_checkpoint="synthetic:2",
                                w_embed_dim=512, dtype="fp16", components=comp)
    solver = generation.Generator(ldm, 50, DDIMScheduler.sd15(), forward_cons_model=fwd, reverse_cons_model=rev,
                                  reverse_timesteps=[259, 519, 779, 999], forward_timesteps=[19, 259, 519, 779])
    prompts = ["a photo of a cat sitting on a bench", "a red car"]
    kw = dict(stop_step=50, is_cons_inversion=True, inv_guidance_scale=0.0, w_embed_dim=512, image_path=paths, prompt=prompts, seed=[1, 2])
    (gt_h, rec_h), lat_h, _ = inversion.invert(solver, **kw)
    (gt_d, rec_d), lat_d, _ = inversion.invert(solver, device_images=True, **kw)
    assert torch.equal(lat_d, lat_h) and tuple(lat_d.shape) == (2, 4, 64, 64)
    assert gt_d.is_cuda and gt_d.dtype == torch.uint8 and tuple(gt_d.shape) == (2, 512, 512, 3)
    assert np.array_equal(gt_d.cpu().numpy(), np.stack(gt_h))
    assert rec_d.is_cuda and rec_d.dtype == torch.uint8 and tuple(rec_d.shape) == (2, 512, 512, 3)
    assert rec_h.shape == (512, 512, 3) and np.array_equal(rec_d[0].cpu().numpy(), rec_h)    # the host route decodes the first image only
    # image2latent: a uint8 batch on the device is encoded (it used to come back unchanged), a floating-point 4-d tensor still passes
    lat = solver.image2latent(gt_d)
    assert torch.equal(lat, solver.image2latent([g for g in gt_h])) and solver.image2latent(lat) is lat
    # the sampler's bytes are those of the expression _to_uint8_device has always evaluated
    run = lambda rt: generation.runner(model=rev, prompt=prompts[:1], controller=None, solver=solver, is_cons_forward=True,
                                       latent=lat_d[:1].cpu(), guidance_scale=7.0, tau1=1.0, tau2=1.0, w_embed_dim=512, return_type=rt)[0]
    sample = rev.vae.decode(1 / 0.18215 * run("latent").to(rev.vae.dtype))["sample"]
    got = run("uint8_device")
    assert got.is_cuda and torch.equal(got, ref.to_u8_torch(sample))
    assert np.array_equal(got.cpu().numpy(), run("image"))
