"""Host-side references of the VAE's two ends, shared by tests/test_vae_ingest.py (CPU) and tests/test_vae_ingest_gpu.py.

Everything here is plain numpy / torch on the CPU / Pillow: the route images take through generation.load_512 and Generator.image2latent
on the host, and the arithmetic of generation._to_uint8_device restated step by step."""
import functools

import numpy as np
import torch

# (H, W, S): identity taps twice, up both axes twice, down both axes with wide tap rows, one axis up and one down at odd widths,
# an extreme upscale with W % 4 != 0, a downscale of odd sizes
SIZES = [(512, 512, 512), (64, 64, 64), (300, 400, 512), (333, 250, 512), (1024, 768, 512), (513, 511, 512), (17, 23, 64), (129, 255, 64)]


def images(B, H, W):
    """[B, H, W, 3] uint8: seeded uniform noise; from B = 3 on, image 1 is constant 255 and image 2 constant 0"""
    imgs = np.random.default_rng(H * 10007 + W * 13 + B).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    if B >= 3:
        imgs[1], imgs[2] = 255, 0
    return imgs


def pil_resize(imgs, S):
    """np.array(Image.fromarray(img).resize((S, S))) per image: what load_512 does to a file's pixels"""
    from PIL import Image
    return np.stack([np.array(Image.fromarray(im).resize((S, S))) for im in imgs])


def host_route(resized):
    """image2latent's host arithmetic on resized uint8 [B, S, S, 3] arrays -> fp32 NCHW in [-1, 1]"""
    return (torch.from_numpy(resized).float() / 127.5 - 1).permute(0, 3, 1, 2)


def to_u8_steps(x):
    """generation._to_uint8_device spelled out on a CPU tensor [B, 3, H, W] (fp16 or fp32): every step in fp32, rounded to the sample's
    dtype before the next one, then truncation towards zero -> uint8 [B, H, W, 3]."""
    dt = x.dtype
    v = (x.float() * 0.5).to(dt)
    v = (v.float() + 0.5).to(dt)
    v = v.float().clamp(0.0, 1.0).to(dt)
    v = (v.float() * 255.0).to(dt)
    return v.float().permute(0, 2, 3, 1).to(torch.uint8).contiguous()


def to_u8_torch(x):
    """the expression generation._to_uint8_device has always evaluated, as torch evaluates it on x's device"""
    image = (x / 2 + 0.5).clamp(0, 1)
    return (image.permute(0, 2, 3, 1) * 255).to(torch.uint8).contiguous()


def fp32_sample(B, H, W, seed):
    """[B, 3, H, W] fp32: seeded uniform values in [-1.5, 1.5] whose first elements are -1, 1, 0, -0 and k / 127.5 - 1 for every byte k
    (as many of them as fit)"""
    x = torch.rand(B * 3 * H * W, generator=torch.Generator().manual_seed(seed)) * 3 - 1.5
    edge = torch.cat([torch.tensor([-1.0, 1.0, 0.0, -0.0, 1.5, -1.5]), torch.arange(256, dtype=torch.float32) / 127.5 - 1])
    n = min(edge.numel(), x.numel())
    x[:n] = edge[:n]
    return x.reshape(B, 3, H, W).contiguous()


@functools.lru_cache(maxsize=None)
def all_fp16_sample(H=148, W=144):
    """Every fp16 bit pattern that is not a NaN (63 490 of them, both infinities and both zeros included) laid out as a [1, 3, H, W]
    sample; the tail repeats the head.  Returns (sample, its bytes by to_u8_steps); neither is to be modified."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    h = bits.view(torch.float16)
    h = h[~torch.isnan(h)]
    assert h.numel() == 65536 - 2 * 1023 and 3 * H * W >= h.numel()
    x = h.repeat((3 * H * W + h.numel() - 1) // h.numel())[:3 * H * W].reshape(1, 3, H, W).contiguous()
    return x, to_u8_steps(x)
