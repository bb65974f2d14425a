"""Host-side references of the SDXL image rules, shared by tests/test_sdxl_images.py (CPU) and tests/test_sdxl_images_gpu.py.

Plain numpy / Pillow restatements of the two diffusers expressions the device entries reproduce:
  ingest   VaeImageProcessor.preprocess:   np.asarray(im, float32) / 255.0, then 2.0 * x - 1.0              (icd_vae_ingest_f32)
  output   VaeImageProcessor.postprocess:  (x / 2 + 0.5).clamp(0, 1) in x's dtype, then (float32 * 255).round().astype("uint8")
                                                                                                           (icd_image_to_u8_round)
Nothing here is to be modified by a test: the tie samples are cached."""
import functools

import numpy as np

TIE_SHAPE = (2, 3, 3, 5)                       # odd, not square: a swapped H / W in the NCHW -> NHWC transposition shows


def images(B, H, W, seed=0):
    """[B, H, W, 3] uint8 seeded uniform noise"""
    return np.random.default_rng(seed + H * 10007 + W * 13 + B).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def pil_resize(imgs, S):
    """np.array(Image.fromarray(img).resize((S, S))) per image: Pillow's default BICUBIC, both axes stretched"""
    from PIL import Image
    return np.stack([np.array(Image.fromarray(im).resize((S, S))) for im in imgs])


def ingest_values(u8):
    """uint8 array -> float32 array of the same shape: preprocess's arithmetic, a float32 division and `2.0 * x - 1.0` in float32"""
    x = np.asarray(u8, dtype=np.float32) / 255.0
    assert x.dtype == np.float32
    return (2.0 * x - 1.0).astype(np.float32)


def split(v):
    """float32 -> (hi, lo) float16: hi = fp16(v), lo = fp16(v - fp32(hi)), the two halves of a split operand"""
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split3_operand(resized_u8):
    """resized uint8 [B, S, S, 3] -> float16 [B * S * S, 24]: the 8-channel packing's split3 layout [hi | lo | hi], pad columns zero"""
    B, S, _, _ = resized_u8.shape
    hi, lo = split(ingest_values(resized_u8).reshape(B * S * S, 3))
    out = np.zeros((B * S * S, 24), dtype=np.float16)
    out[:, 0:3], out[:, 8:11], out[:, 16:19] = hi, lo, hi
    return out


def to_u8_round(x):
    """postprocess on a numpy NCHW sample (float16 or float32) -> uint8 NHWC; every step of the first line in x's own dtype"""
    dt = x.dtype
    assert dt in (np.float16, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.clip(x / dt.type(2) + dt.type(0.5), dt.type(0), dt.type(1))
        assert y.dtype == dt
        return (y.transpose(0, 2, 3, 1).astype(np.float32) * 255).round().astype("uint8")


@functools.lru_cache(maxsize=None)
def tie_samples(dtype_name):
    """A tuple of read-only [2, 3, 3, 5] samples of dtype float16 / float32 whose values straddle every rounding tie of the output rule:
    for k = 0 .. 254, the x for which 255 * (x / 2 + 0.5) is k + 0.5 (as near as the dtype comes) and the values two steps to either
    side of it, in steps of x and in steps of y = x / 2 + 0.5; then 0, -0, +-1, the neighbours of +-1, values outside [-1, 1] and
    +-inf.  The last sample repeats the first values to fill its shape."""
    dt = np.dtype(dtype_name)
    vals = []

    def around(v):
        lo1, hi1 = np.nextafter(v, dt.type(-2)), np.nextafter(v, dt.type(2))
        return [np.nextafter(lo1, dt.type(-2)), lo1, v, hi1, np.nextafter(hi1, dt.type(2))]

    for k in range(255):
        # neighbours of x where x is the coarser grid (x < 0: several y of the dtype share one x), neighbours of y = x / 2 + 0.5 where
        # y is (x >= 0: x = 2 y - 1 is exact there, and the x next to 0 would all give y = 0.5)
        vals += around(dt.type(2.0 * (k + 0.5) / 255.0 - 1.0))
        vals += [dt.type(2.0 * float(y) - 1.0) for y in around(dt.type((k + 0.5) / 255.0))]
    one = dt.type(1)
    vals += [dt.type(0.0), dt.type(-0.0), one, -one, np.nextafter(one, dt.type(0)), np.nextafter(one, dt.type(2)),
             np.nextafter(-one, dt.type(0)), np.nextafter(-one, dt.type(-2)), dt.type(1.5), dt.type(-1.5), dt.type(3.0), dt.type(-7.25),
             dt.type(60000.0), dt.type(-60000.0), dt.type(np.inf), dt.type(-np.inf)]
    flat = np.array(vals, dtype=dt)
    n = int(np.prod(TIE_SHAPE))
    count = (flat.size + n - 1) // n
    flat = np.resize(flat, count * n)                       # repeats from the start
    out = []
    for i in range(count):
        a = flat[i * n:(i + 1) * n].reshape(TIE_SHAPE).copy()
        a.setflags(write=False)
        out.append(a)
    return tuple(out)
