"""Host side of the CLIP image preprocessing: Pillow's BICUBIC resample restated as integer coefficient tables.

`PIL.Image.resize(size, BICUBIC)` is an antialiased two-pass separable resample (horizontal pass, then vertical): the cubic filter
(a = -0.5) is stretched by the scale factor when shrinking, each output pixel's taps are normalised in double, rounded to fixed point
with 22 fractional bits, and both passes accumulate in int32 and clip to uint8.  Once the tables exist the arithmetic is pure integer,
so `icd_clip_preprocess` (csrc/ingest.hip) reproduces it bit for bit.  This module is numpy only: it builds the tables, states the
shortest-edge / centre-crop geometry of `transformers.CLIPImageProcessor`, and carries a numpy emulation of the two passes (the CPU
test's check of the tables against Pillow itself; the device kernel is checked against Pillow on the GPU).
"""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2                      # Pillow's fixed-point fraction: int32 accumulators, 8-bit samples, 2 bits of headroom
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN = (0.485, 0.456, 0.406)            # transformers.BitImageProcessor with DINOv2's preprocessor_config.json
IMAGENET_STD = (0.229, 0.224, 0.225)


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def _lanczos(x):
    """Pillow's lanczos_filter (support 3): sinc(x) sinc(x / 3)"""
    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}      # name -> (kernel, support)


def tap_width(in_size, out_size, filter="bicubic"):
    """Row length of the coefficient table (Pillow's ksize): 2 * ceil(support) + 1 with support = 2 (bicubic) or 3 (lanczos) times
    max(in / out, 1)."""
    return int(math.ceil(FILTERS[filter][1] * max(in_size / out_size, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=64)
def resample_tables(in_size, out_size, filter="bicubic"):
    """One axis of the resample: (first [out] int32, count [out] int32, coef [out, tap_width] int32, zero padded).
    filter: 'bicubic' (Pillow's BICUBIC, the default) or 'lanczos' (Pillow's LANCZOS, what the FID loader resizes with).

    Output pixel i is clip8((sum_k coef[i, k] * in[first[i] + k] + 2^21) >> 22) over k < count[i]."""
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resample_tables: sizes must be positive, got {in_size} -> {out_size}")
    if filter not in FILTERS:
        raise ValueError(f"resample_tables: unknown filter {filter!r} (want one of {sorted(FILTERS)})")
    kernel, width = FILTERS[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = width * filterscale
    ksize = tap_width(in_size, out_size, filter)
    first = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = np.array([kernel((x + xmin - center + 0.5) * ss) for x in range(xmax)], np.float64)
        total = 0.0
        for v in w:                               # Pillow sums in tap order; keep the order so the double result is the same
            total += v
        if total != 0.0:
            w = w / total
        k = np.where(w < 0, (-0.5 + w * (1 << PRECISION_BITS)).astype(np.int64), (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64))
        first[i], count[i] = xmin, xmax
        coef[i, :xmax] = k                        # astype(int64) truncates towards zero, as the C cast does
    for a in (first, count, coef):
        a.setflags(write=False)
    return first, count, coef


def clip_geometry(height, width, size=224, crop=224):
    """(resized_h, resized_w, top, left) of CLIPImageProcessor: shortest edge -> `size` (the longer one truncated), centre crop."""
    if height <= 0 or width <= 0:
        raise ValueError(f"clip_geometry: bad image size {height} x {width}")
    short, long = (width, height) if width <= height else (height, width)
    new_long = int(size * long / short)
    rh, rw = (new_long, size) if width <= height else (size, new_long)
    if rh < crop or rw < crop:
        raise ValueError(f"clip_geometry: resized image {rh} x {rw} is smaller than the {crop} crop")
    return rh, rw, (rh - crop) // 2, (rw - crop) // 2


def _pass(img, tables, axis):
    first, count, coef = tables
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(first),) + img.shape[1:], np.uint8)
    for i in range(len(first)):
        k = coef[i, :count[i]].astype(np.int64)
        acc = np.tensordot(k, img[first[i]:first[i] + count[i]], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_emulated(img, out_h, out_w, filter="bicubic", skip_identity=True):
    """numpy restatement of the two integer passes on a uint8 [H, W, C] image (what the device kernel computes).  Pillow skips a pass
    whose size does not change; the device kernels run it (skip_identity=False) - its table is the identity."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    h, w = img.shape[:2]
    if out_w != w or not skip_identity:
        img = _pass(img, resample_tables(w, out_w, filter), 1)
    if out_h != h or not skip_identity:
        img = _pass(img, resample_tables(h, out_h, filter), 0)
    return img


def fid_geometry(height, width, size=256):
    """(resized_h, resized_w, top, left) of torchvision's Resize(size) + CenterCrop(size): the shorter edge goes to `size`, the longer one
    to int(size * long / short), the crop starts at int(round((resized - size) / 2.0))."""
    if height <= 0 or width <= 0:
        raise ValueError(f"fid_geometry: bad image size {height} x {width}")
    short, long = (width, height) if width <= height else (height, width)
    new_long = int(size * long / short)
    rh, rw = (new_long, size) if width <= height else (size, new_long)
    return rh, rw, int(round((rh - size) / 2.0)), int(round((rw - size) / 2.0))
