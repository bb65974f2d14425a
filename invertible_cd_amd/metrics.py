"""Edit-quality metrics on the device (API mirror of the DINOv2 score, the CLIP scores, PSNR, LPIPS and the inversion report of the
reference's utils/metrics.py).

    calc_dinov2_images_images(images_1, images_2, device, batch_size=50, model=...)          utils/metrics.py:176-207
    calc_clip_score_images_images(images_1, images_2, device, batch_size=50, model=...)      utils/metrics.py:211-242
    calc_clip_score_images_prompts(images, prompts, device, batch_size=50, model=...)        utils/metrics.py:246-280
    calculate_psnr(images_1, images_2, device, batch_size=50)                                utils/metrics.py:295-308
    calculate_lpips(images_1, images_2, device, batch_size=50, model=...)
    calc_inversion(path_to_dir, device, dinov2_model=..., lpips_model=...)

Names, argument order and return values are the reference's; `model=` is what the reference fetched from the hub on every call
(`AutoModel.from_pretrained('openai/clip-vit-large-patch14')`: a clip.CLIPModel, e.g. from loading.load_clip;
`AutoModel.from_pretrained('facebook/dinov2-base')`: a dinov2.Dinov2Model, e.g. from loading.load_dinov2; `piq.LPIPS()`: a lpips.Lpips,
e.g. from loading.load_lpips).  Images may be PIL images, numpy uint8 HWC arrays, or a uint8 NHWC tensor on the device
(generation.runner(..., return_type='uint8_device')), which is preprocessed (icd_clip_preprocess / icd_image_resize_norm), embedded
and scored (icd_cosine_rows / icd_lpips_layer) without a copy to the host.  A list may mix image sizes (each size
is preprocessed as one batch); a tensor or array holds one size.  `prompts` are token ids [N, T]
(as everywhere in this package) or strings together with `tokenizer=`.  LPIPS is computed from its definition (a VGG16 feature stack,
lpips.py) rather than through `piq`; ImageReward and FID stay out: their packages (and weights) are not available.
"""
import json
import math
import os

import numpy as np
import torch

from .resample import resample_tables, clip_geometry, resize_emulated   # noqa: F401  (the host tables are part of this module's interface)


def _need_model(model, what="a clip.CLIPModel, e.g. loading.load_clip(path)"):
    if model is None:
        raise ValueError(f"metrics: pass model= ({what}); nothing is downloaded here")
    return model


def _count(images):
    return images.shape[0] if isinstance(images, (torch.Tensor, np.ndarray)) and images.ndim == 4 else len(images)


def _image_features(model, images):
    """fp32 [N, D] on the device.  A list of images of several sizes (the reference's processor takes one) is embedded size by size."""
    from .encoder import image_size, run_by_size
    if isinstance(images, np.ndarray) and images.ndim == 4:
        images = torch.from_numpy(images)
    if not isinstance(images, (list, tuple)):
        return model.get_image_features(images)
    return run_by_size(len(images), lambda i: image_size(images[i]), lambda idx: model.get_image_features([images[i] for i in idx]))


def _token_ids(prompts, tokenizer):
    if isinstance(prompts, torch.Tensor):
        return prompts
    if isinstance(prompts, np.ndarray):
        return torch.from_numpy(prompts)
    if len(prompts) and isinstance(prompts[0], str):
        if tokenizer is None:
            raise ValueError("metrics: string prompts need tokenizer= (or pass token ids [N, T])")
        return tokenizer(list(prompts), padding=True, truncation=True, max_length=77, return_tensors="pt").input_ids
    return torch.as_tensor(prompts)


@torch.no_grad()
def _paired_cosine(model, images_1, images_2, batch_size):
    """Cosine of the embeddings `model` gives corresponding images -> CPU float tensor [N]."""
    from . import ops
    n = _count(images_2)
    assert _count(images_1) == n
    scores = torch.zeros(n)
    for i in range(0, n, batch_size):
        e1 = _image_features(model, images_1[i:i + batch_size])
        e2 = _image_features(model, images_2[i:i + batch_size])
        scores[i:i + batch_size] = ops.cosine_rows(e2, e1).cpu()
    return scores


def calc_dinov2_images_images(images_1, images_2, device, batch_size=50, model=None):
    """Cosine of the DINOv2 class-token embeddings of corresponding images -> CPU float tensor [N] (the reference's preservation_dinov2)."""
    return _paired_cosine(_need_model(model, "a dinov2.Dinov2Model, e.g. loading.load_dinov2(path)"), images_1, images_2, batch_size)


def calc_clip_score_images_images(images_1, images_2, device, batch_size=50, model=None):
    """Cosine of the CLIP image embeddings of corresponding images -> CPU float tensor [N] (the reference's preservation score)."""
    return _paired_cosine(_need_model(model), images_1, images_2, batch_size)


@torch.no_grad()
def calc_clip_score_images_prompts(images, prompts, device, batch_size=50, model=None, tokenizer=None):
    """Cosine of CLIP image and text embeddings -> CPU float tensor [N] (the reference's editing / generation CLIP score)."""
    from . import ops
    model = _need_model(model)
    ids = _token_ids(prompts, tokenizer)
    n = ids.shape[0]
    assert _count(images) == n
    scores = torch.zeros(n)
    for i in range(0, n, batch_size):
        ei = _image_features(model, images[i:i + batch_size])
        et = model.get_text_features(ids[i:i + batch_size])
        scores[i:i + batch_size] = ops.cosine_rows(et, ei).cpu()
    return scores


def _psnr_from_sums(sums, n):
    psnr = []
    for s in sums:
        mse = float(int(s)) / n                      # an exact integer below 2^53 over n: what np.mean of the float64 squares gives
        if mse == 0:
            return float('inf')                      # the reference returns at the first identical pair
        psnr.append(20 * math.log10(255.0 / math.sqrt(mse)))
    return psnr


def calculate_psnr(images_1, images_2, device, batch_size=50):
    """List of PSNR values in dB (float('inf') as soon as a pair is identical, as the reference returns it).  Device tensors are
    reduced on the device (icd_sq_diff_sum_u8: exact integer sums); host images are reduced on the host, in integers as well."""
    if isinstance(images_1, torch.Tensor) and isinstance(images_2, torch.Tensor) and images_1.is_cuda:
        from . import ops
        if images_1.dtype != torch.uint8 or images_2.dtype != torch.uint8 or images_1.shape != images_2.shape or images_1.dim() != 4:
            raise ValueError("calculate_psnr: device images must be two uint8 [N, H, W, C] tensors of one shape")
        images_2 = images_2.to(images_1.device)
        sums = []
        for i in range(0, images_1.shape[0], batch_size):
            sums += ops.sq_diff_sum_u8(images_1[i:i + batch_size], images_2[i:i + batch_size]).cpu().tolist()
        return _psnr_from_sums(sums, images_1[0].numel())
    psnr = []
    for img1, img2 in zip(images_1, images_2):
        a = np.asarray(img1.cpu() if isinstance(img1, torch.Tensor) else img1)
        b = np.asarray(img2.cpu() if isinstance(img2, torch.Tensor) else img2)
        if a.dtype == np.uint8 and b.dtype == np.uint8:
            diff = a.astype(np.int64) - b.astype(np.int64)
            out = _psnr_from_sums([int((diff * diff).sum())], diff.size)
        else:                                        # anything else: the reference's float64 formula as it stands
            mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
            out = float('inf') if mse == 0 else [20 * math.log10(255.0 / math.sqrt(mse))]
        if not isinstance(out, list):
            return out
        psnr += out
    return psnr


@torch.no_grad()
def calculate_lpips(images_1, images_2, device, batch_size=50, model=None):
    """LPIPS of corresponding images -> CPU float tensor [N] (the reference's piq.LPIPS(reduction='none') on the images resized to
    224 x 224).  Only the scores cross to the host."""
    model = _need_model(model, "a lpips.Lpips, e.g. loading.load_lpips(vgg16_path, lpips_weights_path)")
    n = _count(images_2)
    assert _count(images_1) == n
    scores = torch.zeros(n)
    for i in range(0, n, batch_size):
        scores[i:i + batch_size] = model(images_1[i:i + batch_size], images_2[i:i + batch_size]).cpu()
    return scores


def _directory_images(path):
    """Every file of `path`, in sorted name order, as a 512 x 512 PIL image (generation.load_512 + to_pil_images)."""
    from .generation import load_512, to_pil_images
    return [to_pil_images(load_512(os.path.join(path, name))) for name in sorted(os.listdir(path))]


def calc_inversion(path_to_dir, device, dinov2_model=None, lpips_model=None):
    """The inversion report: `path_to_dir`/generated_images against `path_to_dir`/real_images, scored with the DINOv2 cosine, PSNR and
    LPIPS in batches of 16, written to `path_to_dir`/preservation_metrics_values.json under the reference's three keys
    (preservation_dinov2, preservation_psnr, preservation_lpips), each value the str() of a list of numpy scalars as the reference
    formats it.  Returns that dict.  The reference pairs the files in os.listdir order, which promises nothing about two directories
    agreeing; here BOTH LISTINGS ARE SORTED, so the i-th name of one directory meets the i-th name of the other (files without a
    partner are left out)."""
    _need_model(dinov2_model, "dinov2_model=, a dinov2.Dinov2Model, e.g. loading.load_dinov2(path)")
    _need_model(lpips_model, "lpips_model=, a lpips.Lpips, e.g. loading.load_lpips(vgg16_path, lpips_weights_path)")
    generated = _directory_images(os.path.join(path_to_dir, "generated_images"))
    real = _directory_images(os.path.join(path_to_dir, "real_images"))
    n = min(len(generated), len(real))
    generated, real = generated[:n], real[:n]
    scores = {
        "preservation_dinov2": calc_dinov2_images_images(generated, real, device, batch_size=16, model=dinov2_model),
        "preservation_psnr": calculate_psnr(generated, real, device, batch_size=16),
        "preservation_lpips": calculate_lpips(generated, real, device, batch_size=16, model=lpips_model),
    }
    report = {}
    for key, values in scores.items():
        values = np.atleast_1d(np.array(values))     # PSNR is a bare inf as soon as one pair is identical
        print(f"{key}: mean {float(np.mean(values.astype(np.float64)))}")
        report[key] = str(list(values))
    with open(os.path.join(path_to_dir, "preservation_metrics_values.json"), "w") as fp:
        json.dump(report, fp)
    return report
