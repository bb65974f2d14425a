"""Edit-quality metrics on the device (API mirror of the DINOv2 score, the CLIP scores, PSNR, LPIPS and the inversion report of the
reference's utils/metrics.py).

    calc_dinov2_images_images(images_1, images_2, device, batch_size=50, model=...)          utils/metrics.py:176-207
    calc_clip_score_images_images(images_1, images_2, device, batch_size=50, model=...)      utils/metrics.py:211-242
    calc_clip_score_images_prompts(images, prompts, device, batch_size=50, model=...)        utils/metrics.py:246-280
    calculate_psnr(images_1, images_2, device, batch_size=50)                                utils/metrics.py:295-308
    calculate_lpips(images_1, images_2, device, batch_size=50, model=...)
    calc_inversion(path_to_dir, device, dinov2_model=..., lpips_model=...)
    get_activations / calculate_activation_statistics / calculate_frechet_distance / compute_statistics_of_path /
    save_statistics_of_path / calculate_fid(images, path, device=None, batch_size=40, dims=2048, ..., model=...)    utils/metrics.py:40-171

Names, argument order and return values are the reference's; `model=` is what the reference fetched from the hub on every call
(`AutoModel.from_pretrained('openai/clip-vit-large-patch14')`: a clip.CLIPModel, e.g. from loading.load_clip;
`AutoModel.from_pretrained('facebook/dinov2-base')`: a dinov2.Dinov2Model, e.g. from loading.load_dinov2; `piq.LPIPS()`: a lpips.Lpips,
e.g. from loading.load_lpips).  Images may be PIL images, numpy uint8 HWC arrays, or a uint8 NHWC tensor on the device
(generation.runner(..., return_type='uint8_device')), which is preprocessed (icd_clip_preprocess / icd_image_resize_norm, csrc/ingest.hip), embedded
and scored (icd_cosine_rows / icd_lpips_layer) without a copy to the host.  A list may mix image sizes (each size
is preprocessed as one batch); a tensor or array holds one size.  `prompts` are token ids [N, T]
(as everywhere in this package) or strings together with `tokenizer=`.  LPIPS is computed from its definition (a VGG16 feature stack,
lpips.py) rather than through `piq`, and FID from its own (the FID Inception-v3 of inception.py, `model=` an inception.FidInception, e.g.
from loading.load_inception; the statistics stream through FidStatistics / icd_moments_f64 on the device, the Frechet distance itself is
float64 scipy on the host, as in the reference; dims other than 2048 are refused).

    calc_ir(images, prompts, device, batch_size=50, model=..., tokenizer=...)                utils/metrics.py:283-293
    calc_all(path_to_orig, path_to_edited, path_to_benchmark, outdir, device, clip_model=..., dinov2_model=..., ir_model=...,
             tokenizer=..., ir_tokenizer=...)                                                utils/metrics.py:327-390

ImageReward is the BLIP pair and reward head of blip.py (`RM.load("ImageReward-v1.0")`: a blip.ImageReward, e.g. from
loading.load_imagereward); its prompts are (input_ids, attention_mask) of the package's BERT tokenizer.  The architecture is tested against
`transformers`; the translation of the ImageReward package's checkpoint key names is unverified (blip.py).
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
    from .encoder import image_batch_to_device, image_size, mixed_sizes, run_by_size
    if isinstance(images, np.ndarray):                          # a stacked array is a batch: the towers themselves refuse one
        images = image_batch_to_device(images, model.device)
    if not mixed_sizes(images):
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


def _ir_tokens(prompts, tokenizer):
    """(input_ids, attention_mask) [N, T]: a pair of tensors as it is, strings through `tokenizer` called as the ImageReward package
    calls its BERT tokenizer."""
    if isinstance(prompts, (tuple, list)) and len(prompts) == 2 and all(isinstance(p, (torch.Tensor, np.ndarray)) for p in prompts):
        return torch.as_tensor(prompts[0]), torch.as_tensor(prompts[1])
    if tokenizer is None:
        raise ValueError("metrics: string prompts need tokenizer= (or pass (input_ids, attention_mask) tensors [N, T])")
    enc = tokenizer(list(prompts), padding='max_length', truncation=True, max_length=35, return_tensors='pt')
    return torch.as_tensor(enc["input_ids"]), torch.as_tensor(enc["attention_mask"])


@torch.no_grad()
def calc_ir(images, prompts, device, batch_size=50, model=None, tokenizer=None):
    """ImageReward of corresponding (image, prompt) pairs -> a list of Python floats, one per pair, in the caller's order (the
    reference's editing_imagereward).  model=: a blip.ImageReward, e.g. loading.load_imagereward(path).  prompts: (input_ids,
    attention_mask) tensors [N, T], or strings together with tokenizer= (called with padding='max_length', truncation=True,
    max_length=35, return_tensors='pt', as the package calls it).  The reference scores the pairs one by one; here they are scored
    `batch_size` at a time, and only the scores cross to the host."""
    model = _need_model(model, "a blip.ImageReward, e.g. loading.load_imagereward(path)")
    ids, mask = _ir_tokens(prompts, tokenizer)
    n = ids.shape[0]
    assert _count(images) == n
    rewards = []
    for i in range(0, n, batch_size):
        rewards += model.score(ids[i:i + batch_size], mask[i:i + batch_size], images[i:i + batch_size]).cpu().tolist()
    return [float(r) for r in rewards]


def calc_all(path_to_orig, path_to_edited, path_to_benchmark, outdir, device, clip_model=None, dinov2_model=None, ir_model=None,
             tokenizer=None, ir_tokenizer=None):
    """The editing report (utils/metrics.py:327-390): the edited images `path_to_edited`/<number>.<ext>, in numeric order, against the
    originals and prompts of the editing benchmark (loading.load_benchmark(path_to_benchmark, path_to_orig)), scored in batches of 16
    and written to `outdir`/editing_metrics_values.json under the reference's keys preservation_clip_score, preservation_dinov2,
    editing_clip_score and editing_imagereward, the values stringified as there.  Returns that dict.  tokenizer= is CLIP's,
    ir_tokenizer= ImageReward's BERT tokenizer.  One deliberate difference: an empty `path_to_edited` returns None WITHOUT DELETING
    THE DIRECTORY (the reference calls shutil.rmtree on it)."""
    from .generation import load_512, to_pil_images
    from .loading import load_benchmark
    _need_model(clip_model, "clip_model=, a clip.CLIPModel, e.g. loading.load_clip(path)")
    _need_model(dinov2_model, "dinov2_model=, a dinov2.Dinov2Model, e.g. loading.load_dinov2(path)")
    _need_model(ir_model, "ir_model=, a blip.ImageReward, e.g. loading.load_imagereward(path)")
    editing_benchmark = load_benchmark(path_to_benchmark, path_to_orig)
    files = os.listdir(path_to_edited)
    if len(files) == 0:
        print(path_to_edited)
        return None
    files = [file for file in files if file != 'editing_metrics_values.json']
    files.sort(key=lambda x: int(x.split('.')[0]))
    orig_images, edited_prompts, edited_images = [], [], []
    for j, (image_path, prompts_dict, _) in enumerate(editing_benchmark):
        if j >= len(files):                          # (the reference's `except IndexError: continue`)
            continue
        orig_images.append(to_pil_images(load_512(f'{image_path}')))
        edited_images.append(to_pil_images(load_512(f'{path_to_edited}/{files[j]}')))
        edited_prompts.append(prompts_dict['after'])
    preserve_clip_score = calc_clip_score_images_images(orig_images, edited_images, device, batch_size=16, model=clip_model)
    preserve_dinov2 = calc_dinov2_images_images(orig_images, edited_images, device, batch_size=16, model=dinov2_model)
    editing_clip_score = calc_clip_score_images_prompts(edited_images, edited_prompts, device, batch_size=16, model=clip_model,
                                                        tokenizer=tokenizer)
    editing_imagereward = calc_ir(edited_images, edited_prompts, device, batch_size=16, model=ir_model, tokenizer=ir_tokenizer)
    for name, values in (("cs", preserve_clip_score), ("dinov", preserve_dinov2), ("cs edit", editing_clip_score),
                         ("ir", torch.tensor(editing_imagereward))):
        print(f'{name} {torch.mean(values)}')
        print(f'{name} {torch.std(values)}')
    results = {'preservation_clip_score': str(list(np.array(preserve_clip_score))),
               'preservation_dinov2': str(list(np.array(preserve_dinov2))),
               'editing_clip_score': str(list(np.array(editing_clip_score))),
               'editing_imagereward': str(editing_imagereward)}
    os.makedirs(outdir, exist_ok=True)
    with open(f'{outdir}/editing_metrics_values.json', "w") as fp:
        json.dump(results, fp)
    return results


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


# ------------------------------------------------------------------------------------------------------------ FID
IMAGE_EXTENSIONS = {'bmp', 'jpg', 'jpeg', 'pgm', 'png', 'ppm', 'tif', 'tiff', 'webp'}
INCEPTION_PATH = "files/pt_inception-2015-12-05-6726825d.pth"


def _check_dims(dims):
    if dims != 2048:
        raise ValueError(f"metrics: FID is computed on the pooled features (dims=2048) only, got dims={dims}")


def _fid_model(model, inception_path, device):
    if model is not None:
        return model
    from .loading import load_inception
    return load_inception(inception_path, device="cuda" if device is None else device)


def _open_images(images):
    """file names in a list become PIL images; everything else passes"""
    if isinstance(images, (list, tuple)) and len(images) and isinstance(images[0], (str, os.PathLike)):
        from PIL import Image
        return [Image.open(p).convert("RGB") for p in images]
    return images


def _feature_batches(images, model, batch_size):
    for i in range(0, _count(images), batch_size):
        yield i, model.features(_open_images(images[i:i + batch_size]))


class FidStatistics:
    """Streaming mean and covariance of feature rows: n, sum x and sum x x^T in float64.  `update` adds a batch of fp32 features on the
    device (icd_moments_f64: fixed order, no atomics); sums of several accumulators - batches, ranks - simply add (`merge`, `add`)."""

    def __init__(self):
        self.n, self.total, self.outer = 0, None, None

    def add(self, n, total, outer):
        """add raw sums: n rows, sum x [D], sum x x^T [D, D] (numpy or torch, any device)"""
        as64 = lambda t: (t.detach().to(torch.float64) if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t, np.float64))).clone()
        total, outer = as64(total), as64(outer)
        if self.total is None:
            self.total, self.outer = total, outer
        else:
            if total.shape != self.total.shape:
                raise ValueError(f"FidStatistics: features of width {total.shape[0]} added to sums of width {self.total.shape[0]}")
            self.total += total.to(self.total.device)
            self.outer += outer.to(self.outer.device)
        self.n += int(n)
        return self

    def update(self, features):
        """features: fp32 [n, D] on the device"""
        from . import ops
        if features.dim() != 2 or not features.is_cuda:
            raise ValueError("FidStatistics.update: features must be a device tensor [n, D]")
        f = features.to(torch.float32).contiguous()
        if self.total is None:
            D = f.shape[1]
            self.total = torch.zeros((D,), device=f.device, dtype=torch.float64)
            self.outer = torch.zeros((D, D), device=f.device, dtype=torch.float64)
        ops.moments_f64(f, self.total, self.outer)
        self.n += f.shape[0]
        return self

    def merge(self, other):
        return self.add(other.n, other.total, other.outer) if other.n else self

    def finalize(self):
        """(mu [D], sigma [D, D]) as float64 numpy arrays: np.mean(x, axis=0) and np.cov(x, rowvar=False) (n - 1 in the denominator)."""
        if self.n < 2:
            raise ValueError(f"FidStatistics: {self.n} rows are too few for a covariance")
        total, outer = self.total.cpu().numpy(), self.outer.cpu().numpy()
        mu = total / self.n
        return mu, (outer - self.n * np.outer(mu, mu)) / (self.n - 1)


@torch.no_grad()
def get_activations(images, model, batch_size=50, dims=2048, device='cpu', num_workers=8):
    """The pooled Inception features of every image -> float64 numpy [N, model.cfg.dims] (the reference's pred_arr).  `images`: PIL
    images, numpy uint8 HWC arrays, file names, or a uint8 NHWC tensor on the device; the loader's Resize(256, LANCZOS) + CenterCrop(256)
    runs on the device (icd_fid_ingest).  `device` and `num_workers` are the reference's arguments; the model's device is used."""
    _check_dims(dims)
    n = _count(images)
    if batch_size > n:
        print(f'get_activations: batch_size {batch_size} exceeds the {n} images; using {n}')
        batch_size = n
    pred_arr = np.empty((n, model.cfg.dims))
    for i, f in _feature_batches(images, model, batch_size):
        pred_arr[i:i + f.shape[0]] = f.cpu().numpy()
    return pred_arr


@torch.no_grad()
def calculate_activation_statistics(images, model, batch_size=50, dims=2048, device='cpu', num_workers=8):
    """(mu, sigma) of the pooled features: np.mean(act, axis=0), np.cov(act, rowvar=False), accumulated batch by batch on the device
    (FidStatistics) - the [N, 2048] activations never exist on the host."""
    _check_dims(dims)
    stats = FidStatistics()
    for _, f in _feature_batches(images, model, max(1, min(batch_size, _count(images)))):
        stats.update(f)
    return stats.finalize()


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + tr(sigma1) + tr(sigma2) - 2 tr sqrt(sigma1 sigma2), in float64 on the host (scipy.linalg.sqrtm): the
    reference's arithmetic, off the hot path.  When the root of the product comes back with non-finite entries (a singular product),
    it is taken again with eps added to both diagonals, and a line says so; a root whose diagonal has an imaginary part beyond 1e-3 is
    an error, a smaller imaginary part is numerical noise and is dropped."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape:
        raise ValueError(f"calculate_frechet_distance: mean vectors of lengths {mu1.shape} and {mu2.shape}")
    if sigma1.shape != sigma2.shape:
        raise ValueError(f"calculate_frechet_distance: covariances of shapes {sigma1.shape} and {sigma2.shape}")

    def root(a, b):
        r = linalg.sqrtm(a @ b)
        return r[0] if isinstance(r, tuple) else r
    half = root(sigma1, sigma2)
    if not np.all(np.isfinite(half)):
        print(f"calculate_frechet_distance: sqrt(sigma1 sigma2) is not finite (singular product); retrying with {eps} on both diagonals")
        ridge = eps * np.identity(sigma1.shape[0])
        half = root(sigma1 + ridge, sigma2 + ridge)
    if np.iscomplexobj(half):
        worst = float(np.abs(np.diagonal(half).imag).max())
        if worst > 1e-3:
            raise ValueError(f"calculate_frechet_distance: sqrt(sigma1 sigma2) has an imaginary diagonal of up to {worst}")
        half = half.real
    delta = mu1 - mu2
    return float(delta @ delta) + float(np.trace(sigma1)) + float(np.trace(sigma2)) - 2.0 * float(np.trace(half))


def compute_statistics_of_path(path, model, batch_size, dims, device, num_workers=8):
    """(mu, sigma) from an `.npz` with `mu` / `sigma`, or of the image files of a directory (sorted by name)."""
    path = os.fspath(path)
    if path.endswith('.npz'):
        with np.load(path) as f:
            return f['mu'][:], f['sigma'][:]
    files = sorted(os.path.join(path, name) for name in os.listdir(path) if name.rsplit('.', 1)[-1].lower() in IMAGE_EXTENSIONS)
    return calculate_activation_statistics(files, model, batch_size, dims, device, num_workers)


def save_statistics_of_path(path, out_path, device=None, batch_size=50, dims=2048, num_workers=8, inception_path=INCEPTION_PATH, model=None):
    """The statistics of a directory of images, written as the `.npz` that calculate_fid reads."""
    _check_dims(dims)
    model = _fid_model(model, inception_path, device)
    m1, s1 = compute_statistics_of_path(path, model, batch_size, dims, device, num_workers)
    np.savez(out_path, mu=m1, sigma=s1)


def calculate_fid(images, path, device=None, batch_size=40, dims=2048, num_workers=4, inception_path=INCEPTION_PATH, model=None):
    """FID of `images` against the statistics of `path` (an `.npz` or a directory of images).  model=: an inception.FidInception, e.g.
    loading.load_inception(path); without it `inception_path` is read from disk.  Nothing is downloaded."""
    _check_dims(dims)
    if not os.path.exists(path):
        raise RuntimeError(f'calculate_fid: {path} does not exist (want an .npz of statistics or a directory of images)')
    model = _fid_model(model, inception_path, device)
    m1, s1 = calculate_activation_statistics(images, model, batch_size, dims, device, num_workers)
    m2, s2 = compute_statistics_of_path(path, model, batch_size, dims, device, num_workers)
    return calculate_frechet_distance(m1, s1, m2, s2)
