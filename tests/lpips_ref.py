"""The LPIPS oracle of tests/test_lpips.py and tests/test_lpips_gpu.py: plain torch on the CPU (F.conv2d, F.max_pool2d), the six steps of
piq's LPIPS as invertible_cd_amd/lpips.py restates them, in fp32 - and its fp16-storage emulation, the same graph with the normalised
input and every conv + ReLU output rounded to fp16 and back (what the device path stores; its sums run in another order).  Both take the
weights as they are given: the tests hand them the model's weights after .half().float()."""
import numpy as np
import torch
import torch.nn.functional as F


def resize(images, size):
    """uint8 [N, H, W, 3] -> uint8 [N, size, size, 3]: np.array(PIL.Image.resize((size, size))), Pillow's default BICUBIC."""
    from PIL import Image
    return np.stack([np.array(Image.fromarray(im).resize((size, size))) for im in images])


def _r16(x, emulate):
    return x.half().float() if emulate else x


def taps(cfg, sd, images, emulate=False):
    """images uint8 [N, H, W, 3] -> the five ReLU taps, fp32 NCHW."""
    x = torch.from_numpy(resize(images, cfg.size)).permute(0, 3, 1, 2).float() / 255
    mean, std = torch.tensor(cfg.mean).reshape(1, 3, 1, 1), torch.tensor(cfg.std).reshape(1, 3, 1, 1)
    x = _r16((x - mean) / std, emulate)
    out = []
    keys = iter(cfg.conv_keys())
    with torch.no_grad():
        for level, n in enumerate(cfg.convs):
            if level:
                x = F.max_pool2d(x, 2)
            for _ in range(n):
                k = next(keys)
                x = _r16(F.relu(F.conv2d(x, sd[k + ".weight"], sd[k + ".bias"], padding=1)), emulate)
            out.append(x)
    return out


def distance(taps_1, taps_2, lin):
    """fp32 [N] from the taps of both image sets and the five [1, C, 1, 1] weights."""
    score = 0
    for f1, f2, w in zip(taps_1, taps_2, lin):
        n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
        n2 = f2 / (torch.sqrt(torch.sum(f2 ** 2, dim=1, keepdim=True)) + 1e-10)
        score = score + ((n1 - n2) ** 2 * w.reshape(1, -1, 1, 1)).mean(dim=(2, 3)).sum(dim=1)
    return score


def lpips(cfg, sd, lin, images_1, images_2, emulate=False):
    return distance(taps(cfg, sd, images_1, emulate), taps(cfg, sd, images_2, emulate), lin)


def rounded(sd):
    """the state dict both the device model and the oracle are built from: every tensor representable in fp16"""
    return {k: v.half().float() for k, v in sd.items()}


def structured_images(n, h, w, seed=0):
    """blocks + noise: structure at several scales (the generator of tests/test_dinov2_gpu.py's `_images`)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n, h // 8, w // 8, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(base, 8, 1), 8, 2).astype(np.int64) + rng.integers(-40, 41, (n, h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def six_pairs(h, w, seed):
    """four independent structured pairs, one identical pair (index 4), one 90 / 10 blend (index 5)"""
    a, b = structured_images(6, h, w, seed=2 * seed), structured_images(6, h, w, seed=2 * seed + 1)
    b[4] = a[4]
    b[5] = np.rint(0.9 * a[5].astype(np.float64) + 0.1 * b[5].astype(np.float64)).astype(np.uint8)
    return a, b
