"""The FID oracle of tests/test_fid.py and tests/test_fid_gpu.py: plain torch on the CPU (F.conv2d, F.max_pool2d, F.avg_pool2d,
F.interpolate, Pillow), the network of invertible_cd_amd/inception.py's docstring spelled out layer by layer, in fp32 - and its
fp16-storage emulation, the same graph with the network input and every stored activation (each conv + ReLU output, each average pool)
rounded to fp16 and back (what the device path stores; its sums run in another order).  Weights come either as a pytorch-fid state dict
(`<name>.conv.weight`, `<name>.bn.*`: explicit BatchNorm, eps 1e-3, running statistics) or folded, {name: (weight, bias)}."""
import numpy as np
import torch
import torch.nn.functional as F

# Pooled-feature rel-L2 of the fp16-storage emulation against the fp32 oracle at full width, measured on the CPU: synthetic weights of
# seed 0, 1, 2, each on structured_images(2, 96, 128, seed=10 + weight seed) through the 256 / 299 ingest; beside it the largest stored
# activation of the fp32 run.  tests/test_fid.py recomputes both; the worst value sets the device's bar in tests/test_fid_gpu.py.
EMU_FULL_BY_SEED = (1.303e-4, 1.557e-4, 1.417e-4)
MAX_ACT_BY_SEED = (6.858, 11.473, 8.588)
EMU_FULL = max(EMU_FULL_BY_SEED)


def structured_images(n, h, w, seed=0):
    """uint8 [n, h, w, 3]: 8 x 8 blocks + noise, structure at several scales (any h, w)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n, (h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(base, 8, 1), 8, 2)[:, :h, :w].astype(np.int64) + rng.integers(-40, 41, (n, h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _r16(x, emulate):
    return x.half().float() if emulate else x


def loader(images, crop=256):
    """uint8 HWC images (one size) -> uint8 [N, crop, crop, 3]: torchvision's Resize(crop, LANCZOS) + CenterCrop(crop) done with Pillow."""
    from PIL import Image
    out = []
    for im in images:
        im = Image.fromarray(np.asarray(im))
        w, h = im.size
        short, long = (w, h) if w <= h else (h, w)
        if short != crop:                                        # Resize(int) returns the image itself when the shorter edge fits
            new_long = int(crop * long / short)
            im = im.resize((crop, new_long) if w <= h else (new_long, crop), Image.LANCZOS)
        w, h = im.size
        top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
        out.append(np.array(im.crop((left, top, left + crop, top + crop))))
    return np.stack(out)


def network_input(u8, size=299):
    """uint8 [N, S, S, 3] -> fp32 NCHW in [-1, 1]: ToTensor, the network's bilinear resize (size = 0: none), 2 x - 1."""
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255
    if size:
        x = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False)
    return 2 * x - 1


class Net:
    def __init__(self, weights, emulate=False):
        self.p, self.emulate = weights, emulate
        self.max_abs = 0.0                                       # the largest stored activation of the last run

    def conv(self, name, x, stride=1, padding=0):
        if name in self.p:
            w, b = self.p[name]
            y = F.conv2d(x, w, b, stride=stride, padding=padding)
        else:
            g = lambda k: self.p[f"{name}.bn.{k}"]
            y = F.conv2d(x, self.p[name + ".conv.weight"], None, stride=stride, padding=padding)
            y = F.batch_norm(y, g("running_mean"), g("running_var"), g("weight"), g("bias"), training=False, eps=1e-3)
        y = _r16(F.relu(y), self.emulate)
        self.max_abs = max(self.max_abs, float(y.abs().max()))
        return y

    def avg(self, x):
        return _r16(F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False), self.emulate)

    def a(self, n, x):
        c = lambda k, x, **kw: self.conv(f"{n}.{k}", x, **kw)
        b1 = c("branch1x1", x)
        b5 = c("branch5x5_2", c("branch5x5_1", x), padding=2)
        b3 = c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x), padding=1), padding=1)
        return torch.cat([b1, b5, b3, c("branch_pool", self.avg(x))], 1)

    def b(self, n, x):
        c = lambda k, x, **kw: self.conv(f"{n}.{k}", x, **kw)
        b3 = c("branch3x3", x, stride=2)
        bd = c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x), padding=1), stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, stride=2)], 1)

    def c(self, n, x):
        c = lambda k, x, **kw: self.conv(f"{n}.{k}", x, **kw)
        h, v = dict(padding=(0, 3)), dict(padding=(3, 0))        # (1, 7) and (7, 1) kernels
        b1 = c("branch1x1", x)
        b7 = c("branch7x7_3", c("branch7x7_2", c("branch7x7_1", x), **h), **v)
        bd = c("branch7x7dbl_1", x)
        bd = c("branch7x7dbl_3", c("branch7x7dbl_2", bd, **v), **h)
        bd = c("branch7x7dbl_5", c("branch7x7dbl_4", bd, **v), **h)
        return torch.cat([b1, b7, bd, c("branch_pool", self.avg(x))], 1)

    def d(self, n, x):
        c = lambda k, x, **kw: self.conv(f"{n}.{k}", x, **kw)
        b3 = c("branch3x3_2", c("branch3x3_1", x), stride=2)
        b7 = c("branch7x7x3_3", c("branch7x7x3_2", c("branch7x7x3_1", x), padding=(0, 3)), padding=(3, 0))
        b7 = c("branch7x7x3_4", b7, stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, stride=2)], 1)

    def e(self, n, x, pool):
        c = lambda k, x, **kw: self.conv(f"{n}.{k}", x, **kw)
        h, v = dict(padding=(0, 1)), dict(padding=(1, 0))        # (1, 3) and (3, 1) kernels
        b1 = c("branch1x1", x)
        b3 = c("branch3x3_1", x)
        b3 = torch.cat([c("branch3x3_2a", b3, **h), c("branch3x3_2b", b3, **v)], 1)
        bd = c("branch3x3dbl_2", c("branch3x3dbl_1", x), padding=1)
        bd = torch.cat([c("branch3x3dbl_3a", bd, **h), c("branch3x3dbl_3b", bd, **v)], 1)
        pooled = self.avg(x) if pool == "avg" else F.max_pool2d(x, 3, stride=1, padding=1)
        return torch.cat([b1, b3, bd, c("branch_pool", pooled)], 1)

    @torch.no_grad()
    def blocks(self, x):
        """fp32 NCHW network input -> the four block outputs of pytorch-fid (fp32 NCHW x 3, and the pooled [N, dims])."""
        self.max_abs = 0.0
        x = _r16(x, self.emulate)
        x = self.conv("Conv2d_2b_3x3", self.conv("Conv2d_2a_3x3", self.conv("Conv2d_1a_3x3", x, stride=2)), padding=1)
        t0 = x = F.max_pool2d(x, 3, stride=2)
        x = self.conv("Conv2d_4a_3x3", self.conv("Conv2d_3b_1x1", x))
        t1 = x = F.max_pool2d(x, 3, stride=2)
        for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = self.a(n, x)
        x = self.b("Mixed_6a", x)
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self.c(n, x)
        t2 = x
        x = self.d("Mixed_7a", x)
        x = self.e("Mixed_7c", self.e("Mixed_7b", x, "avg"), "max")
        return [t0, t1, t2, x.mean(dim=(2, 3))]


def features(weights, images, crop=256, size=299, emulate=False, batch=16):
    """uint8 HWC images of one size -> fp32 [N, dims] through the loader, the resize and the network."""
    net, out = Net(weights, emulate), []
    for i in range(0, len(images), batch):
        u8 = loader(images[i:i + batch], crop) if crop else np.stack(images[i:i + batch])
        out.append(net.blocks(network_input(u8, size))[-1])
    return torch.cat(out)


def frechet_eig(mu1, s1, mu2, s2):
    """The Frechet distance by the eigenvalue route: tr sqrt(S1 S2) = sum sqrt(eig(S1^1/2 S2 S1^1/2)), symmetric problems only."""
    mu1, mu2, s1, s2 = (np.asarray(a, np.float64) for a in (mu1, mu2, s1, s2))
    lam, q = np.linalg.eigh(s1)
    root = (q * np.sqrt(np.clip(lam, 0, None))) @ q.T
    ev = np.linalg.eigvalsh(root @ s2 @ root)
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.clip(ev, 0, None)).sum())
