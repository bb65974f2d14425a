"""LPIPS (the reference's third preservation figure, utils/metrics.py calculate_lpips) on the HIP kernels of this package.

Drop-in for what the reference calls as `piq.LPIPS(reduction='none')(x, y)` on `np.array(img.resize((224, 224)))` / 255:
    1. (x - mean) / std with the ImageNet constants;
    2. torchvision's vgg16().features: 3 x 3 convolutions (padding 1, bias, ReLU) in blocks of 2, 2, 3, 3, 3 of widths 64, 128, 256,
       512, 512, MaxPool2d(2) in front of blocks 2 .. 5;
    3. taps after the last ReLU of each block (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3);
    4. each tap channel-normalised, f / (sqrt(sum_c f^2) + 1e-10);
    5. score = sum over taps of sum_c mean_hw((n1 - n2)^2 * w_tap[c]) with piq's non-negative `lpips_weights.pt`.
`piq` is not a dependency: the list above is the definition the tests hold this module to.

On the device both image sets run as one batch of 2 N: `icd_image_resize_norm` (Pillow's BICUBIC stretch to size x size, bit for bit,
normalise, NHWC fp16 with Cin padded from 3 to 8), 13 x `ops.conv3x3` with bias, `icd_relu` after the eight convolutions that are
no tap, and - because ReLU commutes with a maximum - no ReLU pass for the five taps: `icd_maxpool2x2(relu=1)` and
`icd_lpips_layer(relu=1)` apply it on load.  The five `icd_lpips_layer` launches accumulate into one fp32 [N].  No torch
convolution runs here.
"""
from dataclasses import dataclass

import torch

from . import ops
from .encoder import check_state_dict, image_batch_to_device, image_size, mixed_sizes, run_by_size
from .resample import IMAGENET_MEAN, IMAGENET_STD


@dataclass(frozen=True)
class LpipsConfig:
    widths: tuple = (64, 128, 256, 512, 512)
    convs: tuple = (2, 2, 3, 3, 3)
    size: int = 224
    mean: tuple = IMAGENET_MEAN
    std: tuple = IMAGENET_STD

    def conv_keys(self):
        """'features.<i>' of every convolution, in order: torchvision's numbering (a ReLU after each conv, a pool after each block)."""
        keys, i = [], 0
        for n in self.convs:
            for _ in range(n):
                keys.append(f"features.{i}")
                i += 2
            i += 1
        return keys

    def state_dict_shapes(self):
        out, cin = {}, 3
        keys = iter(self.conv_keys())
        for width, n in zip(self.widths, self.convs):
            for _ in range(n):
                k = next(keys)
                out[k + ".weight"], out[k + ".bias"] = (width, cin, 3, 3), (width,)
                cin = width
        return out


LPIPS_VGG16 = LpipsConfig()


class Lpips:
    def __init__(self, cfg: LpipsConfig, vgg_state_dict, lin_weights, device="cuda"):
        if len(cfg.widths) != len(cfg.convs) or not cfg.widths or min(cfg.convs) < 1:
            raise ValueError("Lpips: widths and convs must name the same (non-zero) number of blocks, every block at least one conv")
        if any(w <= 0 or w % 8 for w in cfg.widths):
            raise ValueError(f"Lpips: block widths must be positive multiples of 8, got {cfg.widths}")
        if cfg.size <= 0 or cfg.size % 4 or cfg.size >> (len(cfg.widths) - 1) < 1:
            raise ValueError(f"Lpips: size must be a multiple of 4 that survives {len(cfg.widths) - 1} poolings, got {cfg.size}")
        self.cfg, self.device = cfg, torch.device(device)
        sd = vgg_state_dict
        check_state_dict(sd, cfg.state_dict_shapes(), "VGG16")
        if len(lin_weights) != len(cfg.widths):
            raise ValueError(f"Lpips: {len(cfg.widths)} lin weights expected, got {len(lin_weights)}")
        f32 = lambda t: t.detach().to("cpu", torch.float32)
        self.convs = []                                          # per block: [(packed fp16 weight [O, 9 * Cin], fp32 bias)]
        keys = iter(cfg.conv_keys())
        for n in cfg.convs:
            block = []
            for _ in range(n):
                k = next(keys)
                w = f32(sd[k + ".weight"])
                if w.shape[1] == 3:                              # Cin 3 -> 8 with zeros: K = 72, as the VAE encoder's conv_in
                    w8 = torch.zeros(w.shape[0], 8, 3, 3)
                    w8[:, :3] = w
                    w = w8
                block.append((ops.pack_conv_weight(w).to(self.device).contiguous(), f32(sd[k + ".bias"]).to(self.device).contiguous()))
            self.convs.append(block)
        self.lin = []
        for i, (lw, width) in enumerate(zip(lin_weights, cfg.widths)):
            lw = f32(torch.as_tensor(lw))
            if lw.numel() != width:
                raise ValueError(f"Lpips: lin weight {i} holds {lw.numel()} values for a tap of {width} channels")
            self.lin.append(lw.reshape(width).to(self.device).contiguous())

    def eval(self):
        return self

    def to(self, *args, **kw):
        return self

    def ingest(self, images):
        """PIL images / numpy uint8 HWC arrays / a stacked uint8 NHWC array or tensor (one size) -> (fp16 [B * size * size, 8], B)."""
        t = image_batch_to_device(images, self.device)
        return ops.image_resize_norm(t, self.cfg.size, self.cfg.mean, self.cfg.std), t.shape[0]

    def _stack(self, x, B, tap):
        """The convolutions; tap(level, pre-ReLU output [B * s * s, width], s) is called once per block."""
        s = self.cfg.size
        for level, block in enumerate(self.convs):
            if level:
                x = ops.maxpool2x2(x, B, s, s, relu=True)        # relu(max) = max(relu): the tap in front needs no ReLU pass
                s //= 2
            for j, (w, b) in enumerate(block):
                x = ops.conv3x3(x, B, s, s, w, b)
                if j + 1 < len(block):
                    ops.relu(x, inplace=True)
            tap(level, x, s)

    @torch.no_grad()
    def features(self, images):
        """The five taps with ReLU applied: fp16 [B, s, s, width] each (NHWC)."""
        x, B = self.ingest(images)
        taps = []
        self._stack(x, B, lambda level, f, s: taps.append(ops.relu(f).reshape(B, s, s, f.shape[1])))
        return taps

    @torch.no_grad()
    def _pairs(self, images_1, images_2):
        x1, n = self.ingest(images_1)
        x2, n2 = self.ingest(images_2)
        if n != n2:
            raise ValueError(f"Lpips: {n} images against {n2}")
        out = torch.empty((n,), device=self.device, dtype=torch.float32)
        x = torch.cat([x1, x2])
        del x1, x2
        self._stack(x, 2 * n, lambda level, f, s: ops.lpips_layer(f, n, s * s, self.lin[level], out=out, relu=True, accumulate=level > 0))
        return out

    def forward(self, images_1, images_2):
        """fp32 [N] on the device.  A list may mix image sizes (each side of a pair is resized on its own): the pairs are ingested size by
        size and the scores come back in the caller's order."""
        if not mixed_sizes(images_1) and not mixed_sizes(images_2):
            return self._pairs(images_1, images_2)
        a, b = list(images_1), list(images_2)
        if len(a) != len(b):
            raise ValueError(f"Lpips: {len(a)} images against {len(b)}")
        return run_by_size(len(a), lambda i: (image_size(a[i]), image_size(b[i])),
                           lambda idx: self._pairs([a[i] for i in idx], [b[i] for i in idx]))

    __call__ = forward
