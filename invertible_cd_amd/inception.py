"""The FID Inception-v3 (the reference's utils/inception.py, pytorch-fid's `pt_inception-2015-12-05`) on the HIP kernels of this package.

What the reference runs per image, restated (`torchvision` and `pytorch-fid` are no dependencies, this list is the
definition the tests hold the module to):
    1. the loader of utils/metrics.py get_activations: Resize(256, LANCZOS) (shorter edge to 256, the longer one to int(256 long / short),
       Pillow's antialiased Lanczos on uint8), CenterCrop(256), ToTensor (u / 255);
    2. F.interpolate(x, (299, 299), mode='bilinear', align_corners=False), then 2 x - 1;
    3. BasicConv2d = conv without bias -> BatchNorm(eps 1e-3, running statistics) -> ReLU everywhere;
       stem Conv2d_1a_3x3 (3 -> 32, k3 s2), 2a (32 -> 32, k3), 2b (32 -> 64, k3 p1), maxpool k3 s2, 3b (64 -> 80, k1), 4a (80 -> 192, k3),
       maxpool k3 s2; Mixed_5b/5c/5d (InceptionA), 6a (B), 6b..6e (C), 7a (D), 7b/7c (E), as `_blocks` below spells them out, with the
       FID variants: the average pools of A, C and 7b divide by the taps inside the image (count_include_pad=False), 7c pools with a
       MAXIMUM (k3 s1 p1);
    4. global average pool -> [N, 2048].

On the device: `icd_fid_ingest` (steps 1 and 2, the Lanczos pass bit for bit), one `icd_conv2d` per BasicConv2d (BatchNorm folded into
the fp16 weight and an fp32 bias at load, in float64, rounded once; ReLU in the epilogue), `icd_pool3x3`, `icd_global_avgpool`.  Every
branch of a block stores straight into its column slice of the block's output: no concat pass exists.  No torch convolution runs here.
"""
from dataclasses import dataclass

import torch

from . import _lib, ops
from .encoder import check_state_dict, image_batch_to_device, image_size, mixed_sizes, run_by_size

BN_EPS = 1e-3
MAX_S2, MAX_S1P1, AVG = "max_s2", "max_s1p1", "avg"
_POOL = {MAX_S2: _lib.ICD_POOL_MAX_S2, MAX_S1P1: _lib.ICD_POOL_MAX_S1P1, AVG: _lib.ICD_POOL_AVG_S1P1}


def _c(name, cout, k=(1, 1), s=1, p=(0, 0)):
    return (name, cout, k, s, p)


def _a(pf):
    return [[_c("branch1x1", 64)],
            [_c("branch5x5_1", 48), _c("branch5x5_2", 64, (5, 5), 1, (2, 2))],
            [_c("branch3x3dbl_1", 64), _c("branch3x3dbl_2", 96, (3, 3), 1, (1, 1)), _c("branch3x3dbl_3", 96, (3, 3), 1, (1, 1))],
            [AVG, _c("branch_pool", pf)]]


def _b():
    return [[_c("branch3x3", 384, (3, 3), 2)],
            [_c("branch3x3dbl_1", 64), _c("branch3x3dbl_2", 96, (3, 3), 1, (1, 1)), _c("branch3x3dbl_3", 96, (3, 3), 2)],
            [MAX_S2]]


def _cc(c7):
    h, v = ((1, 7), 1, (0, 3)), ((7, 1), 1, (3, 0))
    return [[_c("branch1x1", 192)],
            [_c("branch7x7_1", c7), _c("branch7x7_2", c7, *h), _c("branch7x7_3", 192, *v)],
            [_c("branch7x7dbl_1", c7), _c("branch7x7dbl_2", c7, *v), _c("branch7x7dbl_3", c7, *h), _c("branch7x7dbl_4", c7, *v),
             _c("branch7x7dbl_5", 192, *h)],
            [AVG, _c("branch_pool", 192)]]


def _d():
    return [[_c("branch3x3_1", 192), _c("branch3x3_2", 320, (3, 3), 2)],
            [_c("branch7x7x3_1", 192), _c("branch7x7x3_2", 192, (1, 7), 1, (0, 3)), _c("branch7x7x3_3", 192, (7, 1), 1, (3, 0)),
             _c("branch7x7x3_4", 192, (3, 3), 2)],
            [MAX_S2]]


def _e(pool):
    h, v = ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0))
    return [[_c("branch1x1", 320)],
            [_c("branch3x3_1", 384), (_c("branch3x3_2a", 384, *h), _c("branch3x3_2b", 384, *v))],
            [_c("branch3x3dbl_1", 448), _c("branch3x3dbl_2", 384, (3, 3), 1, (1, 1)),
             (_c("branch3x3dbl_3a", 384, *h), _c("branch3x3dbl_3b", 384, *v))],
            [pool, _c("branch_pool", 192)]]


# A block is a list of branches, a branch a list of steps, a step a pool mode, a convolution (name, cout, (kh, kw), stride, (ph, pw)) or -
# last in its branch - a tuple of convolutions that read the same tensor and are concatenated.
_STEM = ([_c("Conv2d_1a_3x3", 32, (3, 3), 2), _c("Conv2d_2a_3x3", 32, (3, 3)), _c("Conv2d_2b_3x3", 64, (3, 3), 1, (1, 1)), MAX_S2],
         [_c("Conv2d_3b_1x1", 80), _c("Conv2d_4a_3x3", 192, (3, 3)), MAX_S2])
_BLOCKS = (("Mixed_5b", _a(32)), ("Mixed_5c", _a(64)), ("Mixed_5d", _a(64)), ("Mixed_6a", _b()), ("Mixed_6b", _cc(128)),
           ("Mixed_6c", _cc(160)), ("Mixed_6d", _cc(160)), ("Mixed_6e", _cc(192)), ("Mixed_7a", _d()), ("Mixed_7b", _e(AVG)),
           ("Mixed_7c", _e(MAX_S1P1)))
_TAP_AFTER = "Mixed_6e"                           # the third block output of pytorch-fid (768 x 17 x 17)


@dataclass(frozen=True)
class InceptionConfig:
    div: int = 1            # every width of the network is ceil(width / div) rounded up to a multiple of 8 (1: the real network)
    crop: int = 256         # Resize(crop, LANCZOS) + CenterCrop(crop) of the loader; 0: square images are taken as they are
    size: int = 299         # the network's own bilinear resize; 0: none (the network runs at the crop's, or the images', size)

    def width(self, c):
        return c if self.div == 1 else (-(-c // self.div) + 7) // 8 * 8

    def convs(self):
        """{conv name: (cout, cin, kh, kw, stride, ph, pw)} in network order, widths as this configuration scales them."""
        out = {}

        def conv(prefix, step, cin):
            name, cout, k, s, p = step
            out[prefix + name] = (self.width(cout), cin, k[0], k[1], s, p[0], p[1])
            return self.width(cout)
        c = 3
        for seq in _STEM:
            for step in seq:
                c = conv("", step, c) if not isinstance(step, str) else c
        for bname, branches in _BLOCKS:
            total = 0
            for branch in branches:
                bc = c
                for step in branch:
                    if isinstance(step, str):
                        continue
                    if isinstance(step[0], tuple):
                        bc = sum(conv(bname + ".", s, bc) for s in step)
                    else:
                        bc = conv(bname + ".", step, bc)
                total += bc
            c = total
        return out

    @property
    def dims(self):
        """width of the pooled features (Mixed_7c's concat)"""
        return self.width(320) + 4 * self.width(384) + self.width(192)

    def state_dict_shapes(self):
        out = {}
        for name, (cout, cin, kh, kw, *_) in self.convs().items():
            out[name + ".conv.weight"] = (cout, cin, kh, kw)
            for k in ("weight", "bias", "running_mean", "running_var"):
                out[f"{name}.bn.{k}"] = (cout,)
        return out


FID_INCEPTION = InceptionConfig()
# the tests' network: every convolution 8 wide, all eleven blocks with their 5 x 5, 1 x 7 / 7 x 1 and 1 x 3 / 3 x 1 layers, 48 features
FID_INCEPTION_REDUCED = InceptionConfig(div=64)


def fold_batchnorm(weight, gamma, beta, mean, var, eps=BN_EPS):
    """(W', b') in float64 with relu(W' * x + b') = relu(BatchNorm(W * x)) for running statistics: W' = W gamma / sqrt(var + eps) per
    output channel, b' = beta - mean gamma / sqrt(var + eps).  The caller rounds once (fp16 weight, fp32 bias), as encoder.fold_output's
    callers do."""
    d = torch.float64
    scale = gamma.to(d) / torch.sqrt(var.to(d) + eps)
    return weight.to(d) * scale.reshape(-1, 1, 1, 1), beta.to(d) - mean.to(d) * scale


def folded_weights(cfg, state_dict):
    """{conv name: (weight [O, I, kh, kw] rounded to fp16, kept as fp32; bias fp32)} on the host: exactly the numbers the device model
    multiplies with (the tests build their oracle from it)."""
    sd = {k: v for k, v in state_dict.items() if not k.startswith("fc.") and not k.endswith("num_batches_tracked")}
    check_state_dict(sd, cfg.state_dict_shapes(), "Inception")
    out = {}
    for name in cfg.convs():
        f = lambda k: sd[name + k].detach().to("cpu", torch.float32)
        w, b = fold_batchnorm(f(".conv.weight"), f(".bn.weight"), f(".bn.bias"), f(".bn.running_mean"), f(".bn.running_var"))
        out[name] = (w.to(torch.float16).float(), b.float())
    return out


class FidInception:
    def __init__(self, cfg: InceptionConfig, state_dict, device="cuda"):
        if cfg.div < 1 or cfg.crop < 0 or cfg.crop % 4 or cfg.size < 0:
            raise ValueError(f"FidInception: div must be >= 1, crop a non-negative multiple of 4, size non-negative, got {cfg}")
        self.cfg, self.device = cfg, torch.device(device)
        self.geom = cfg.convs()
        self.w = {}                                              # name -> (packed fp16 [O, kh * kw * Cin'], fp32 bias)
        for name, (w, b) in folded_weights(cfg, state_dict).items():
            self.w[name] = (ops.pack_conv_weight_hw(w).to(self.device).contiguous(), b.to(self.device).contiguous())

    def eval(self):
        return self

    def to(self, *args, **kw):
        return self

    # ------------------------------------------------------------------------------------------------------- front end
    def ingest(self, images):
        """PIL images / numpy uint8 HWC arrays / a stacked uint8 NHWC array or tensor (one size) ->
        (fp16 [B * s * s, 8] network input, uint8 [B, crop, crop, 3] the loader's output, B, s)."""
        t = image_batch_to_device(images, self.device)
        cfg = self.cfg
        if not cfg.crop and t.shape[1] != t.shape[2]:
            raise ValueError(f"FidInception: crop = 0 takes square images, got {tuple(t.shape[1:3])}")
        s = cfg.size or cfg.crop or t.shape[1]
        x, mid = ops.fid_ingest(t, cfg.crop, s)
        return x, mid, t.shape[0], s

    # ------------------------------------------------------------------------------------------------------- the network
    def _conv(self, name, x, B, H, W, out=None, col_off=0):
        _, _, kh, kw, s, ph, pw = self.geom[name]
        w, b = self.w[name]
        y = ops.conv2d(x, B, H, W, w, b, kh, kw, s, ph, pw, relu=True, out=out, col_off=col_off)
        return (y,) + ops.conv2d_out_size(H, W, kh, kw, s, ph, pw)

    @staticmethod
    def _pool_size(mode, H, W):
        return ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == MAX_S2 else (H, W)

    def _block(self, bname, branches, x, B, H, W):
        cin = x.shape[1]
        widths = []
        for branch in branches:
            last = branch[-1]
            widths.append(cin if isinstance(last, str) else sum(self.geom[f"{bname}.{s[0]}"][0] for s in (last if isinstance(last[0], tuple)
                                                                                                              else (last,))))
        out, off, Ho, Wo = None, 0, H, W
        for branch, width in zip(branches, widths):
            y, h, w = x, H, W
            for i, step in enumerate(branch):
                final = i + 1 == len(branch)
                if final:
                    Ho, Wo = self._pool_size(step, h, w) if isinstance(step, str) else \
                        ops.conv2d_out_size(h, w, *[self.geom[f"{bname}.{(step[0] if isinstance(step[0], tuple) else step)[0]}"][j]
                                                    for j in (2, 3, 4, 5, 6)])
                    if out is None:
                        out = torch.empty((B * Ho * Wo, sum(widths)), device=x.device, dtype=torch.float16)
                if isinstance(step, str):
                    y = ops.pool3x3(y, B, h, w, _POOL[step], out=out if final else None, col_off=off if final else 0)
                    h, w = self._pool_size(step, h, w)
                elif isinstance(step[0], tuple):                 # a fork: always the branch's last step
                    o = off
                    for s in step:
                        self._conv(f"{bname}.{s[0]}", y, B, h, w, out, o)
                        o += self.geom[f"{bname}.{s[0]}"][0]
                else:
                    y, h, w = self._conv(f"{bname}.{step[0]}", y, B, h, w, out if final else None, off if final else 0)
            off += width
        return out, Ho, Wo

    def _network(self, x, B, s):
        """fp16 [B * s * s, 8] -> the four block outputs of pytorch-fid: fp16 [B, h, w, C] x 3 and the pooled fp32 [B, dims]."""
        taps, H, W = [], s, s
        for seq in _STEM:
            for step in seq:
                if isinstance(step, str):
                    x = ops.pool3x3(x, B, H, W, _POOL[step])
                    H, W = self._pool_size(step, H, W)
                else:
                    x, H, W = self._conv(step[0], x, B, H, W)
            taps.append(x.reshape(B, H, W, -1))
        for bname, branches in _BLOCKS:
            x, H, W = self._block(bname, branches, x, B, H, W)
            if bname == _TAP_AFTER:
                taps.append(x.reshape(B, H, W, -1))
        taps.append(ops.global_avgpool(x, B, H * W))
        return taps

    @torch.no_grad()
    def _blocks_one_size(self, images):
        x, _, B, s = self.ingest(images)
        return self._network(x, B, s)

    def blocks(self, images):
        """The four block outputs (64 x 73^2, 192 x 35^2, 768 x 17^2 as fp16 NHWC, and the pooled fp32 [N, 2048]) of images of ONE size."""
        return self._blocks_one_size(images)

    def features(self, images):
        """fp32 [N, dims] on the device.  A list may mix image sizes: each size is ingested as one batch, the rows come back in the
        caller's order."""
        if not mixed_sizes(images):
            return self._blocks_one_size(images)[-1]
        items = list(images)
        return run_by_size(len(items), lambda i: image_size(items[i]), lambda idx: self._blocks_one_size([items[i] for i in idx])[-1])

    __call__ = features
