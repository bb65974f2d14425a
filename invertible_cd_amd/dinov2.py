"""DINOv2 image encoder (the reference's preservation metric, utils/metrics.py calc_dinov2_images_images) on the HIP kernels of this package.

Drop-in for what the reference calls on `AutoModel.from_pretrained('facebook/dinov2-base')` behind its `AutoImageProcessor`:
    model(**processor(images=..., return_tensors='pt')).pooler_output          utils/metrics.py:176-207      -> [B, 768]

Architecture (transformers.Dinov2Model; the tests run the real class as the oracle): a 14 x 14 patch convolution, a class token and a
position table trained on a 37 x 37 grid that is bicubically resized to the grid of the image at hand, N pre-LayerNorm blocks of
multi-head self-attention and an erf-GELU MLP whose two branch outputs are multiplied by learned per-channel LayerScale vectors before
they join the residual stream, a final LayerNorm, class-token pooling.  There is no LayerNorm in front of the blocks: the embeddings are
the start of the residual stream.

Everything that does not depend on the image is folded on the host, once, at load time:
  * LayerScale: lambda1 of layer_scale1 scales the rows and the bias of attention.output.dense (the V bias leaves through that bias, as in
    clip.py), lambda1 of layer_scale2 those of mlp.fc2 - in float64, rounded to the storage type afterwards (encoder.fold_output).  No
    LayerScale pass runs.
  * the position table is resized to (crop_size / patch_size)^2 by upstream's own `torch.nn.functional.interpolate` call (fp32, bicubic,
    align_corners=False), so the table is upstream's bit for bit; nothing is interpolated when the grids agree.
  * one fp32 token table tok [1 + n, C]: row 0 = cls_token + position 0, row 1 + p = position p + patch bias.
On the device: `icd_clip_preprocess` at resize 256 / crop 224 with the ImageNet constants (transformers.BitImageProcessor), the patch
GEMM with fp32 output, `icd_vit_tokens` (adds the table, writes the fp16 stream and its fp32 twin), then the blocks of encoder.py, which
the CLIP towers run too.
"""
from dataclasses import dataclass, asdict
from types import SimpleNamespace

import torch

from . import ops
from .encoder import ModelOutput, check_state_dict, check_widths, fold_output, full, half, images_to_device, prepare_block, run_blocks
from .resample import IMAGENET_MEAN, IMAGENET_STD


@dataclass(frozen=True)
class Dinov2Config:
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    mlp_ratio: int = 4
    image_size: int = 518            # the resolution the position table was trained at (37 x 37 patches), not the input's
    patch_size: int = 14
    num_channels: int = 3
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-6
    qkv_bias: bool = True
    use_swiglu_ffn: bool = False
    crop_size: int = 224             # preprocessor_config.json: centre crop ...
    resize_shortest_edge: int = 256  # ... of the image whose shortest edge was resized to this

    def to_dict(self):
        return asdict(self)

    @property
    def intermediate_size(self):
        return int(self.hidden_size * self.mlp_ratio)

    @property
    def num_positions(self):
        """rows of the stored position table: the trained grid and the class token."""
        return (self.image_size // self.patch_size) ** 2 + 1

    @property
    def num_tokens(self):
        """tokens of one preprocessed image: the crop's grid and the class token."""
        return (self.crop_size // self.patch_size) ** 2 + 1

    def state_dict_shapes(self):
        """keys -> shapes of transformers.Dinov2Model (without embeddings.mask_token, which only pre-training reads)."""
        C, I, P = self.hidden_size, self.intermediate_size, self.patch_size
        out = {"embeddings.cls_token": (1, 1, C), "embeddings.position_embeddings": (1, self.num_positions, C),
               "embeddings.patch_embeddings.projection.weight": (C, self.num_channels, P, P),
               "embeddings.patch_embeddings.projection.bias": (C,)}
        for i in range(self.num_hidden_layers):
            p = f"encoder.layer.{i}."
            out[p + "norm1.weight"] = (C,); out[p + "norm1.bias"] = (C,)
            for n in ("query", "key", "value"):
                out[p + f"attention.attention.{n}.weight"] = (C, C)
                if self.qkv_bias:
                    out[p + f"attention.attention.{n}.bias"] = (C,)
            out[p + "attention.output.dense.weight"] = (C, C); out[p + "attention.output.dense.bias"] = (C,)
            out[p + "layer_scale1.lambda1"] = (C,)
            out[p + "norm2.weight"] = (C,); out[p + "norm2.bias"] = (C,)
            out[p + "mlp.fc1.weight"] = (I, C); out[p + "mlp.fc1.bias"] = (I,)
            out[p + "mlp.fc2.weight"] = (C, I); out[p + "mlp.fc2.bias"] = (C,)
            out[p + "layer_scale2.lambda1"] = (C,)
        out["layernorm.weight"] = (C,); out["layernorm.bias"] = (C,)
        return out


DINOV2_BASE = Dinov2Config()                                                         # facebook/dinov2-base


def _canon(sd):
    return {(k[len("dinov2."):] if k.startswith("dinov2.") else k): v for k, v in sd.items()}


def fold_layer_scale(weight, bias, lam, v_bias=None):
    """float64 (W', b') with W' x + b' = lam * (W (x + v_bias) + b): encoder.fold_output under the name and argument order it had here."""
    return fold_output(weight, bias, v_bias, lam)


def position_table(pos, grid):
    """stored position table [1, 1 + g0 * g0, C] fp32 -> its patch rows on a grid x grid image, [grid * grid, C]: upstream's
    Dinov2Embeddings.interpolate_pos_encoding (the same interpolate call on the same layout), or the stored rows when g0 == grid."""
    n0, dim = pos.shape[1] - 1, pos.shape[2]
    g0 = int(n0 ** 0.5)
    if g0 * g0 != n0:
        raise ValueError(f"Dinov2Model: the position table holds {n0} patch rows, which is no square grid")
    patch = pos[:, 1:]
    if g0 == grid:
        return patch[0]
    patch = patch.reshape(1, g0, g0, dim).permute(0, 3, 1, 2)
    patch = torch.nn.functional.interpolate(patch.to(torch.float32), size=(grid, grid), mode="bicubic", align_corners=False)
    return patch.permute(0, 2, 3, 1).reshape(-1, dim)


class Dinov2Model:
    def __init__(self, cfg: Dinov2Config, state_dict, device="cuda", dtype=torch.float16):
        if cfg.use_swiglu_ffn:
            raise ValueError("Dinov2Model: use_swiglu_ffn (the giant model's feed-forward) is not supported")
        check_widths("Dinov2Model", cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.hidden_act)
        if cfg.num_channels != 3 or cfg.image_size % cfg.patch_size or cfg.crop_size % cfg.patch_size or cfg.crop_size % 4 \
                or cfg.resize_shortest_edge < cfg.crop_size:
            raise ValueError("Dinov2Model: 3 channels, image and crop sizes multiples of the patch size, the crop a multiple of 4 and no "
                             "larger than the resized shortest edge")
        self.cfg = cfg
        self.device, self.dtype = torch.device(device), dtype
        self.config = SimpleNamespace(**cfg.to_dict())
        sd = _canon(state_dict)                                 # embeddings.mask_token, if present, is not read
        want = cfg.state_dict_shapes()
        check_state_dict(sd, want, "DINOv2")
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32) if k in want else None   # a q/k/v bias is read only under qkv_bias
        C = cfg.hidden_size
        kp = 3 * cfg.patch_size ** 2
        wp = torch.zeros((C, (kp + 7) // 8 * 8))                 # icd_gemm needs K % 8 == 0: pad columns are zero here and in the patch matrix
        wp[:, :kp] = f32("embeddings.patch_embeddings.projection.weight").reshape(C, kp)
        pos = f32("embeddings.position_embeddings")
        tok = torch.empty((cfg.num_tokens, C))
        tok[0] = f32("embeddings.cls_token")[0, 0] + pos[0, 0]
        tok[1:] = position_table(pos, cfg.crop_size // cfg.patch_size) + f32("embeddings.patch_embeddings.projection.bias")
        w = {"patch.w": half(wp, device), "tok": full(tok, device)}
        self.blocks = [f"encoder.layer.{i}." for i in range(cfg.num_hidden_layers)]
        for p in self.blocks:
            a = p + "attention.attention."
            names = {"q": a + "query", "k": a + "key", "v": a + "value", "out": p + "attention.output.dense", "norm1": p + "norm1",
                     "norm2": p + "norm2", "fc1": p + "mlp.fc1", "fc2": p + "mlp.fc2"}
            w.update((p + k, t) for k, t in prepare_block(f32, names, device, lam1=f32(p + "layer_scale1.lambda1"),
                                                          lam2=f32(p + "layer_scale2.lambda1")).items())
        w["ln_f.w"], w["ln_f.b"] = full(f32("layernorm.weight"), device), full(f32("layernorm.bias"), device)
        self.w = w

    def eval(self):
        return self

    def to(self, *args, **kw):
        return self

    def preprocess(self, images):
        """uint8 NHWC images -> the patch matrix [B * n_patches, pad8(3 * patch^2)] (transformers.BitImageProcessor on the device:
        shortest edge to resize_shortest_edge, centre crop, ImageNet mean / std)."""
        cfg = self.cfg
        return ops.clip_preprocess(images_to_device(images, self.device), size=cfg.resize_shortest_edge, crop=cfg.crop_size,
                                   patch=cfg.patch_size, mean=IMAGENET_MEAN, std=IMAGENET_STD)

    @torch.no_grad()
    def forward_patches(self, patches, output_hidden_states=False):
        """patch matrix of `preprocess` -> pooler_output fp32 [B, C] (and the L + 1 hidden states, the embeddings first, when asked)."""
        cfg, w = self.cfg, self.w
        C, H, T = cfg.hidden_size, cfg.num_attention_heads, cfg.num_tokens
        n = T - 1
        if patches.dim() != 2 or patches.shape[0] % n or patches.shape[1] != w["patch.w"].shape[1]:
            raise ValueError(f"Dinov2Model: patch matrix must be [B * {n}, {w['patch.w'].shape[1]}], got {tuple(patches.shape)}")
        B = patches.shape[0] // n
        # no LayerNorm precedes the blocks: the embeddings start the residual stream, so its fp32 twin starts here too
        x, x32 = ops.vit_tokens(ops.gemm(patches, w["patch.w"], out_f32=True), w["tok"], B)
        hs = [x]
        x, _ = run_blocks(w, self.blocks, x, x32, B, T, H, cfg.layer_norm_eps, cfg.hidden_act, False, hs)
        tok0 = x.reshape(B, T, C)[:, 0].contiguous()           # only the class token is pooled
        pooled = ops.layernorm(tok0, w["ln_f.w"], w["ln_f.b"], cfg.layer_norm_eps).float()
        if output_hidden_states:
            return pooled, tuple(h.reshape(B, T, C) for h in hs)
        return pooled

    def __call__(self, images, output_hidden_states=False):
        out = self.forward_patches(self.preprocess(images), output_hidden_states)
        if output_hidden_states:
            return ModelOutput(out[0], pooler_output=out[0], hidden_states=out[1])
        return ModelOutput(out, pooler_output=out)

    def get_image_features(self, images):
        """what metrics._image_features calls on either encoder: fp32 [B, C] on the device."""
        return self.forward_patches(self.preprocess(images))
