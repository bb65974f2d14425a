"""ImageReward (the reference's editing / generation score, utils/metrics.py calc_ir) on the HIP kernels of this package: the BLIP image
tower, the BLIP text tower that cross-attends to it, and the reward head.

Drop-in for what the reference calls on `RM.load("ImageReward-v1.0")`:
    model.score(prompt, [image])                                                   utils/metrics.py:283-293
which is  mlp(text_encoder(ids, mask, encoder_hidden_states=visual_encoder(image)).last_hidden_state[:, 0])  normalised by the package's
(mean, std).  Here `ImageReward.score(prompt_ids, attention_mask, images)` returns that for a whole batch, fp32 [B] on the device.

THE ARCHITECTURE IS TESTED AGAINST `transformers` (BlipVisionModel and BlipTextModel run as the oracle on seeded weights, and their
state-dict names are this module's); THE ImageReward PACKAGE'S OWN KEY NAMES (`blip.visual_encoder.*`, `blip.text_encoder.*`,
`mlp.layers.*`, translated by `translate_package_keys`) ARE UNVERIFIED: neither the package nor its checkpoint was at hand.

BlipVisionModel: a 16 x 16 patch convolution with bias, a class embedding, a position table of (image / patch)^2 + 1 rows, pre-LayerNorm
blocks with one fused qkv Linear, an erf-GELU MLP, post_layernorm over all tokens.  Built as dinov2.Dinov2Model is: qkv split into the
q | k and v pieces of encoder.prepare_block, the V bias folded into the projection's bias, one fp32 token table for icd_vit_tokens,
encoder.run_blocks.  Every LayerNorm of the tower, post_layernorm included, reads the fp32 twin of the stream (icd_layernorm_f32;
run_blocks' norm_f32), and q and k carry their fp16 rounding error into the scores (run_blocks' split_qk: icd_gemm's out_carry,
icd_attention_probs_split, P.V as a batched GEMM): on peaked attention rows the 24 blocks otherwise end at 1.15e-3 of the fp32 oracle,
above the project's 1e-3 bar.  Preprocessing is ImageReward's
Resize(224, BICUBIC) + CenterCrop(224) + CLIP's mean / std as icd_clip_preprocess: torchvision resizes the long edge to
int(224 * long / short), which is resample.clip_geometry's rule; its CenterCrop starts at round(margin / 2) where the kernel starts at
margin // 2, which differ when the margin is odd and its half rounds up (a margin of 3, 7, 11, ... pixels: one pixel of offset).

BlipTextModel (add_pooling_layer=False, is_decoder config, bidirectional self-attention): word + absolute position embeddings and
embeddings.LayerNorm, then post-LayerNorm layers of self-attention under the padding mask (icd_attention_masked: a per-sample key
count, so RIGHT PADDING IS REQUIRED and checked), cross-attention to the image tokens without a mask (icd_attention_fused) and an
erf-GELU feed-forward; each sublayer ends in LayerNorm(x + dense(...)).  The stream is fp32 between sublayers: the GEMM that ends a
sublayer adds the fp32 stream and writes the fp32 sum (icd_gemm_desc.resid / out_f32), icd_layernorm_f32 normalises it and writes the
fp16 copy the next GEMM reads and the fp32 copy the next sum reads - no fp16 rounding between a sum and its LayerNorm.  The V biases
are folded into the output projections (softmax rows sum to one), which needs at least one valid key per sample: an all-zero mask row is
refused.  The keys of all cross-attention layers come from one GEMM over the concatenated weights.

The head is five Linears with dropout between them and no activation: folded at load time, in float64, with (r - mean) / std, into one
vector w [768] and a scalar.
"""
from dataclasses import dataclass, asdict
from types import SimpleNamespace

import torch

from . import ops
from .encoder import (ModelOutput, check_state_dict, check_widths, fold_output, full, half, image_batch_to_device, image_size,
                      images_to_device, mixed_sizes, prepare_block, run_blocks, run_by_size)
from .resample import CLIP_MEAN, CLIP_STD

REWARD_MEAN = 0.16717362830052426            # the ImageReward package's normalisation constants
REWARD_STD = 1.0333394966054072
HEAD_LAYERS = (0, 2, 4, 6, 7)                # the Linears of the package's nn.Sequential (dropout between them)


# ------------------------------------------------------------------------------------------------------------ image tower
@dataclass(frozen=True)
class BlipVisionConfig:
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    image_size: int = 224
    patch_size: int = 16
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-6

    def to_dict(self):
        return asdict(self)

    @property
    def num_positions(self):
        return (self.image_size // self.patch_size) ** 2 + 1

    def state_dict_shapes(self):
        """keys -> shapes of transformers.BlipVisionModel"""
        C, I, P = self.hidden_size, self.intermediate_size, self.patch_size
        out = {"embeddings.class_embedding": (1, 1, C), "embeddings.position_embedding": (1, self.num_positions, C),
               "embeddings.patch_embedding.weight": (C, 3, P, P), "embeddings.patch_embedding.bias": (C,)}
        for i in range(self.num_hidden_layers):
            p = f"encoder.layers.{i}."
            out[p + "self_attn.qkv.weight"] = (3 * C, C); out[p + "self_attn.qkv.bias"] = (3 * C,)
            out[p + "self_attn.projection.weight"] = (C, C); out[p + "self_attn.projection.bias"] = (C,)
            out[p + "layer_norm1.weight"] = (C,); out[p + "layer_norm1.bias"] = (C,)
            out[p + "layer_norm2.weight"] = (C,); out[p + "layer_norm2.bias"] = (C,)
            out[p + "mlp.fc1.weight"] = (I, C); out[p + "mlp.fc1.bias"] = (I,)
            out[p + "mlp.fc2.weight"] = (C, I); out[p + "mlp.fc2.bias"] = (C,)
        out["post_layernorm.weight"] = (C,); out["post_layernorm.bias"] = (C,)
        return out


IMAGEREWARD_VISION = BlipVisionConfig()                                              # BLIP ViT-L/16 at 224


class BlipVisionModel:
    def __init__(self, cfg: BlipVisionConfig, state_dict, device="cuda", dtype=torch.float16):
        check_widths("BlipVisionModel", cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.hidden_act)
        if cfg.image_size % cfg.patch_size or cfg.image_size % 4:
            raise ValueError("BlipVisionModel: image size a multiple of the patch size and of 4")
        self.cfg = cfg
        self.device, self.dtype = torch.device(device), dtype
        self.config = SimpleNamespace(**cfg.to_dict())
        sd = state_dict
        check_state_dict(sd, cfg.state_dict_shapes(), "BLIP vision")
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
        C = cfg.hidden_size
        kp = 3 * cfg.patch_size ** 2
        wp = torch.zeros((C, (kp + 7) // 8 * 8))                 # icd_gemm needs K % 8 == 0 (3 * 16^2 already is one)
        wp[:, :kp] = f32("embeddings.patch_embedding.weight").reshape(C, kp)
        pos = f32("embeddings.position_embedding")
        tok = torch.empty((cfg.num_positions, C))
        tok[0] = f32("embeddings.class_embedding")[0, 0] + pos[0, 0]
        tok[1:] = pos[0, 1:] + f32("embeddings.patch_embedding.bias")
        w = {"patch.w": half(wp, device), "tok": full(tok, device)}
        self.blocks = [f"encoder.layers.{i}." for i in range(cfg.num_hidden_layers)]
        names = {"q": "q", "k": "k", "v": "v", "out": "self_attn.projection", "norm1": "layer_norm1", "norm2": "layer_norm2",
                 "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
        for p in self.blocks:
            qkv_w, qkv_b = f32(p + "self_attn.qkv.weight"), f32(p + "self_attn.qkv.bias")
            pieces = {f"{n}.{kind}": t[i * C:(i + 1) * C] for i, n in enumerate("qkv") for kind, t in (("weight", qkv_w), ("bias", qkv_b))}
            get = lambda k, p=p, pieces=pieces: pieces[k] if k in pieces else f32(p + k)
            w.update((p + k, t) for k, t in prepare_block(get, names, device).items())
        w["ln_post.w"], w["ln_post.b"] = full(f32("post_layernorm.weight"), device), full(f32("post_layernorm.bias"), device)
        self.w = w

    def eval(self):
        return self

    def to(self, *args, **kw):
        return self

    def preprocess(self, images):
        """uint8 NHWC images -> the patch matrix [B * n_patches, 3 * patch^2] (Resize(224, BICUBIC), CenterCrop(224), CLIP mean / std)."""
        cfg = self.cfg
        return ops.clip_preprocess(images_to_device(images, self.device), size=cfg.image_size, crop=cfg.image_size, patch=cfg.patch_size,
                                   mean=CLIP_MEAN, std=CLIP_STD)

    @torch.no_grad()
    def forward_patches(self, patches, output_hidden_states=False):
        """patch matrix of `preprocess` -> last_hidden_state fp16 [B, T, C] (and the L + 1 hidden states, the embeddings first, when asked)."""
        cfg, w = self.cfg, self.w
        C, H, T = cfg.hidden_size, cfg.num_attention_heads, cfg.num_positions
        n = T - 1
        if patches.dim() != 2 or patches.shape[0] % n or patches.shape[1] != w["patch.w"].shape[1]:
            raise ValueError(f"BlipVisionModel: patch matrix must be [B * {n}, {w['patch.w'].shape[1]}], got {tuple(patches.shape)}")
        B = patches.shape[0] // n
        x, x32 = ops.vit_tokens(ops.gemm(patches, w["patch.w"], out_f32=True), w["tok"], B)
        hs = [x]
        x, x32 = run_blocks(w, self.blocks, x, x32, B, T, H, cfg.layer_norm_eps, cfg.hidden_act, False, hs, norm_f32=True, split_qk=True)
        last, _ = ops.layernorm_f32(x32, w["ln_post.w"], w["ln_post.b"], cfg.layer_norm_eps, want32=False)
        last = last.reshape(B, T, C)
        if output_hidden_states:
            return last, tuple(h.reshape(B, T, C) for h in hs)
        return last

    def __call__(self, images, output_hidden_states=False):
        out = self.forward_patches(self.preprocess(images), output_hidden_states)
        if output_hidden_states:
            return ModelOutput(out[0], last_hidden_state=out[0], hidden_states=out[1])
        return ModelOutput(out, last_hidden_state=out)


# ------------------------------------------------------------------------------------------------------------ text tower
@dataclass(frozen=True)
class BlipTextConfig:
    vocab_size: int = 30524                  # bert-base-uncased and BLIP's [DEC], [ENC]
    hidden_size: int = 768
    encoder_hidden_size: int = 1024
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 512
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-12

    def to_dict(self):
        return asdict(self)

    def state_dict_shapes(self):
        """keys -> shapes of transformers.BlipTextModel(config with is_decoder=True, add_pooling_layer=False)"""
        C, E, I = self.hidden_size, self.encoder_hidden_size, self.intermediate_size
        out = {"embeddings.word_embeddings.weight": (self.vocab_size, C), "embeddings.position_embeddings.weight": (self.max_position_embeddings, C),
               "embeddings.LayerNorm.weight": (C,), "embeddings.LayerNorm.bias": (C,)}
        for i in range(self.num_hidden_layers):
            p = f"encoder.layer.{i}."
            for a, kv in (("attention", C), ("crossattention", E)):
                for n, k in (("query", C), ("key", kv), ("value", kv)):
                    out[p + f"{a}.self.{n}.weight"] = (C, k); out[p + f"{a}.self.{n}.bias"] = (C,)
                out[p + f"{a}.output.dense.weight"] = (C, C); out[p + f"{a}.output.dense.bias"] = (C,)
                out[p + f"{a}.output.LayerNorm.weight"] = (C,); out[p + f"{a}.output.LayerNorm.bias"] = (C,)
            out[p + "intermediate.dense.weight"] = (I, C); out[p + "intermediate.dense.bias"] = (I,)
            out[p + "output.dense.weight"] = (C, I); out[p + "output.dense.bias"] = (C,)
            out[p + "output.LayerNorm.weight"] = (C,); out[p + "output.LayerNorm.bias"] = (C,)
        return out


IMAGEREWARD_TEXT = BlipTextConfig()


def key_counts_of(attention_mask):
    """attention_mask [B, T] of ones followed by zeros (right padding) -> the number of ones per row, int64 [B] on the host.  Anything
    else - a zero before a one, an all-zero row, values other than 0 / 1 - is refused: the kernel knows a key COUNT per sample, and the
    folded V biases need at least one key."""
    m = torch.as_tensor(attention_mask).detach().cpu()
    if m.dim() != 2:
        raise ValueError(f"attention_mask must be [B, T], got {tuple(m.shape)}")
    m = m.to(torch.int64)
    if bool(((m != 0) & (m != 1)).any()):
        raise ValueError("attention_mask must hold zeros and ones only")
    counts = m.sum(1)
    if bool((m != (torch.arange(m.shape[1])[None, :] < counts[:, None])).any()):
        raise ValueError("attention_mask must be right-padded: in every row ones followed by zeros")
    if bool((counts == 0).any()):
        raise ValueError("attention_mask has an all-zero row: every sample needs at least one valid token")
    return counts


class BlipTextModel:
    def __init__(self, cfg: BlipTextConfig, state_dict, device="cuda", dtype=torch.float16):
        check_widths("BlipTextModel", cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.hidden_act,
                     extra=(cfg.encoder_hidden_size,))
        if cfg.hidden_size // cfg.num_attention_heads > 128 or cfg.hidden_size > 4096:
            raise ValueError("BlipTextModel: head dim <= 128 (icd_attention_masked) and hidden size <= 4096 (icd_layernorm_f32)")
        self.cfg = cfg
        self.device, self.dtype = torch.device(device), dtype
        self.config = SimpleNamespace(**cfg.to_dict())
        sd = state_dict
        check_state_dict(sd, cfg.state_dict_shapes(), "BLIP text")
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
        w = {"tok": half(f32("embeddings.word_embeddings.weight"), device), "pos": half(f32("embeddings.position_embeddings.weight"), device),
             "ln_e.w": full(f32("embeddings.LayerNorm.weight"), device), "ln_e.b": full(f32("embeddings.LayerNorm.bias"), device)}
        self.layers = [f"encoder.layer.{i}." for i in range(cfg.num_hidden_layers)]
        ck_w, ck_b = [], []
        for p in self.layers:
            for a, tag in (("attention", "sa."), ("crossattention", "ca.")):
                s = p + a + ".self."
                wo, bo = fold_output(f32(p + a + ".output.dense.weight"), f32(p + a + ".output.dense.bias"), f32(s + "value.bias"))
                w[p + tag + "v.w"] = half(f32(s + "value.weight"), device)
                w[p + tag + "o.w"], w[p + tag + "o.b"] = half(wo, device), full(bo, device)
                w[p + tag + "ln.w"] = full(f32(p + a + ".output.LayerNorm.weight"), device)
                w[p + tag + "ln.b"] = full(f32(p + a + ".output.LayerNorm.bias"), device)
            s = p + "attention.self."
            w[p + "sa.qk.w"] = half(torch.cat([f32(s + "query.weight"), f32(s + "key.weight")]), device)
            w[p + "sa.qk.b"] = full(torch.cat([f32(s + "query.bias"), f32(s + "key.bias")]), device)
            s = p + "crossattention.self."
            w[p + "ca.q.w"], w[p + "ca.q.b"] = half(f32(s + "query.weight"), device), full(f32(s + "query.bias"), device)
            ck_w.append(f32(s + "key.weight")); ck_b.append(f32(s + "key.bias"))
            w[p + "fc1.w"], w[p + "fc1.b"] = half(f32(p + "intermediate.dense.weight"), device), full(f32(p + "intermediate.dense.bias"), device)
            w[p + "fc2.w"], w[p + "fc2.b"] = half(f32(p + "output.dense.weight"), device), full(f32(p + "output.dense.bias"), device)
            w[p + "ln.w"], w[p + "ln.b"] = full(f32(p + "output.LayerNorm.weight"), device), full(f32(p + "output.LayerNorm.bias"), device)
        w["ca.k.w"], w["ca.k.b"] = half(torch.cat(ck_w), device), full(torch.cat(ck_b), device)     # every layer's cross keys: one GEMM
        self.w = w

    def eval(self):
        return self

    def to(self, *args, **kw):
        return self

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask, encoder_hidden_states, output_hidden_states=False):
        """input_ids, attention_mask [B, T] (right-padded), encoder_hidden_states fp16 [B, Nk, encoder_hidden_size] on the device ->
        last_hidden_state fp16 [B, T, C] and its fp32 copy `last_hidden_state_f32` (every row, padded ones included, as the oracle
        computes them)."""
        cfg, w = self.cfg, self.w
        ids = torch.as_tensor(input_ids)
        if ids.dim() != 2 or ids.shape[1] > cfg.max_position_embeddings:
            raise ValueError(f"BlipTextModel: input_ids must be [B, T <= {cfg.max_position_embeddings}] (the position table), got {tuple(ids.shape)}")
        if ids.shape[1] > 128:
            raise ValueError(f"BlipTextModel: at most 128 tokens (icd_attention_masked), got {ids.shape[1]}")
        B, T = ids.shape
        counts = key_counts_of(attention_mask)
        if tuple(torch.as_tensor(attention_mask).shape) != (B, T):
            raise ValueError(f"BlipTextModel: attention_mask must be [{B}, {T}] like input_ids")
        ids = ids.to(self.device, torch.int64)
        if int(ids.min()) < 0 or int(ids.max()) >= cfg.vocab_size:
            raise IndexError("BlipTextModel: token id out of range")
        enc = encoder_hidden_states
        C, E, H = cfg.hidden_size, cfg.encoder_hidden_size, cfg.num_attention_heads
        if not (isinstance(enc, torch.Tensor) and enc.is_cuda and enc.dtype == torch.float16 and enc.dim() == 3 and enc.shape[0] == B
                and enc.shape[2] == E):
            raise ValueError(f"BlipTextModel: encoder_hidden_states must be a cuda fp16 [{B}, Nk, {E}] tensor")
        Nk = enc.shape[1]
        enc = enc.contiguous().reshape(B * Nk, E)
        d, scale, eps = C // H, (C // H) ** -0.5, cfg.layer_norm_eps
        ld, ldc = (T + 7) // 8 * 8, (Nk + 7) // 8 * 8
        kc = counts.to(torch.int32).to(self.device)
        # the embeddings: a gather and an add in fp32 (exact on the fp16 tables), then embeddings.LayerNorm from fp32
        e32 = (w["tok"][ids].float() + w["pos"][:T].float()[None]).reshape(B * T, C).contiguous()
        x, x32 = ops.layernorm_f32(e32, w["ln_e.w"], w["ln_e.b"], eps)
        hs = [x]

        def add_norm(f, wk, ln, x32):
            s32 = torch.empty(x32.shape, device=x32.device, dtype=torch.float32)
            ops.gemm(f, w[wk + ".w"], w[wk + ".b"], resid=x32, out32=s32)            # s32 = x32 + dense(f) before any fp16 rounding
            return ops.layernorm_f32(s32, w[ln + ".w"], w[ln + ".b"], eps)
        ck = ops.gemm(enc, w["ca.k.w"], w["ca.k.b"])                                 # [B * Nk, L * C]
        for i, p in enumerate(self.layers):
            qk = ops.gemm(x, w[p + "sa.qk.w"], w[p + "sa.qk.b"])
            vt = ops.project_vt(x, w[p + "sa.v.w"], B, T, ld)
            o = ops.attention_masked(qk[:, :C], qk[:, C:], vt, kc, B, H, T, T, d, scale)
            x, x32 = add_norm(o, p + "sa.o", p + "sa.ln", x32)
            q = ops.gemm(x, w[p + "ca.q.w"], w[p + "ca.q.b"])
            vt = ops.project_vt(enc, w[p + "ca.v.w"], B, Nk, ldc)
            o = ops.attention_fused(q, ck[:, i * C:(i + 1) * C], vt, B, H, T, Nk, d, scale)
            x, x32 = add_norm(o, p + "ca.o", p + "ca.ln", x32)
            f = ops.activation(ops.gemm(x, w[p + "fc1.w"], w[p + "fc1.b"]), ops.ACT_GELU)
            x, x32 = add_norm(f, p + "fc2", p + "ln", x32)
            hs.append(x)
        last, last32 = x.reshape(B, T, C), x32.reshape(B, T, C)
        hidden = tuple(h.reshape(B, T, C) for h in hs) if output_hidden_states else None
        return ModelOutput(last, last_hidden_state=last, last_hidden_state_f32=last32, hidden_states=hidden)


# ------------------------------------------------------------------------------------------------------------ the head
def head_shapes(hidden=768):
    dims = (hidden, 1024, 128, 64, 16, 1)
    out = {}
    for n, i in enumerate(HEAD_LAYERS):
        out[f"mlp.layers.{i}.weight"] = (dims[n + 1], dims[n]); out[f"mlp.layers.{i}.bias"] = (dims[n + 1],)
    return out


def fold_head(sd, mean=REWARD_MEAN, std=REWARD_STD):
    """The five Linears mlp.layers.{0,2,4,6,7} (nothing but dropout between them) and (r - mean) / std as one float64 vector w and one
    float64 scalar c:  (mlp(x) - mean) / std = w . x + c."""
    W, b = None, None
    for i in HEAD_LAYERS:
        Wi, bi = sd[f"mlp.layers.{i}.weight"].detach().cpu().double(), sd[f"mlp.layers.{i}.bias"].detach().cpu().double()
        W, b = (Wi, bi) if W is None else (Wi @ W, Wi @ b + bi)
    if tuple(W.shape[:1]) != (1,):
        raise ValueError(f"fold_head: the last Linear must have one output, got {W.shape[0]}")
    return W[0] / std, float((b[0] - mean) / std)


# ------------------------------------------------------------------------------------------------------------ key names
_VISION_BLOCK = {"norm1": "layer_norm1", "norm2": "layer_norm2", "attn.qkv": "self_attn.qkv", "attn.proj": "self_attn.projection",
                 "mlp.fc1": "mlp.fc1", "mlp.fc2": "mlp.fc2"}
_VISION_TOP = {"cls_token": "embeddings.class_embedding", "pos_embed": "embeddings.position_embedding",
               "patch_embed.proj.weight": "embeddings.patch_embedding.weight", "patch_embed.proj.bias": "embeddings.patch_embedding.bias",
               "norm.weight": "post_layernorm.weight", "norm.bias": "post_layernorm.bias"}


def translate_package_keys(sd):
    """A state dict under the ImageReward package's names -> this module's (the oracle's) names: `blip.visual_encoder.*` (timm style)
    -> `vision_model.*` (transformers.BlipVisionModel), `blip.text_encoder.*` (BERT style, the names BlipTextModel kept) ->
    `text_encoder.*`, `mlp.layers.*` as it is.  Keys of neither family (the text decoder's, position_ids buffers) are dropped.  A dict
    without a `blip.` key is returned unchanged.  UNVERIFIED against the real checkpoint (see the module docstring)."""
    if not any(k.startswith("blip.") for k in sd):
        return sd
    out = {}
    for k, v in sd.items():
        if k.startswith("mlp.layers."):
            out[k] = v
        elif k.startswith("blip.text_encoder."):
            if not k.endswith("position_ids"):
                out["text_encoder." + k[len("blip.text_encoder."):]] = v
        elif k.startswith("blip.visual_encoder."):
            r = k[len("blip.visual_encoder."):]
            if r in _VISION_TOP:
                out["vision_model." + _VISION_TOP[r]] = v
            elif r.startswith("blocks."):
                _, n, rest = r.split(".", 2)
                mod, kind = rest.rsplit(".", 1)
                if mod in _VISION_BLOCK:
                    out[f"vision_model.encoder.layers.{n}.{_VISION_BLOCK[mod]}.{kind}"] = v
    return out


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


# ------------------------------------------------------------------------------------------------------------ the model
class ImageReward:
    """Both towers and the folded head.  state_dict: `vision_model.*`, `text_encoder.*`, `mlp.layers.{0,2,4,6,7}.*` (or the package's
    names, which translate_package_keys maps onto these)."""

    def __init__(self, vision_cfg: BlipVisionConfig = IMAGEREWARD_VISION, text_cfg: BlipTextConfig = IMAGEREWARD_TEXT, state_dict=None,
                 device="cuda", dtype=torch.float16):
        if state_dict is None:
            raise ValueError("ImageReward: pass state_dict= (nothing is downloaded here)")
        if text_cfg.encoder_hidden_size != vision_cfg.hidden_size:
            raise ValueError("ImageReward: the text tower's encoder_hidden_size must be the image tower's hidden size")
        sd = translate_package_keys(state_dict)
        check_state_dict(sd, head_shapes(text_cfg.hidden_size), "ImageReward head")
        self.device, self.dtype = torch.device(device), dtype
        self.vision_model = BlipVisionModel(vision_cfg, _sub(sd, "vision_model."), device, dtype)
        self.text_encoder = BlipTextModel(text_cfg, _sub(sd, "text_encoder."), device, dtype)
        self.head_w64, self.head_c64 = fold_head(sd)
        self.head_w = self.head_w64.to(torch.float32).to(device).contiguous()
        self.head_c = float(self.head_c64)

    def eval(self):
        return self

    def to(self, *args, **kw):
        return self

    @torch.no_grad()
    def features(self, prompt_ids, attention_mask, images):
        """the fp32 class-token row of the text tower per (prompt, image) pair, [B, hidden] on the device"""
        enc = self.vision_model.forward_patches(self.vision_model.preprocess(images))
        out = self.text_encoder(prompt_ids, attention_mask, enc)
        return out.last_hidden_state_f32[:, 0].contiguous()

    @torch.no_grad()
    def score(self, prompt_ids, attention_mask, images):
        """(mlp(cls) - mean) / std per pair -> fp32 [B] on the device.  images: PIL images, uint8 HWC arrays (a list may mix sizes) or a
        uint8 NHWC device tensor."""
        import numpy as np
        ids, mask = torch.as_tensor(prompt_ids), torch.as_tensor(attention_mask)
        if isinstance(images, np.ndarray):
            images = image_batch_to_device(images, self.device)
        n = images.shape[0] if isinstance(images, torch.Tensor) else len(images)
        if ids.dim() != 2 or ids.shape[0] != n or tuple(mask.shape) != tuple(ids.shape):
            raise ValueError(f"ImageReward.score: {n} images need input_ids and attention_mask [{n}, T], got {tuple(ids.shape)}, {tuple(mask.shape)}")
        run = lambda idx_ids, idx_mask, imgs: self.features(idx_ids, idx_mask, imgs) @ self.head_w + self.head_c
        if not mixed_sizes(images):
            return run(ids, mask, images)
        return run_by_size(n, lambda i: image_size(images[i]), lambda idx: run(ids[idx], mask[idx], [images[i] for i in idx]))
