"""CLIP text encoders (the step in front of the iCD path) on the HIP kernels of this package - SURVEY.md section 8f rank 3.

Drop-in for what the reference calls on `model.text_encoder` / `pipe.text_encoder(_2)` (transformers classes there):
    text_encoder(input_ids)[0]                                   utils/generation.py:293,301      -> [B, 77, 768]
    out = text_encoder(input_ids, output_hidden_states=True)     utils/generation_sdxl.py:31-44
    out[0] (pooled text_embeds of the projection model), out.hidden_states[-2]
    .device, .dtype, .config

Architecture (transformers CLIPTextModel / CLIPTextModelWithProjection; oracle/clip_ref.py runs the real classes):
token + position embeddings (`icd_embed_tokens`), N pre-LayerNorm blocks of causal multi-head self-attention (head dim 64;
`icd_attention_fused_ex` with ICD_ATTN_CAUSAL, q/k from one fused biased GEMM, V^T from the transposing GEMM epilogue) and a
biased MLP (`icd_gemm` -> `icd_activation` quick_gelu | gelu -> `icd_gemm` + residual), final LayerNorm, EOS pooling, optional
bias-free projection.  The blocks, their weight preparation and the fp32 twin of the residual stream are encoder.py's, shared with the
image tower below and with dinov2.py.  Tokenizers need a vocabulary that is not available offline: callers pass
token ids (synthetic.SyntheticTokenizer produces ids of the right shape).

The image tower (`CLIPVisionModelWithProjection`) and the joint `CLIPModel` serve the edit-quality metrics (metrics.py): what the
reference gets from `AutoModel.from_pretrained('openai/clip-vit-large-patch14')` as `get_image_features` / `get_text_features`
(utils/metrics.py).  Same transformer on the same operators; it starts from the patch matrix of `icd_clip_preprocess`, attends without
a mask over 257 tokens and pools token 0.
"""
from dataclasses import dataclass, asdict
from types import SimpleNamespace

import torch

from . import ops
from .encoder import ModelOutput, check_state_dict, check_widths, full, half, prepare_block, run_blocks
from .encoder import images_to_device   # noqa: F401  (its first home: still importable from here)

TextEncoderOutput = ModelOutput           # likewise


def _block_shapes(C, I, layers):
    """keys -> shapes of the encoder layers, which the two towers name alike"""
    out = {}
    for i in range(layers):
        p = f"encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            out[p + f"self_attn.{n}.weight"] = (C, C); out[p + f"self_attn.{n}.bias"] = (C,)
        for n in ("layer_norm1", "layer_norm2"):
            out[p + n + ".weight"] = (C,); out[p + n + ".bias"] = (C,)
        out[p + "mlp.fc1.weight"] = (I, C); out[p + "mlp.fc1.bias"] = (I,)
        out[p + "mlp.fc2.weight"] = (C, I); out[p + "mlp.fc2.bias"] = (C,)
    return out


def _block_names(p):
    a = p + "self_attn."
    return {"q": a + "q_proj", "k": a + "k_proj", "v": a + "v_proj", "out": a + "out_proj", "norm1": p + "layer_norm1",
            "norm2": p + "layer_norm2", "fc1": p + "mlp.fc1", "fc2": p + "mlp.fc2"}


def _strip(sd, prefix):
    return {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in sd.items()}


@dataclass(frozen=True)
class CLIPTextConfig:
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 77
    hidden_act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5
    projection_dim: int = 768
    eos_token_id: int = 2            # legacy value of the released checkpoints: pooling takes argmax(input_ids)
    bos_token_id: int = 0
    pad_token_id: int = 1

    def to_dict(self):
        return asdict(self)

    def state_dict_shapes(self, with_projection=False):
        C, I, V, T = self.hidden_size, self.intermediate_size, self.vocab_size, self.max_position_embeddings
        out = {"embeddings.token_embedding.weight": (V, C), "embeddings.position_embedding.weight": (T, C)}
        out.update(_block_shapes(C, I, self.num_hidden_layers))
        out["final_layer_norm.weight"] = (C,); out["final_layer_norm.bias"] = (C,)
        if with_projection:
            out["text_projection.weight"] = (self.projection_dim, C)
        return out


CLIP_VIT_L = CLIPTextConfig()                                                        # SD1.5 / SDXL text_encoder
OPENCLIP_BIGG = CLIPTextConfig(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                               hidden_act="gelu", projection_dim=1280)               # SDXL text_encoder_2 (with projection)


class CLIPTextModel:
    def __init__(self, cfg: CLIPTextConfig, state_dict, with_projection=False, device="cuda", dtype=torch.float16):
        check_widths("CLIPTextModel", cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.hidden_act)
        self.cfg, self.with_projection = cfg, with_projection
        self.device, self.dtype = torch.device(device), dtype
        self.config = SimpleNamespace(**cfg.to_dict())
        sd = _strip(state_dict, "text_model.")
        check_state_dict(sd, cfg.state_dict_shapes(with_projection), "CLIP text")
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
        w = {"tok": half(f32("embeddings.token_embedding.weight"), device), "pos": half(f32("embeddings.position_embedding.weight"), device)}
        self.blocks = [f"encoder.layers.{i}." for i in range(cfg.num_hidden_layers)]
        for p in self.blocks:
            # the V bias is folded in fp32 here; float64 (as in the image tower) is sounder, but moves the text embeddings in the last bit
            w.update((p + k, t) for k, t in prepare_block(f32, _block_names(p), device, fold_dtype=torch.float32).items())
        w["ln_f.w"], w["ln_f.b"] = full(f32("final_layer_norm.weight"), device), full(f32("final_layer_norm.bias"), device)
        if with_projection:
            w["proj.w"] = half(f32("text_projection.weight"), device)
        self.w = w

    def to(self, *args, **kw):
        for a in list(args) + [kw.get("dtype")]:
            if isinstance(a, torch.dtype):
                self.dtype = a
        return self

    def eval(self):
        return self

    @torch.no_grad()
    def __call__(self, input_ids, output_hidden_states=False, **unused):
        cfg, w = self.cfg, self.w
        if input_ids.dim() != 2 or input_ids.shape[1] > cfg.max_position_embeddings:
            raise ValueError(f"CLIPTextModel: input_ids must be [B, T <= {cfg.max_position_embeddings}], got {tuple(input_ids.shape)}")
        ids = input_ids.to(self.device, torch.int64).contiguous()
        if int(ids.min()) < 0 or int(ids.max()) >= cfg.vocab_size:
            raise IndexError("CLIPTextModel: token id out of range")
        B, T = ids.shape
        C = cfg.hidden_size
        x = ops.embed_tokens(ids, w["tok"], w["pos"])
        hs = [x]
        # the text encoders run once per prompt, outside every timed loop: the fp32 twin of the residual stream costs nothing that is measured
        x, _ = run_blocks(w, self.blocks, x, None, B, T, cfg.num_attention_heads, cfg.layer_norm_eps, cfg.hidden_act, True, hs)
        last = ops.layernorm(x, w["ln_f.w"], w["ln_f.b"], cfg.layer_norm_eps).reshape(B, T, C)
        if cfg.eos_token_id == 2:                               # transformers: legacy configs pool at argmax(input_ids)
            eos = ids.argmax(dim=-1)
        else:
            eos = (ids == cfg.eos_token_id).int().argmax(dim=-1)
        pooled = last[torch.arange(B, device=self.device), eos].contiguous()
        cast = lambda t: t.to(self.dtype)
        hidden = tuple(cast(h.reshape(B, T, C)) for h in hs) if output_hidden_states else None
        if self.with_projection:
            embeds = ops.gemm(pooled, w["proj.w"])
            return ModelOutput(cast(embeds), text_embeds=cast(embeds), last_hidden_state=cast(last), hidden_states=hidden)
        return ModelOutput(cast(last), last_hidden_state=cast(last), pooler_output=cast(pooled), hidden_states=hidden)


# ------------------------------------------------------------------------------------------------------------ image tower
@dataclass(frozen=True)
class CLIPVisionConfig:
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    num_channels: int = 3
    image_size: int = 224
    patch_size: int = 14
    hidden_act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5
    projection_dim: int = 768

    def to_dict(self):
        return asdict(self)

    @property
    def num_positions(self):
        return (self.image_size // self.patch_size) ** 2 + 1

    def state_dict_shapes(self):
        """canonical ('vision_model.' prefix stripped) keys -> shapes of transformers.CLIPVisionModelWithProjection ('pre_layrnorm' sic)."""
        C, I, P = self.hidden_size, self.intermediate_size, self.patch_size
        out = {"embeddings.class_embedding": (C,), "embeddings.patch_embedding.weight": (C, self.num_channels, P, P),
               "embeddings.position_embedding.weight": (self.num_positions, C),
               "pre_layrnorm.weight": (C,), "pre_layrnorm.bias": (C,)}
        out.update(_block_shapes(C, I, self.num_hidden_layers))
        out["post_layernorm.weight"] = (C,); out["post_layernorm.bias"] = (C,)
        out["visual_projection.weight"] = (self.projection_dim, C)
        return out


CLIP_VIT_L_VISION = CLIPVisionConfig()                                               # openai/clip-vit-large-patch14


class CLIPVisionModelWithProjection:
    def __init__(self, cfg: CLIPVisionConfig, state_dict, device="cuda", dtype=torch.float16):
        check_widths("CLIPVisionModel", cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.hidden_act,
                     extra=(cfg.projection_dim,))
        if cfg.num_channels != 3 or cfg.image_size % cfg.patch_size or cfg.image_size % 4:
            raise ValueError("CLIPVisionModel: 3 channels, image size a multiple of the patch size and of 4")
        self.cfg = cfg
        self.device, self.dtype = torch.device(device), dtype
        self.config = SimpleNamespace(**cfg.to_dict())
        sd = _strip(state_dict, "vision_model.")
        check_state_dict(sd, cfg.state_dict_shapes(), "CLIP vision")
        f32 = lambda k: sd[k].detach().to("cpu", torch.float32)
        C = cfg.hidden_size
        kp = 3 * cfg.patch_size ** 2
        wp = torch.zeros((C, (kp + 7) // 8 * 8))                 # icd_gemm needs K % 8 == 0: pad columns are zero here and in the patch matrix
        wp[:, :kp] = f32("embeddings.patch_embedding.weight").reshape(C, kp)
        pos = f32("embeddings.position_embedding.weight")
        w = {"patch.w": half(wp, device), "pos": half(pos[1:], device), "cls": half(f32("embeddings.class_embedding") + pos[0], device)}
        w["ln_pre.w"], w["ln_pre.b"] = full(f32("pre_layrnorm.weight"), device), full(f32("pre_layrnorm.bias"), device)
        self.blocks = [f"encoder.layers.{i}." for i in range(cfg.num_hidden_layers)]
        for p in self.blocks:
            w.update((p + k, t) for k, t in prepare_block(f32, _block_names(p), device).items())
        w["ln_post.w"], w["ln_post.b"] = full(f32("post_layernorm.weight"), device), full(f32("post_layernorm.bias"), device)
        w["proj.w"] = half(f32("visual_projection.weight"), device)
        self.w = w

    def eval(self):
        return self

    def preprocess(self, images):
        """uint8 NHWC images -> the patch matrix [B * n_patches, pad8(3 * patch^2)] (transformers.CLIPImageProcessor on the device)."""
        cfg = self.cfg
        return ops.clip_preprocess(images_to_device(images, self.device), cfg.image_size, cfg.image_size, cfg.patch_size)

    @torch.no_grad()
    def forward_patches(self, patches, output_hidden_states=False):
        """patch matrix of `preprocess` -> image_embeds fp32 [B, projection_dim] (and the L + 1 hidden states when asked)."""
        cfg, w = self.cfg, self.w
        C, H, T = cfg.hidden_size, cfg.num_attention_heads, cfg.num_positions
        n = T - 1
        if patches.dim() != 2 or patches.shape[0] % n or patches.shape[1] != w["patch.w"].shape[1]:
            raise ValueError(f"CLIPVisionModel: patch matrix must be [B * {n}, {w['patch.w'].shape[1]}], got {tuple(patches.shape)}")
        B = patches.shape[0] // n
        # embeddings: patch GEMM (+ position rows as its residual), the class token (+ its position) in front
        pe = ops.gemm(patches, w["patch.w"], resid=w["pos"].repeat(B, 1))
        e = torch.empty((B, T, C), device=self.device, dtype=torch.float16)
        e[:, 0] = w["cls"]
        e[:, 1:] = pe.reshape(B, n, C)
        x = ops.layernorm(e.reshape(B * T, C), w["ln_pre.w"], w["ln_pre.b"], cfg.layer_norm_eps)
        hs = [x]
        x, _ = run_blocks(w, self.blocks, x, None, B, T, H, cfg.layer_norm_eps, cfg.hidden_act, False, hs)
        tok0 = x.reshape(B, T, C)[:, 0].contiguous()           # only the class token is pooled
        pooled = ops.layernorm(tok0, w["ln_post.w"], w["ln_post.b"], cfg.layer_norm_eps)
        embeds = ops.gemm(pooled, w["proj.w"], out_f32=True)
        if output_hidden_states:
            return embeds, tuple(h.reshape(B, T, C) for h in hs)
        return embeds

    def __call__(self, images, output_hidden_states=False):
        out = self.forward_patches(self.preprocess(images), output_hidden_states)
        if output_hidden_states:
            return ModelOutput(out[0], image_embeds=out[0], hidden_states=out[1])
        return ModelOutput(out, image_embeds=out)


class CLIPModel:
    """The two towers behind the CLIP scores: get_image_features(images) and get_text_features(input_ids), fp32 [B, projection_dim]."""

    def __init__(self, text_cfg: CLIPTextConfig, vision_cfg: CLIPVisionConfig, state_dict, device="cuda", dtype=torch.float16):
        if text_cfg.projection_dim != vision_cfg.projection_dim:
            raise ValueError("CLIPModel: the towers project to different widths")
        text_sd = {k: v for k, v in state_dict.items() if k.startswith("text_model.") or k == "text_projection.weight"}
        vis_sd = {k: v for k, v in state_dict.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}
        self.text_model = CLIPTextModel(text_cfg, text_sd, True, device, dtype)
        self.vision_model = CLIPVisionModelWithProjection(vision_cfg, vis_sd, device, dtype)
        self.device, self.dtype = torch.device(device), dtype

    def eval(self):
        return self

    def to(self, *args, **kw):
        return self

    def get_image_features(self, images):
        return self.vision_model.forward_patches(self.vision_model.preprocess(images))

    def get_text_features(self, input_ids):
        return self.text_model(input_ids).text_embeds.float()
