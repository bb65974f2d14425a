"""The oracle of the ImageReward tests: transformers' BlipVisionModel and BlipTextModel in fp32 on seeded weights, the unfolded
five-Linear reward head in float64, and the seeded state-dict maker (test infrastructure, like lpips_ref.py and inception_ref.py).

The state dict is under the names of invertible_cd_amd.blip: `vision_model.*` (BlipVisionModel's own), `text_encoder.*` (BlipTextModel's
own, config is_decoder=True so that the crossattention modules exist, add_pooling_layer=False), `mlp.layers.{0,2,4,6,7}.*`.  Every value
is rounded to fp16 first, so the oracle and the device read the same weights.  Default initialisation (std 0.02) leaves the softmaxes
nearly flat; the query and key weights are drawn with variance QK_GAIN / fan_in instead, which gives scores a deviation of about QK_GAIN
and peaked attention rows (`first_layer_probs` shows them; the tests assert the share of peaked rows on it)."""
import torch

QK_GAIN = 3.0
HEAD_LAYERS = (0, 2, 4, 6, 7)
HEAD_DIMS = (1024, 128, 64, 16, 1)


def make_state_dict(vcfg, tcfg, seed=0, qk_gain=QK_GAIN):
    from invertible_cd_amd import blip
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def fill(prefix, shapes):
        for k, shp in shapes.items():
            if k.endswith("LayerNorm.weight") or (k.endswith(".weight") and ("layer_norm" in k or "layernorm" in k)):
                t = 1.0 + 0.1 * torch.randn(shp, generator=g)
            elif k.endswith(".bias"):
                t = 0.05 * torch.randn(shp, generator=g)
            elif ".query.weight" in k or ".key.weight" in k:
                t = torch.randn(shp, generator=g) * (qk_gain / shp[1]) ** 0.5
            elif k.endswith("qkv.weight"):
                t = torch.randn(shp, generator=g) * 0.04
                C = shp[1]
                t[:2 * C] = torch.randn((2 * C, C), generator=g) * (qk_gain / C) ** 0.5
            elif "embedding" in k and not k.endswith("patch_embedding.weight"):
                t = 0.5 * torch.randn(shp, generator=g)
            else:
                t = torch.randn(shp, generator=g) * 0.04
            sd[prefix + k] = t.half().float()
    fill("vision_model.", vcfg.state_dict_shapes())
    fill("text_encoder.", tcfg.state_dict_shapes())
    for k, shp in blip.head_shapes(tcfg.hidden_size).items():
        sd[k] = (torch.randn(shp, generator=g) * (shp[-1] ** -0.5 if k.endswith("weight") else 0.1)).half().float()
    return sd


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def vision_oracle(vcfg, sd):
    import transformers
    from transformers.models.blip.modeling_blip import BlipVisionModel
    tc = transformers.BlipVisionConfig(**vcfg.to_dict())
    tc._attn_implementation = "eager"
    m = BlipVisionModel(tc).eval().float()
    m.load_state_dict(_sub(sd, "vision_model."), strict=True)
    return m


def text_oracle(tcfg, sd):
    import transformers
    from transformers.models.blip.modeling_blip_text import BlipTextModel
    tc = transformers.BlipTextConfig(**tcfg.to_dict(), is_decoder=True, pad_token_id=0, bos_token_id=1, sep_token_id=2, eos_token_id=2)
    tc._attn_implementation = "eager"
    m = BlipTextModel(tc, add_pooling_layer=False).eval().float()
    m.load_state_dict(_sub(sd, "text_encoder."), strict=True)
    return m


@torch.no_grad()
def text_forward(oracle, ids, mask, image_tokens):
    """last_hidden_state fp32 [B, T, C]: bidirectional self-attention under the padding mask (is_decoder=False, the default of
    forward), cross-attention to all image tokens (the reference passes a mask of ones)."""
    ones = torch.ones(image_tokens.shape[:2], dtype=torch.long)
    return oracle(input_ids=ids, attention_mask=mask, encoder_hidden_states=image_tokens, encoder_attention_mask=ones).last_hidden_state


def head_ref(sd, x, mean, std):
    """the five Linears applied one after the other in float64, then (r - mean) / std -> float64 [B]"""
    x = x.double()
    for i in HEAD_LAYERS:
        x = x @ sd[f"mlp.layers.{i}.weight"].double().T + sd[f"mlp.layers.{i}.bias"].double()
    return (x[:, 0] - mean) / std


@torch.no_grad()
def first_layer_probs(oracle, ids, mask):
    """the self-attention probabilities of the text tower's first layer, fp32 [B, H, T, T], from the oracle's own modules"""
    x = oracle.embeddings(input_ids=ids)
    a = oracle.encoder.layer[0].attention.self
    B, T, C = x.shape
    H = a.num_attention_heads
    split = lambda t: t.reshape(B, T, H, C // H).permute(0, 2, 1, 3)
    s = split(a.query(x)) @ split(a.key(x)).transpose(-1, -2) / (C // H) ** 0.5
    s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    return s.softmax(-1)


def to_package_names(sd):
    """the same weights under the ImageReward package's names (timm-style `blip.visual_encoder.*`, BERT-style `blip.text_encoder.*`)"""
    block = {"layer_norm1": "norm1", "layer_norm2": "norm2", "self_attn.qkv": "attn.qkv", "self_attn.projection": "attn.proj",
             "mlp.fc1": "mlp.fc1", "mlp.fc2": "mlp.fc2"}
    top = {"embeddings.class_embedding": "cls_token", "embeddings.position_embedding": "pos_embed",
           "embeddings.patch_embedding.weight": "patch_embed.proj.weight", "embeddings.patch_embedding.bias": "patch_embed.proj.bias",
           "post_layernorm.weight": "norm.weight", "post_layernorm.bias": "norm.bias"}
    out = {}
    for k, v in sd.items():
        if k.startswith("text_encoder."):
            out["blip." + k] = v
        elif k.startswith("vision_model."):
            r = k[len("vision_model."):]
            if r in top:
                out["blip.visual_encoder." + top[r]] = v
            else:
                _, _, n, rest = r.split(".", 3)
                mod, kind = rest.rsplit(".", 1)
                out[f"blip.visual_encoder.blocks.{n}.{block[mod]}.{kind}"] = v
        else:
            out[k] = v
    out["blip.text_encoder.embeddings.position_ids"] = torch.arange(8)[None]       # a buffer the package's checkpoint carries
    return out
