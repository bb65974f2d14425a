"""Host side of the DINOv2 encoder (dinov2.py, metrics.calc_dinov2_images_images, synthetic weights): no GPU, no library.

The oracle is `transformers.Dinov2Model` itself: its state-dict layout, and its own `interpolate_pos_encoding` for the folded token
table.  The table is produced by the same interpolate call on the same values, so the tolerance is exact equality; the LayerScale fold
is checked in float64, where 1e-12 is several orders above the rounding of a length-512 dot product of O(1) terms (512 * 2^-53 ~ 6e-14)."""
import dataclasses

import numpy as np
import pytest
import torch

REDUCED = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2)


def _upstream_config(cfg):
    import transformers
    d = cfg.to_dict()
    d.pop("crop_size"); d.pop("resize_shortest_edge")                        # the image processor's, not the model's
    return transformers.Dinov2Config(**d)


def test_state_dict_layout_is_transformers():
    import transformers
    from invertible_cd_amd import dinov2
    for cfg in (dinov2.Dinov2Config(**REDUCED), dinov2.DINOV2_BASE):
        with torch.device("meta"):
            m = transformers.Dinov2Model(_upstream_config(cfg))
        ref = {k: tuple(v.shape) for k, v in m.state_dict().items() if k != "embeddings.mask_token"}
        assert "embeddings.mask_token" in m.state_dict()
        assert cfg.state_dict_shapes() == ref
    assert dinov2.DINOV2_BASE.num_positions == 37 * 37 + 1 and dinov2.DINOV2_BASE.num_tokens == 257
    assert dinov2.DINOV2_BASE.to_dict()["layer_norm_eps"] == 1e-6


def _upstream(cfg, sd):
    import transformers
    m = transformers.Dinov2Model(_upstream_config(cfg)).eval().float()
    own = m.state_dict()
    assert all(k in sd or k == "embeddings.mask_token" for k in own)
    m.load_state_dict({k: sd.get(k, v) for k, v in own.items()}, strict=True)
    return m


def test_token_table_is_upstreams_interpolated_position_table_bit_for_bit():
    """tok[0] = cls_token + pos[0]; tok[1 + p] = interpolate_pos_encoding(...)[1 + p] + patch bias.  `(a + b) - b == a` does not hold in
    floating point, so "minus the patch bias" is checked in its two exact forms: with the bias set to zero the rows ARE upstream's, and
    with the seeded (nonzero) bias they are upstream's rows plus it, the one fp32 add the fold makes."""
    from invertible_cd_amd import dinov2, synthetic
    cfg = dinov2.Dinov2Config(**REDUCED)                                      # image_size 518: a 37 x 37 table resized to 16 x 16
    sd = synthetic.synthetic_dinov2_state_dict(cfg, seed=1)
    sd["embeddings.mask_token"] = torch.zeros(1, cfg.hidden_size)            # accepted and ignored
    bias = sd["embeddings.patch_embeddings.projection.bias"]
    assert float(bias.abs().min()) > 0
    up = _upstream(cfg, sd)
    with torch.no_grad():
        ref = up.embeddings.interpolate_pos_encoding(torch.zeros(1, 257, cfg.hidden_size), 224, 224)[0]
        cls = up.embeddings.cls_token[0, 0] + up.embeddings.position_embeddings[0, 0]
    assert tuple(ref.shape) == (257, cfg.hidden_size)
    tok = dinov2.Dinov2Model(cfg, sd, device="cpu").w["tok"]
    assert tok.dtype == torch.float32 and tuple(tok.shape) == (257, cfg.hidden_size)
    assert torch.equal(tok[0], cls)
    assert torch.equal(tok[1:], ref[1:] + bias)
    zero = dict(sd)
    zero["embeddings.patch_embeddings.projection.bias"] = torch.zeros_like(bias)
    tok0 = dinov2.Dinov2Model(cfg, zero, device="cpu").w["tok"]
    assert torch.equal(tok0[1:], ref[1:]) and torch.equal(tok0[0], cls)
    assert not torch.equal(tok0[1:], tok[1:])
    # grids agree (image_size 224): nothing is interpolated, the stored table is the table
    same = dataclasses.replace(cfg, image_size=224)
    sd2 = synthetic.synthetic_dinov2_state_dict(same, seed=2)
    pos = sd2["embeddings.position_embeddings"][0]
    t2 = dinov2.Dinov2Model(same, sd2, device="cpu").w["tok"]
    assert torch.equal(t2[1:], pos[1:] + sd2["embeddings.patch_embeddings.projection.bias"])
    assert torch.equal(t2[0], sd2["embeddings.cls_token"][0, 0] + pos[0])
    with torch.no_grad():
        assert torch.equal(_upstream(same, sd2).embeddings.interpolate_pos_encoding(torch.zeros(1, 257, 128), 224, 224)[0], pos)


def test_layer_scale_fold_in_float64():
    from invertible_cd_amd import dinov2, synthetic
    cfg = dinov2.Dinov2Config(**REDUCED)
    sd = synthetic.synthetic_dinov2_state_dict(cfg, seed=3)
    p = "encoder.layer.1."
    lam1, lam2 = sd[p + "layer_scale1.lambda1"], sd[p + "layer_scale2.lambda1"]
    for lam in (lam1, lam2):
        assert float(lam.min()) >= 0.25 and float(lam.max()) <= 1.0 and float((lam - 1).abs().min()) > 0
    g = torch.Generator().manual_seed(0)
    # attention output: o = P (V x + b_v) = P V x + b_v (softmax rows sum to one), then lambda1 * (W o + b)
    W, b, bv = sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"], sd[p + "attention.attention.value.bias"]
    o = torch.randn(7, cfg.hidden_size, generator=g, dtype=torch.float64)
    Wf, bf = dinov2.fold_layer_scale(W, b, lam1, bv)
    assert Wf.dtype == bf.dtype == torch.float64
    want = lam1.double() * ((o + bv.double()) @ W.double().T + b.double())
    assert float((o @ Wf.T + bf - want).abs().max()) < 1e-12
    W, b = sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"]
    h = torch.randn(7, cfg.intermediate_size, generator=g, dtype=torch.float64)
    Wf, bf = dinov2.fold_layer_scale(W, b, lam2)
    want = lam2.double() * (h @ W.double().T + b.double())
    assert float((h @ Wf.T + bf - want).abs().max()) < 1e-12
    # ... and the prepared weights are those products, rounded to the storage types
    m = dinov2.Dinov2Model(cfg, sd, device="cpu")
    assert torch.equal(m.w[p + "fc2.w"], Wf.to(torch.float16)) and torch.equal(m.w[p + "fc2.b"], bf.float())
    assert not torch.equal(m.w[p + "fc2.w"], W.to(torch.float16))


def test_refusals():
    from invertible_cd_amd import dinov2, metrics, synthetic
    imgs = np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="model="):
        metrics.calc_dinov2_images_images(imgs, imgs, "cuda")
    with pytest.raises(ValueError, match="model="):
        metrics.calc_dinov2_images_images(imgs, imgs, "cuda", model=None)
    cfg = dinov2.Dinov2Config(**REDUCED)
    sd = synthetic.synthetic_dinov2_state_dict(cfg, seed=1)
    dinov2.Dinov2Model(cfg, sd, device="cpu")
    with pytest.raises(ValueError, match="swiglu"):
        dinov2.Dinov2Model(dataclasses.replace(cfg, use_swiglu_ffn=True), sd, device="cpu")
    with pytest.raises(KeyError, match="layer_scale2"):
        dinov2.Dinov2Model(cfg, {k: v for k, v in sd.items() if not k.endswith("1.layer_scale2.lambda1")}, device="cpu")
    bad = dict(sd)
    bad["layernorm.weight"] = torch.zeros(127)
    with pytest.raises(ValueError, match="layernorm.weight"):
        dinov2.Dinov2Model(cfg, bad, device="cpu")
    odd = dataclasses.replace(cfg, hidden_size=120)                          # head dim 60: not a multiple of 8
    with pytest.raises(ValueError, match="multiple of 8"):
        dinov2.Dinov2Model(odd, synthetic.synthetic_dinov2_state_dict(odd, seed=1), device="cpu")
    wide = dataclasses.replace(cfg, hidden_size=336)                         # head dim 168 > 160
    with pytest.raises(ValueError, match="<= 160"):
        dinov2.Dinov2Model(wide, synthetic.synthetic_dinov2_state_dict(wide, seed=1), device="cpu")
    with pytest.raises(ValueError, match="hidden_act"):
        dinov2.Dinov2Model(dataclasses.replace(cfg, hidden_act="relu"), sd, device="cpu")


def test_load_dinov2_reads_a_transformers_layout_directory(tmp_path):
    import json
    from safetensors.torch import save_file
    from invertible_cd_amd import dinov2, loading
    from invertible_cd_amd import synthetic
    cfg = dinov2.Dinov2Config(**REDUCED)
    sd = synthetic.synthetic_dinov2_state_dict(cfg, seed=4)
    d = cfg.to_dict()
    d.pop("crop_size"); d.pop("resize_shortest_edge")
    d["model_type"] = "dinov2"                                               # fields this package does not know are ignored
    (tmp_path / "config.json").write_text(json.dumps(d))
    (tmp_path / "preprocessor_config.json").write_text(json.dumps({"crop_size": {"height": 224, "width": 224}, "size": {"shortest_edge": 256},
                                                                   "image_mean": [0.485, 0.456, 0.406]}))
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        loading.load_dinov2(str(tmp_path), device="cpu")
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    m, direct = loading.load_dinov2(str(tmp_path), device="cpu"), dinov2.Dinov2Model(cfg, sd, device="cpu")
    assert m.cfg == cfg and m.w.keys() == direct.w.keys() and all(torch.equal(m.w[k], direct.w[k]) for k in m.w)
    m2 = loading.load_dinov2(sd, device="cpu", config=cfg)
    assert all(torch.equal(m2.w[k], direct.w[k]) for k in direct.w)
    with pytest.raises(KeyError, match="lacks"):                             # without a config the dinov2-base defaults do not fit these weights
        loading.load_dinov2(sd, device="cpu")
