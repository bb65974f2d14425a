"""Host side of the edit-quality metrics (metrics.py, resample.py, clip.CLIPVisionConfig): no GPU.

The resample tables are checked against Pillow itself.  Pillow's BICUBIC resize is integer arithmetic once the coefficient tables
exist, so the tolerance is exact equality: it is derived, not chosen."""
import math

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("h,w", [(512, 512), (1024, 1024), (480, 640), (640, 480), (200, 200)])
def test_resample_tables_reproduce_pillow_bicubic_bit_for_bit(h, w):
    """512 -> 224, 1024 -> 224, 640 x 480 (both orientations) -> shortest edge 224, and the upscale 200 -> 224: the two integer passes
    driven by the host tables equal PIL.Image.resize(..., BICUBIC) exactly."""
    from PIL import Image
    from invertible_cd_amd import metrics
    rng = np.random.default_rng(h * 7 + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rh, rw, top, left = metrics.clip_geometry(h, w)
    assert min(rh, rw) == 224 and 0 <= top <= rh - 224 and 0 <= left <= rw - 224
    got = metrics.resize_emulated(img, rh, rw)
    ref = np.asarray(Image.fromarray(img).resize((rw, rh), Image.BICUBIC))
    assert got.shape == ref.shape and np.array_equal(got, ref)
    first, count, coef = metrics.resample_tables(w, rw)
    assert first.dtype == count.dtype == coef.dtype == np.int32 and coef.shape == (rw, math.ceil(2 * max(w / rw, 1)) * 2 + 1)
    assert (first >= 0).all() and (first + count <= w).all() and (count <= coef.shape[1]).all()
    assert metrics.resample_tables(w, rw)[2] is coef                         # cached per (in_size, out_size)


def test_geometry_and_crop_match_the_transformers_processor():
    """Shortest-edge size and centre crop as transformers' PIL image processor applies them (the GPU test compares the kernel itself)."""
    import transformers
    from PIL import Image
    from invertible_cd_amd import metrics, resample
    proc = transformers.CLIPImageProcessorPil()
    rng = np.random.default_rng(3)
    mean, std = np.array(resample.CLIP_MEAN, np.float32), np.array(resample.CLIP_STD, np.float32)
    for h, w in [(480, 640), (300, 517), (517, 300)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rh, rw, top, left = metrics.clip_geometry(h, w)
        u = metrics.resize_emulated(img, rh, rw)[top:top + 224, left:left + 224]
        pv = proc(images=[Image.fromarray(img)], return_tensors="pt")["pixel_values"][0].numpy().transpose(1, 2, 0)
        rec = np.rint((pv * std + mean) * 255).astype(np.int64)
        assert np.array_equal(rec, u.astype(np.int64)), (h, w)


def test_psnr_on_host_images_is_the_reference_formula_exactly():
    from invertible_cd_amd import metrics
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (3, 64, 48, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (3, 64, 48, 3), dtype=np.uint8)
    b[1] = np.clip(a[1].astype(np.int64) + rng.integers(-2, 3, a[1].shape), 0, 255).astype(np.uint8)
    got = metrics.calculate_psnr(list(a), list(b), "cpu")
    want = []
    for x, y in zip(a, b):
        mse = np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2)
        want.append(20 * math.log10(255.0 / math.sqrt(mse)))
    assert got == want                                                       # float64, exactly
    from PIL import Image
    assert metrics.calculate_psnr([Image.fromarray(x) for x in a], [Image.fromarray(y) for y in b], "cpu") == want
    assert metrics.calculate_psnr(list(a), list(a), "cpu") == float("inf")
    assert metrics.calculate_psnr([a[0], a[1]], [b[0], a[1]], "cpu") == float("inf")     # the reference returns at the first identical pair


def test_vision_state_dict_layout_is_transformers():
    import transformers
    from invertible_cd_amd import clip
    for cfg in (clip.CLIP_VIT_L_VISION, clip.CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=2,
                                                              num_attention_heads=2, projection_dim=64)):
        with torch.device("meta"):
            m = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**cfg.to_dict()))
        canon = lambda k: k[len("vision_model."):] if k.startswith("vision_model.") else k
        ref = {canon(k): tuple(v.shape) for k, v in m.state_dict().items() if not k.endswith("position_ids")}
        assert cfg.state_dict_shapes() == ref


def test_vision_model_refuses_bad_state_dicts_and_widths():
    """Refusals happen before anything touches a device (device='cpu' here: construction only)."""
    from invertible_cd_amd import clip, synthetic
    cfg = clip.CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, projection_dim=64)
    sd = synthetic.synthetic_clip_vision_state_dict(cfg, seed=1)
    clip.CLIPVisionModelWithProjection(cfg, sd, device="cpu")
    missing = {k: v for k, v in sd.items() if not k.endswith("pre_layrnorm.weight")}
    with pytest.raises(KeyError, match="pre_layrnorm"):
        clip.CLIPVisionModelWithProjection(cfg, missing, device="cpu")
    bad = dict(sd)
    bad["visual_projection.weight"] = torch.zeros(64, 127)
    with pytest.raises(ValueError, match="visual_projection.weight"):
        clip.CLIPVisionModelWithProjection(cfg, bad, device="cpu")
    import dataclasses
    odd = dataclasses.replace(cfg, hidden_size=120, num_attention_heads=2)            # head dim 60: not a multiple of 8
    with pytest.raises(ValueError, match="multiple of 8"):
        clip.CLIPVisionModelWithProjection(odd, synthetic.synthetic_clip_vision_state_dict(odd, seed=1), device="cpu")


def test_metrics_refuse_a_missing_model_and_untokenised_prompts():
    from invertible_cd_amd import metrics
    imgs = np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="model="):
        metrics.calc_clip_score_images_images(imgs, imgs, "cuda")
    with pytest.raises(ValueError, match="tokenizer="):
        metrics.calc_clip_score_images_prompts(imgs, ["a cat"], "cuda", model=object())


# ------------------------------------------------------------------------------------------------ loading.load_clip (host side)
def _reduced_clip(seed=4):
    from invertible_cd_amd import clip, synthetic
    tcfg = clip.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2,
                               projection_dim=64, eos_token_id=998)
    vcfg = clip.CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, projection_dim=64)
    sd = synthetic.synthetic_clip_state_dict(tcfg, True, seed=seed)
    sd.update(synthetic.synthetic_clip_vision_state_dict(vcfg, seed=seed))
    return tcfg, vcfg, sd


def _write_clip_dir(root, tcfg, vcfg, sd, weights=True):
    """A transformers-layout directory: config.json with text_config / vision_config sections and a top-level projection_dim."""
    import json
    from safetensors.torch import save_file
    t, v = tcfg.to_dict(), vcfg.to_dict()
    t.pop("projection_dim"); v.pop("projection_dim")                         # the released config.json carries it at the top level
    t["model_type"], v["dropout"] = "clip_text_model", 0.0                   # fields this package does not know are ignored
    with open(root / "config.json", "w") as f:
        json.dump({"model_type": "clip", "projection_dim": tcfg.projection_dim, "logit_scale_init_value": 2.6592,
                   "text_config": t, "vision_config": v}, f)
    if weights:
        save_file({k: x.contiguous() for k, x in sd.items()}, str(root / "model.safetensors"))


def test_load_clip_reads_a_transformers_layout_directory(tmp_path):
    """config.json overrides reach both towers (widths, depth, the text tower's eos_token_id pooling rule, projection_dim from the top
    level); the weights are those of the state dict; a directory without model.safetensors and refused configurations raise."""
    import dataclasses
    from invertible_cd_amd import clip, loading
    tcfg, vcfg, sd = _reduced_clip()
    _write_clip_dir(tmp_path, tcfg, vcfg, sd)
    m = loading.load_clip(str(tmp_path), device="cpu")
    assert isinstance(m, clip.CLIPModel)
    assert m.text_model.cfg == tcfg and m.vision_model.cfg == vcfg           # eos_token_id 998, 3 / 2 layers, projection 64: not the ViT-L defaults
    assert m.text_model.with_projection and m.text_model.cfg.eos_token_id == 998
    direct = clip.CLIPModel(tcfg, vcfg, sd, device="cpu")
    for a, b in ((m.text_model.w, direct.text_model.w), (m.vision_model.w, direct.vision_model.w)):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    # a state dict with explicit configurations is the other route
    m2 = loading.load_clip(sd, device="cpu", text_config=tcfg, vision_config=vcfg)
    assert all(torch.equal(m2.vision_model.w[k], direct.vision_model.w[k]) for k in direct.vision_model.w)
    with pytest.raises(KeyError, match="lacks"):                             # ... and without them the ViT-L/14 defaults (12 layers) do not fit these weights
        loading.load_clip(sd, device="cpu")
    empty = tmp_path / "empty"
    empty.mkdir()
    _write_clip_dir(empty, tcfg, vcfg, sd, weights=False)
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        loading.load_clip(str(empty), device="cpu")
    bad = tmp_path / "bad"
    bad.mkdir()
    _write_clip_dir(bad, tcfg, dataclasses.replace(vcfg, num_channels=4), sd)
    with pytest.raises(ValueError, match="3 channels"):
        loading.load_clip(str(bad), device="cpu")
    mixed = tmp_path / "mixed"
    mixed.mkdir()
    _write_clip_dir(mixed, dataclasses.replace(tcfg, projection_dim=32), vcfg, sd)      # top-level projection_dim 32 reaches both towers
    with pytest.raises(ValueError, match="projection"):
        loading.load_clip(str(mixed), device="cpu")
