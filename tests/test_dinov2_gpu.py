"""The DINOv2 preservation score on the device against its oracles: torch's fp32 add for the token-assembly kernel (exact), transformers'
PIL image processor for the preprocessing kernel at resize 256 / crop 224 (exact), fp32 `transformers.Dinov2Model` on the CPU (same seeded
weights, rounded to fp16 first) for the tower and the scores.  Bars: rel-L2 < 1e-3 on pooler_output (the project's bar for every encoder);
|score difference| < 2e-3 (two unit vectors with relative errors e1, e2 move their cosine by at most e1 + e2 to first order).
The per-layer figures are printed, not asserted; profiles/r09_dinov2_parity.txt keeps one run of them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

REDUCED = dict(hidden_size=128, num_hidden_layers=4, num_attention_heads=2)          # image_size 518: the 37 x 37 table is resized


def _images(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n, h // 8, w // 8, 3), dtype=np.uint8)               # blocks + noise: structure at several scales
    img = np.repeat(np.repeat(base, 8, 1), 8, 2).astype(np.int64) + rng.integers(-40, 41, (n, h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _processor():
    import transformers
    from invertible_cd_amd import resample
    return transformers.BitImageProcessorPil(size={"shortest_edge": 256}, resample=3, crop_size=224,
                                             image_mean=list(resample.IMAGENET_MEAN), image_std=list(resample.IMAGENET_STD))


def _pixel_values(imgs):
    from PIL import Image
    return _processor()(images=[Image.fromarray(i) for i in imgs], return_tensors="pt")["pixel_values"]


def _oracle(cfg, sd):
    import transformers
    d = cfg.to_dict()
    d.pop("crop_size"); d.pop("resize_shortest_edge")                        # the image processor's, not the model's
    tc = transformers.Dinov2Config(**d)
    tc._attn_implementation = "eager"
    m = transformers.Dinov2Model(tc).eval().float()
    own = m.state_dict()
    assert all(k in sd or k == "embeddings.mask_token" for k in own)
    m.load_state_dict({k: (sd[k].float() if k in sd else v) for k, v in own.items()}, strict=True)
    return m


# ------------------------------------------------------------------------------------------------ 1. icd_vit_tokens
@pytest.mark.parametrize("B,n,C,lda", [(3, 5, 136, 144), (2, 256, 768, 768)])
def test_vit_tokens_is_torchs_fp32_add_bit_for_bit(B, n, C, lda):
    """C = 136 is a multiple of 8 and of nothing larger, with a padded accumulator whose pad columns hold NaN; 2 x 257 x 768 is the
    tower's own shape (several blocks).  One fp32 add and one rounding per element: exact equality."""
    from invertible_cd_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + C)
    acc = torch.randn(B * n, lda, generator=g)
    acc[:, C:] = float("nan")
    tok = torch.randn(1 + n, C, generator=g)
    out16, out32 = ops.vit_tokens(acc.cuda(), tok.cuda(), B)
    assert out16.dtype == torch.float16 and out32.dtype == torch.float32 and tuple(out16.shape) == tuple(out32.shape) == (B * (1 + n), C)
    want = torch.empty(B, 1 + n, C)
    want[:, 0] = tok[0]
    want[:, 1:] = acc[:, :C].reshape(B, n, C) + tok[1:]
    want = want.reshape(B * (1 + n), C)
    assert torch.equal(out32.cpu(), want)
    assert torch.equal(out16.cpu(), want.half())
    assert torch.isfinite(out32).all()


def test_vit_tokens_refuses_bad_arguments_before_any_launch():
    from invertible_cd_amd import _lib
    lib = _lib.load()
    INVALID = -1
    B, n, C = 2, 3, 16
    acc = torch.ones(B * n, C, device="cuda")
    tok = torch.ones(1 + n, C, device="cuda")
    o16 = torch.zeros(B * (1 + n), C, device="cuda", dtype=torch.float16)
    o32 = torch.zeros(B * (1 + n), C, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(acc=p(acc), lda=C, tok=p(tok), B=B, n=n, C=C, o16=p(o16), o32=p(o32)):
        return lib.icd_vit_tokens(acc, lda, tok, B, n, C, o16, o32, None)
    for kwargs, word in [(dict(C=12), "multiple of 8"), (dict(C=0), "multiple of 8"), (dict(acc=None), "null"), (dict(tok=None), "null"),
                         (dict(o16=None), "null"), (dict(o32=None), "null"), (dict(n=0), "positive"), (dict(B=0), "positive"),
                         (dict(B=-1), "positive"), (dict(lda=8), "lda"), (dict(lda=18), "lda"),
                         (dict(acc=ctypes.c_void_p(acc.data_ptr() + 4)), "aligned")]:
        assert call(**kwargs) == INVALID, kwargs
        assert word.encode() in lib.icd_last_error(), (kwargs, lib.icd_last_error())
    torch.cuda.synchronize()
    assert int(o16.count_nonzero()) == 0 and int(o32.count_nonzero()) == 0   # nothing was launched on the outputs
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((o32 == 2).reshape(B, 1 + n, C)[:, 1:].all()) and bool((o32 == 1).reshape(B, 1 + n, C)[:, 0].all())


# ------------------------------------------------------------------------------------------------ 2. preprocessing at 256 / 224
@pytest.mark.parametrize("h,w", [(256, 320), (300, 400), (333, 250), (512, 512)])
def test_preprocess_resize_256_crop_224_equals_the_pil_image_processor(h, w):
    """Resize to a shortest edge of 256 (341 on the long edge of 300 x 400, truncated), then a 224 crop that starts 16 pixels in:
    the kernel's tables are offset on both axes, which the CLIP geometry (resize = crop) never did."""
    from PIL import Image
    from invertible_cd_amd import ops, resample
    B = 3
    rng = np.random.default_rng(h + w)
    imgs = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    dev = torch.from_numpy(imgs).cuda()
    pm = ops.clip_preprocess(dev, 256, 224, 14, resample.IMAGENET_MEAN, resample.IMAGENET_STD)
    assert pm.is_cuda and pm.dtype == torch.float16 and tuple(pm.shape) == (B * 256, 592)
    pm = pm.cpu()
    assert (pm[:, 588:] == 0).all()
    # patch matrix -> [B, 3, 224, 224]
    px = pm[:, :588].reshape(B, 16, 16, 3, 14, 14).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224)
    ref = _pixel_values(imgs)
    mean = torch.tensor(resample.IMAGENET_MEAN).reshape(1, 3, 1, 1)
    std = torch.tensor(resample.IMAGENET_STD).reshape(1, 3, 1, 1)
    u_ref = torch.round((ref * std + mean) * 255)                            # the uint8 image after resize + crop, as PIL made it
    rh, rw, top, left = resample.clip_geometry(h, w, 256, 224)
    assert min(rh, rw) == 256 and top == (rh - 224) // 2 and left == (rw - 224) // 2
    for b in range(B):                                                       # ... which is Pillow's own resize, cropped
        pil = np.asarray(Image.fromarray(imgs[b]).resize((rw, rh), Image.BICUBIC))[top:top + 224, left:left + 224]
        assert np.array_equal(u_ref[b].permute(1, 2, 0).numpy().astype(np.uint8), pil)
    u_got = torch.round((px.float() * std + mean) * 255)
    assert torch.equal(u_got, u_ref), f"{int((u_got != u_ref).sum())} resized bytes differ from PIL"
    want = ((u_ref / 255 - mean) / std).to(torch.float16)                    # fp32 arithmetic, one rounding to fp16
    assert torch.equal(px, want)


# ------------------------------------------------------------------------------------------------ 3. / 4. the tower
def _tower(cfg, seed, B):
    from invertible_cd_amd import dinov2, synthetic
    sd = {k: v.half().float() for k, v in synthetic.synthetic_dinov2_state_dict(cfg, seed=seed).items()}
    imgs = _images(B, 256, 320, seed=seed)
    oracle = _oracle(cfg, sd)
    pv = _pixel_values(imgs)
    with torch.no_grad():
        ref = oracle(pixel_values=pv, output_hidden_states=True)
    assert len(ref.hidden_states) == cfg.num_hidden_layers + 1
    m = dinov2.Dinov2Model(cfg, sd)
    out = m(torch.from_numpy(imgs).cuda(), output_hidden_states=True)
    got, hs = out.pooler_output, out.hidden_states
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (B, cfg.hidden_size) and out[0] is got
    assert len(hs) == cfg.num_hidden_layers + 1
    with torch.no_grad():
        low = oracle.half().cuda()(pixel_values=pv.half().cuda(), output_hidden_states=True)
    growth = [rel_l2(g.float().cpu(), r) for g, r in zip(hs, ref.hidden_states)]
    floor_growth = [rel_l2(g.float().cpu(), r) for g, r in zip(low.hidden_states, ref.hidden_states)]
    return rel_l2(got.cpu(), ref.pooler_output), rel_l2(low.pooler_output.float().cpu(), ref.pooler_output), growth, floor_growth


def _report(name, e, floor, growth, floor_growth):
    print(f"[{name}] pooler_output rel-L2 = {e:.3e} (fp16-transformers floor {floor:.3e})")
    print("    per layer (embeddings first): " + " ".join(f"{g:.1e}" for g in growth))
    print("    fp16 floor per layer:         " + " ".join(f"{g:.1e}" for g in floor_growth))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_dinov2_reduced_width_matches_transformers(seed):
    from invertible_cd_amd import dinov2
    e, floor, growth, fg = _tower(dinov2.Dinov2Config(**REDUCED), seed, B=3)
    _report(f"dinov2 4 x 128, seed {seed}", e, floor, growth, fg)
    assert e < 1e-3


def test_dinov2_base_matches_transformers():
    """facebook/dinov2-base at full size (12 x 768, 257 tokens, the 37 x 37 position table resized to 16 x 16) on seeded weights."""
    from invertible_cd_amd import dinov2
    e, floor, growth, fg = _tower(dinov2.DINOV2_BASE, 5, B=2)
    _report("dinov2-base", e, floor, growth, fg)
    assert e < 1e-3


# ------------------------------------------------------------------------------------------------ 5. scores
@functools.lru_cache(maxsize=1)
def _scorer(seed=4):
    """(HIP Dinov2Model, fp32 transformers oracle) on one set of reduced seeded weights, built once for the score tests."""
    from invertible_cd_amd import dinov2, synthetic
    cfg = dinov2.Dinov2Config(**REDUCED)
    sd = {k: v.half().float() for k, v in synthetic.synthetic_dinov2_state_dict(cfg, seed=seed).items()}
    return dinov2.Dinov2Model(cfg, sd), _oracle(cfg, sd)


def _unit(x):
    return x / torch.norm(x, dim=-1, keepdim=True)


def test_dinov2_scores_match_the_fp32_oracle_embeddings(monkeypatch):
    from PIL import Image
    from invertible_cd_amd import metrics
    model, oracle = _scorer()
    N = 5
    a, b = _images(N, 512, 512, seed=8), _images(N, 512, 512, seed=9)
    b[0] = a[0]
    with torch.no_grad():
        ea, eb = (_unit(oracle(pixel_values=_pixel_values(x)).pooler_output) for x in (a, b))
    want = (eb * ea).sum(-1)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    # the device-tensor route: only the scores cross to the host
    crossed = []
    real_cpu, real_numpy, real_to = torch.Tensor.cpu, torch.Tensor.numpy, torch.Tensor.to

    def spy_to(self, *args, **kw):
        out = real_to(self, *args, **kw)
        if self.is_cuda and not out.is_cuda:
            crossed.append(self.numel())
        return out
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", lambda self, *args, **kw: (crossed.append(self.numel()), real_cpu(self, *args, **kw))[1])
        mp.setattr(torch.Tensor, "numpy", lambda self, *args, **kw: (crossed.append(self.numel()), real_numpy(self, *args, **kw))[1])
        mp.setattr(torch.Tensor, "to", spy_to)
        got = metrics.calc_dinov2_images_images(da, db, "cuda", batch_size=2, model=model)
    assert crossed == [2, 2, 1], crossed                                     # three batches of scores; no image (786432 bytes each) among them
    assert not got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (N,)
    d = float((got - want).abs().max())
    print(f"[dinov2 scores] max |score - oracle| = {d:.3e}; scores " + " ".join(f"{float(s):.4f}" for s in got))
    assert d < 2e-3
    assert abs(float(got[0]) - 1.0) < 1e-6                                   # identical images: identical embeddings
    # host arrays and PIL images take the same route after an upload
    host = metrics.calc_dinov2_images_images(list(a), list(b), "cuda", batch_size=50, model=model)
    pil = metrics.calc_dinov2_images_images([Image.fromarray(x) for x in a], [Image.fromarray(x) for x in b], "cuda", model=model)
    stacked = metrics.calc_dinov2_images_images(a, b, "cuda", batch_size=3, model=model)
    assert torch.equal(host, got) and torch.equal(pil, got) and torch.equal(stacked, got)


def test_dinov2_scores_of_a_list_of_mixed_sizes_keep_the_callers_order():
    from invertible_cd_amd import metrics
    model, _ = _scorer()
    a, b = _images(3, 264, 328, seed=3)[:, :-5, :-5], _images(3, 264, 328, seed=4)[:, :-5, :-5]      # 259 x 323: odd sizes
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    c, d = _images(2, 256, 320, seed=5), _images(2, 256, 320, seed=6)
    odd = metrics.calc_dinov2_images_images(list(a), list(b), "cuda", model=model)
    small = metrics.calc_dinov2_images_images(list(c), list(d), "cuda", model=model)
    la, lb = [a[0], c[0], a[1], c[1], a[2]], [b[0], d[0], b[1], d[1], b[2]]
    mixed = metrics.calc_dinov2_images_images(la, lb, "cuda", model=model)
    assert torch.isfinite(mixed).all() and len(set(mixed.tolist())) == 5
    assert torch.equal(mixed[0::2], odd) and torch.equal(mixed[1::2], small)


# ------------------------------------------------------------------------------------------------ 6. the loader
def test_load_dinov2_from_a_directory_gives_the_embeddings_of_the_state_dict(tmp_path):
    import json
    from safetensors.torch import save_file
    from invertible_cd_amd import dinov2, loading, synthetic
    cfg = dinov2.Dinov2Config(**REDUCED)
    sd = {k: v.half().float() for k, v in synthetic.synthetic_dinov2_state_dict(cfg, seed=7).items()}
    d = cfg.to_dict()
    d.pop("crop_size"); d.pop("resize_shortest_edge")
    (tmp_path / "config.json").write_text(json.dumps(dict(d, model_type="dinov2")))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    loaded, direct = loading.load_dinov2(str(tmp_path)), dinov2.Dinov2Model(cfg, sd)
    assert loaded.cfg == cfg
    imgs = torch.from_numpy(_images(2, 256, 320, seed=2)).cuda()
    e = loaded(imgs).pooler_output
    assert e.is_cuda and e.dtype == torch.float32 and tuple(e.shape) == (2, 128)
    assert torch.equal(e, direct(imgs).pooler_output) and torch.equal(e, direct.get_image_features(imgs))
