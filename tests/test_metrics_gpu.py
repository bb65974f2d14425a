"""Edit-quality metrics on the device against their oracles: Pillow / transformers' PIL image processor for the preprocessing kernel,
the fp32 `transformers` CLIP classes on the CPU (same seeded weights) for the image tower and the scores, torch integer / float64
arithmetic for the two reductions.  Bars: exact equality where the arithmetic is integer; rel-L2 < 1e-3 on image_embeds (the project's
bar for every encoder); |score difference| < 2e-3 (two unit vectors with relative errors e1, e2 move their cosine by at most e1 + e2 to
first order)."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

SMALL = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=4, num_attention_heads=2, projection_dim=64)


def _images(shapes_or_n, h=None, w=None, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (shapes_or_n, h // 8, w // 8, 3), dtype=np.uint8)          # blocks + noise: structure at several scales
    img = np.repeat(np.repeat(base, 8, 1), 8, 2).astype(np.int64) + rng.integers(-40, 41, (shapes_or_n, h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 4. preprocessing kernel
@pytest.mark.parametrize("h,w", [(512, 512), (1024, 1024), (480, 640), (640, 480), (200, 200), (333, 517)])
def test_clip_preprocess_equals_the_pil_image_processor(h, w):
    import transformers
    from PIL import Image
    from invertible_cd_amd import ops, resample
    B = 3
    rng = np.random.default_rng(h + w)
    imgs = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    dev = torch.from_numpy(imgs).cuda()
    pm = ops.clip_preprocess(dev)
    assert pm.is_cuda and pm.dtype == torch.float16 and tuple(pm.shape) == (B * 256, 592)
    pm = pm.cpu()
    assert (pm[:, 588:] == 0).all()
    # patch matrix -> [B, 3, 224, 224]
    px = pm[:, :588].reshape(B, 16, 16, 3, 14, 14).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224)
    proc = transformers.CLIPImageProcessorPil()
    ref = proc(images=[Image.fromarray(i) for i in imgs], return_tensors="pt")["pixel_values"]
    mean = torch.tensor(resample.CLIP_MEAN).reshape(1, 3, 1, 1)
    std = torch.tensor(resample.CLIP_STD).reshape(1, 3, 1, 1)
    u_ref = torch.round((ref * std + mean) * 255)                            # the uint8 image after resize + crop, as PIL made it
    rh, rw, top, left = resample.clip_geometry(h, w)
    for b in range(B):                                                       # ... which is Pillow's own resize, cropped
        pil = np.asarray(Image.fromarray(imgs[b]).resize((rw, rh), Image.BICUBIC))[top:top + 224, left:left + 224]
        assert np.array_equal(u_ref[b].permute(1, 2, 0).numpy().astype(np.uint8), pil)
    u_got = torch.round((px.float() * std + mean) * 255)
    assert torch.equal(u_got, u_ref), f"{int((u_got != u_ref).sum())} resized bytes differ from PIL"
    want = ((u_ref / 255 - mean) / std).to(torch.float16)                    # fp32 arithmetic, one rounding to fp16
    assert torch.equal(px, want)


# ------------------------------------------------------------------------------------------------ attention at the tower's shape
def test_flash_attention_non_causal_257_tokens_masks_the_key_tail():
    """The image tower's attention shape (T = 257, d = 64, V^T leading dimension 264, no mask) against torch in fp32: the 7 pad keys of
    the ragged last tile must not be attended and the ragged last query tile must not be written out of range."""
    from invertible_cd_amd import ops
    B, H, T, d, ld = 2, 4, 257, 64, 264
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(B * T, H * d, generator=g).half() for _ in range(3))
    vt = torch.full((B, H * d, ld), 100.0, dtype=torch.float16)              # poison in the pad columns: a leak would be visible
    vt[:, :, :T] = v.reshape(B, T, H * d).permute(0, 2, 1)
    out = ops.attention_fused(q.cuda(), k.cuda(), vt.cuda(), B, H, T, T, d, d ** -0.5, causal=False).float().cpu()
    qf, kf, vf = (t.float().reshape(B, T, H, d).permute(0, 2, 1, 3) for t in (q, k, v))
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) * d ** -0.5, -1) @ vf).permute(0, 2, 1, 3).reshape(B * T, H * d)
    e = rel_l2(out, ref)
    print(f"[attention 257 x 257, d 64, non-causal] rel-L2 = {e:.3e}")
    assert e < 2e-3                                                          # the bar tests/test_ops_gpu.py sets for fp16 P


# ------------------------------------------------------------------------------------------------ 5. image tower
def _oracle(cfg, sd):
    import transformers
    tc = transformers.CLIPVisionConfig(**cfg.to_dict())
    tc._attn_implementation = "eager"
    m = transformers.CLIPVisionModelWithProjection(tc).eval().float()
    own = m.state_dict()
    new = {k: (sd[k].float() if k in sd else v) for k, v in own.items()}
    assert all(k in sd or k.endswith("position_ids") for k in own)
    m.load_state_dict(new, strict=True)
    return m


def _pixel_values(imgs):
    import transformers
    from PIL import Image
    return transformers.CLIPImageProcessorPil()(images=[Image.fromarray(i) for i in imgs], return_tensors="pt")["pixel_values"]


def _tower(cfg, seed, B):
    from invertible_cd_amd import clip, synthetic
    sd = {k: v.half().float() for k, v in synthetic.synthetic_clip_vision_state_dict(cfg, seed=seed).items()}
    imgs = _images(B, 256, 320, seed=seed)
    oracle = _oracle(cfg, sd)
    pv = _pixel_values(imgs)
    with torch.no_grad():
        ref = oracle(pixel_values=pv, output_hidden_states=True)
    m = clip.CLIPVisionModelWithProjection(cfg, sd)
    dev_imgs = torch.from_numpy(imgs).cuda()
    got, hs = m.forward_patches(m.preprocess(dev_imgs), output_hidden_states=True)
    assert got.is_cuda and got.dtype == torch.float32
    with torch.no_grad():
        floor = oracle.half().cuda()(pixel_values=pv.half().cuda()).image_embeds.float().cpu()
    growth = [rel_l2(g.float().cpu(), r) for g, r in zip(hs, ref.hidden_states)]
    return rel_l2(got.cpu(), ref.image_embeds), rel_l2(floor, ref.image_embeds), growth


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_image_tower_reduced_width_matches_transformers(seed):
    from invertible_cd_amd import clip
    e, floor, growth = _tower(clip.CLIPVisionConfig(**SMALL), seed, B=3)
    print(f"[image tower 4 x 128, seed {seed}] image_embeds rel-L2 = {e:.3e} (fp16-torch floor {floor:.3e}); per layer " +
          " ".join(f"{g:.1e}" for g in growth))
    assert e < 1e-3


def test_image_tower_full_vit_l_14_matches_transformers():
    """openai/clip-vit-large-patch14's image tower at full size (24 x 1024, 257 tokens) on seeded weights."""
    from invertible_cd_amd import clip
    e, floor, growth = _tower(clip.CLIP_VIT_L_VISION, 5, B=2)
    print(f"[image tower ViT-L/14] image_embeds rel-L2 = {e:.3e} (fp16-torch floor {floor:.3e}); per layer " +
          " ".join(f"{g:.1e}" for g in growth))
    assert e < 1e-3


# ------------------------------------------------------------------------------------------------ 6. scores
def _clip_model(seed=4):
    """(HIP CLIPModel, fp32 transformers text + vision oracles) on one set of reduced seeded weights."""
    import transformers
    from invertible_cd_amd import clip, synthetic
    from oracle import clip_ref
    tcfg = clip.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2,
                               projection_dim=64)
    vcfg = clip.CLIPVisionConfig(**SMALL)
    sd = {k: v.half().float() for k, v in synthetic.synthetic_clip_state_dict(tcfg, True, seed=seed).items()}
    sd.update({k: v.half().float() for k, v in synthetic.synthetic_clip_vision_state_dict(vcfg, seed=seed).items()})
    text = clip_ref.build(tcfg.to_dict(), {k: v for k, v in sd.items() if k.startswith("text_") }, True)
    vision = _oracle(vcfg, sd)
    return clip.CLIPModel(tcfg, vcfg, sd), text, vision, tcfg


def _unit(x):
    return x / torch.norm(x, dim=-1, keepdim=True)


def test_clip_scores_match_the_fp32_oracle_embeddings():
    from invertible_cd_amd import metrics
    from test_clip_gpu import _ids
    model, text, vision, tcfg = _clip_model()
    N = 5
    a, b = _images(N, 512, 512, seed=8), _images(N, 512, 512, seed=9)
    b[0] = a[0]
    ids = _ids(N, 77, tcfg.vocab_size, 3)
    with torch.no_grad():
        ea, eb = (_unit(vision(pixel_values=_pixel_values(x)).image_embeds) for x in (a, b))
        et = _unit(text(ids).text_embeds)
    want_ii, want_it = (eb * ea).sum(-1), (et * eb).sum(-1)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got_ii = metrics.calc_clip_score_images_images(da, db, "cuda", batch_size=2, model=model)
    got_it = metrics.calc_clip_score_images_prompts(db, ids, "cuda", batch_size=2, model=model)
    assert not got_ii.is_cuda and got_ii.dtype == torch.float32 and tuple(got_ii.shape) == (N,)
    d_ii, d_it = float((got_ii - want_ii).abs().max()), float((got_it - want_it).abs().max())
    print(f"[clip scores] max |score - oracle|: images-images {d_ii:.3e}, images-prompts {d_it:.3e}")
    assert d_ii < 2e-3 and d_it < 2e-3
    assert abs(float(got_ii[0]) - 1.0) < 1e-6                                # identical images: identical embeddings
    # host images take the same route after an upload
    host = metrics.calc_clip_score_images_images(list(a), list(b), "cuda", batch_size=50, model=model)
    assert torch.equal(host, got_ii)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_cosine_rows_against_float64(dtype):
    """Bound: a length-768 fp32 dot product accumulated in any order errs by at most 768 * 2^-24 = 4.6e-5 relative to sum |a_i b_i|
    (the classical n * u bound), and the three sums enter the cosine once each, so |error| <= 3 * n * u ~ 1.4e-4 for a cosine whose
    terms do not cancel; the assertion uses 1e-5, which the measured worst case over seeds 0 .. 4 on both dtypes (fp32 6.2e-8, fp16
    inputs 7.9e-8, profiles/r08_metrics_parity.txt) clears by more than 100 x."""
    from invertible_cd_amd import ops
    worst = 0.0
    for seed in range(5):
        g = torch.Generator().manual_seed(seed)
        a = torch.randn(37, 768, generator=g).to(dtype)
        b = (0.5 * a.float() + torch.randn(37, 768, generator=g)).to(dtype)
        got = ops.cosine_rows(a.cuda(), b.cuda()).cpu().double()
        a64, b64 = a.double(), b.double()
        want = (a64 * b64).sum(-1) / (a64.norm(dim=-1) * b64.norm(dim=-1))
        worst = max(worst, float((got - want).abs().max()))
    print(f"[cosine_rows {dtype}] worst |error| vs float64 over 5 seeds = {worst:.3e}")
    assert worst < 1e-5
    # a width that is not a multiple of the vector length, and a strided operand
    a = torch.randn(9, 70, generator=torch.Generator().manual_seed(1)).to(dtype).cuda()
    wide = torch.randn(9, 77, generator=torch.Generator().manual_seed(2)).to(dtype).cuda()
    b = wide[:, 3:73]
    want = torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)
    assert float((ops.cosine_rows(a, b).double() - want).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ 7. squared differences, PSNR
def test_sq_diff_sum_is_exact_and_psnr_on_the_device_is_the_host_value():
    from invertible_cd_amd import metrics, ops
    g = torch.Generator().manual_seed(0)
    for shape in [(3, 512, 512, 3), (2, 33, 47, 3), (5, 1), (1, 1024 * 1024 * 3 + 5)]:
        a = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        b = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        want = ((a.long() - b.long()) ** 2).reshape(shape[0], -1).sum(-1)
        got = ops.sq_diff_sum_u8(a.cuda(), b.cuda()).cpu()
        assert got.dtype == torch.int64 and torch.equal(got, want), shape
    lo, hi = torch.zeros(1, 1024, 1024, 3, dtype=torch.uint8), torch.full((1, 1024, 1024, 3), 255, dtype=torch.uint8)
    assert ops.sq_diff_sum_u8(lo.cuda(), hi.cuda()).cpu().tolist() == [1024 * 1024 * 3 * 255 * 255]
    a, b = _images(3, 64, 48, seed=1), _images(3, 64, 48, seed=2)
    host = metrics.calculate_psnr(list(a), list(b), "cpu")
    want = [20 * math.log10(255.0 / math.sqrt(np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2))) for x, y in zip(a, b)]
    dev = metrics.calculate_psnr(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), "cuda", batch_size=2)
    assert host == want and dev == want
    assert metrics.calculate_psnr(torch.from_numpy(a).cuda(), torch.from_numpy(a).cuda(), "cuda") == float("inf")


# ------------------------------------------------------------------------------------------------ 8. images stay on the device
def test_runner_keeps_images_on_the_device_and_scores_them_there(monkeypatch):
    """A ControllerBatch edit of two pairs on the stub UNet + SyntheticVAE: return_type='uint8_device' gives the bytes of
    return_type='image', on the device; the scores computed from the device tensor equal those of the host-image route, and no image
    crosses to the host on the way (every tensor the metric path sees is a cuda tensor)."""
    from stubs import StubModel, StubScheduler
    from invertible_cd_amd import generation as G, metrics, ops, p2p, synthetic
    m = StubModel()
    m.device, m.vae = torch.device("cuda"), synthetic.SyntheticVAE("cuda", torch.float32)
    s = G.Generator(m, 50, StubScheduler(), forward_cons_model=m, reverse_cons_model=m,
                    reverse_timesteps=[259, 519, 779, 999], forward_timesteps=[19, 259, 519, 779])

    def init_prompt(prompt, unc=None):
        s.context, s.prompt = torch.zeros(2 * len(prompt), 77, 8, device="cuda"), prompt
    s.init_prompt = init_prompt
    groups = [["a cat on a bench", "a dog on a bench"], ["a red car", "a blue car"]]
    for name, val in (('tokenizer', m.tokenizer), ('NUM_DDIM_STEPS', 4), ('device', 'cuda')):
        monkeypatch.setattr(p2p, name, val)
    kw = dict(is_cons_forward=True, guidance_scale=19.0, dynamic_guidance=True, tau1=0.8, tau2=0.8, w_embed_dim=512)
    outs = {}
    for rt in ("image", "uint8_device"):
        batch = p2p.ControllerBatch([p2p.make_controller(p, True, 0.5, 0.5) for p in groups])
        outs[rt], _ = G.runner(model=m, prompt=groups, controller=batch, solver=s, generator=torch.Generator().manual_seed(21),
                               return_type=rt, **kw)
    host, dev = outs["image"], outs["uint8_device"]
    assert isinstance(host, np.ndarray) and host.shape == (4, 512, 512, 3)
    assert dev.is_cuda and dev.dtype == torch.uint8 and torch.equal(dev.cpu(), torch.from_numpy(host))
    assert host.std() > 0
    model, _, _, tcfg = _clip_model()
    seen = []
    real = ops.clip_preprocess
    monkeypatch.setattr(ops, "clip_preprocess", lambda images, *a, **k: (seen.append(images.is_cuda and images.data_ptr()), real(images, *a, **k))[1])
    src, edit = dev[0::2], dev[1::2].contiguous()
    src = src.contiguous()
    from test_clip_gpu import _ids
    ids = _ids(2, 77, tcfg.vocab_size, 6)                                    # token ids of the two edit prompts (no vocabulary offline)
    pres = metrics.calc_clip_score_images_images(src, edit, "cuda", model=model)
    edsc = metrics.calc_clip_score_images_prompts(edit, ids, "cuda", model=model)
    psnr = metrics.calculate_psnr(src, edit, "cuda")
    assert seen == [src.data_ptr(), edit.data_ptr(), edit.data_ptr()]        # the very tensors, not copies that went through the host
    assert torch.equal(pres, metrics.calc_clip_score_images_images(list(host[0::2]), list(host[1::2]), "cuda", model=model))
    assert torch.equal(edsc, metrics.calc_clip_score_images_prompts(list(host[1::2]), ids, "cuda", model=model))
    assert psnr == metrics.calculate_psnr(list(host[0::2]), list(host[1::2]), "cpu")
    assert torch.isfinite(pres).all() and torch.isfinite(edsc).all()


# ------------------------------------------------------------------------------------------------ 9. C-ABI refusals
def test_new_entries_refuse_bad_arguments_before_any_launch():
    from invertible_cd_amd import _lib, resample
    lib = _lib.load()
    INVALID = -1
    x = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(x.data_ptr())
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    taps = resample.tap_width(512, 224)

    def pre(images=p, B=1, H=512, W=512, rh=224, rw=224, ht=taps, vt=taps, tab=p, tmp=p, out=p):
        return lib.icd_clip_preprocess(images, B, H, W, rh, rw, 224, 14, tab, tab, tab, ht, tab, tab, tab, vt, f3, f3, tmp, out, 592, None)
    for kwargs, word in [(dict(images=None), "null"), (dict(tab=None), "null"), (dict(out=None), "null"), (dict(B=0), "B must be positive"),
                         (dict(H=0), "positive"), (dict(W=-3), "positive"), (dict(rw=200), "smaller than the crop"),
                         (dict(ht=taps + 2), "do not match"), (dict(H=1024), "do not match")]:
        assert pre(**kwargs) == INVALID, kwargs
        assert word.encode() in lib.icd_last_error(), (kwargs, lib.icd_last_error())
    out = ctypes.c_void_p(x.data_ptr())
    for args, word in [((None, p, 4, 8, 8, 8, 0, out, None), "null"), ((p, p, 0, 8, 8, 8, 0, out, None), "bad shape"),
                       ((p, p, 4, 8, 4, 8, 0, out, None), "bad shape"), ((p, p, 4, 8, 8, 8, 2, out, None), "is_f32")]:
        assert lib.icd_cosine_rows(*args) == INVALID and word.encode() in lib.icd_last_error(), args
    for args, word in [((p, None, 1, 16, out, None), "null"), ((p, p, 0, 16, out, None), "rows"), ((p, p, 1, 0, out, None), "rows"),
                       ((p, p, 70000, 16, out, None), "rows")]:
        assert lib.icd_sq_diff_sum_u8(*args) == INVALID and word.encode() in lib.icd_last_error(), args
    torch.cuda.synchronize()
    assert int(x.sum()) == 0                                                 # nothing was launched on the buffer


# ------------------------------------------------------------------------------------------------ slices, mixed sizes, the loader
def test_clip_preprocess_on_slices_that_start_at_any_byte():
    """images[i:] of a batch whose images are not a multiple of 16 bytes starts at an unaligned address: the kernel takes it as it is and
    gives the bytes of the same images preprocessed as a batch of their own."""
    from invertible_cd_amd import ops
    rng = np.random.default_rng(12)
    for h, w in [(250, 250), (333, 517)]:
        assert (h * w * 3) % 16
        imgs = torch.from_numpy(rng.integers(0, 256, (4, h, w, 3), dtype=np.uint8)).cuda()
        whole = ops.clip_preprocess(imgs)
        for i in (1, 2, 3):
            view = imgs[i:]
            assert view.data_ptr() % 16 and view.is_contiguous()
            assert torch.equal(ops.clip_preprocess(view), whole[i * 256:])
        assert torch.equal(ops.clip_preprocess(imgs[1:].clone()), whole[256:])


def test_scores_in_batches_of_odd_sized_images_and_lists_of_mixed_sizes():
    from invertible_cd_amd import metrics
    model, _, _, _ = _clip_model()
    a, b = _images(5, 248, 328, seed=3)[:, :-5, :-5], _images(5, 248, 328, seed=4)[:, :-5, :-5]       # 243 x 323: 235467 bytes per image
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    one = metrics.calc_clip_score_images_images(da, db, "cuda", batch_size=50, model=model)
    two = metrics.calc_clip_score_images_images(da, db, "cuda", batch_size=2, model=model)           # batches 2 and 3 start at unaligned bytes
    assert torch.equal(one, two) and torch.isfinite(one).all()
    # a list that mixes sizes: each image scores what it scores in a list of its own size
    c, d = _images(2, 256, 320, seed=5), _images(2, 256, 320, seed=6)
    la, lb = [a[0], c[0], a[1], c[1]], [b[0], d[0], b[1], d[1]]
    mixed = metrics.calc_clip_score_images_images(la, lb, "cuda", model=model)
    small = metrics.calc_clip_score_images_images(list(c), list(d), "cuda", model=model)
    assert torch.equal(mixed[0::2], one[:2]) and torch.equal(mixed[1::2], small)


def test_load_clip_from_a_directory_gives_the_embeddings_of_the_state_dict(tmp_path):
    from test_clip_gpu import _ids
    from test_metrics import _reduced_clip, _write_clip_dir
    from invertible_cd_amd import clip, loading
    tcfg, vcfg, sd = _reduced_clip()
    sd = {k: v.half().float() for k, v in sd.items()}
    _write_clip_dir(tmp_path, tcfg, vcfg, sd)
    loaded, direct = loading.load_clip(str(tmp_path)), clip.CLIPModel(tcfg, vcfg, sd)
    assert loaded.text_model.cfg == tcfg and loaded.vision_model.cfg == vcfg
    imgs = torch.from_numpy(_images(2, 256, 320, seed=2)).cuda()
    ids = _ids(2, 77, tcfg.vocab_size, 9)
    ei, et = loaded.get_image_features(imgs), loaded.get_text_features(ids)
    assert ei.is_cuda and tuple(ei.shape) == (2, 64) and tuple(et.shape) == (2, 64)
    assert torch.equal(ei, direct.get_image_features(imgs)) and torch.equal(et, direct.get_text_features(ids))
    # eos_token_id from config.json switches the text tower's pooling rule: 998 is the first token of these ids, the ViT-L default (2: argmax
    # of the ids) pools at the first 999
    import dataclasses
    legacy = clip.CLIPModel(dataclasses.replace(tcfg, eos_token_id=2), vcfg, sd)
    assert not torch.equal(legacy.get_text_features(ids), et)


def test_uint8_images_on_the_device_are_the_host_bytes_in_fp16_too():
    """Generator.latent2image / latent2image(on_device=True) against the host expression on a decoded fp16 sample (numpy fp16 and torch
    fp16 both multiply through fp32 and round once), and on fp32."""
    from invertible_cd_amd.generation import _to_uint8_device
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float16, torch.float32):
        x = (1.3 * torch.randn(2, 3, 64, 96, generator=g)).to(dtype).cuda()
        x[0, 0, 0, :8] = torch.tensor([-1.0, 1.0, 0.0, 0.999, -0.999, 0.5, 2.0, -2.0], dtype=dtype)
        host = (x / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
        host = (host * 255).astype(np.uint8)
        dev = _to_uint8_device(x)
        assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), host)


def test_clip_preprocess_refuses_a_patch_row_that_does_not_fit_in_lds():
    from invertible_cd_amd import _lib, resample
    lib = _lib.load()
    x = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(x.data_ptr())
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    t = resample.tap_width(512, 448)
    rc = lib.icd_clip_preprocess(p, 1, 512, 512, 448, 448, 448, 64, p, p, p, t, p, p, p, t, f3, f3, p, p, 3 * 64 * 64, None)
    assert rc == -1 and b"LDS" in lib.icd_last_error()
    torch.cuda.synchronize()
    assert int(x.sum()) == 0
