"""ImageReward on the device against its oracles: float64 torch for icd_attention_masked and icd_layernorm_f32, Pillow for the
preprocessing at 224, fp32 `transformers` BlipVisionModel / BlipTextModel (blip_ref.py, same seeded weights rounded to fp16) for the
towers and the score.  Bars: the kernels' own (below); rel-L2 < 1e-3 on every tower's last_hidden_state (the project's bar for every
tower); |score - oracle| <= 1e-3 ||w|| ||cls|| (Cauchy-Schwarz on the feature bar; 1 / std is inside w).
Every measured figure is printed; with ICD_PARITY_LOG=<file> it is appended there too (profiles/r15_blip_parity.txt keeps one run)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import blip_ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _record(line):
    print(line)
    path = os.environ.get("ICD_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------ 1. icd_attention_masked
def _attn_case(B, H, Nq, Nk, d, counts, seed, wide=False, vt_pad=float("nan")):
    """q, k [B, N, ld], vt [B, H d, ldvt], out [B, Nq, ldo] on the device; with `wide` the leading dims exceed H d / pad8(Nk).  The
    padding holds NaN (q, k, and vt unless `vt_pad` says otherwise) or a sentinel (out)."""
    g = torch.Generator().manual_seed(seed)
    C = H * d
    ldq, ldk, ldo, ldvt = (C + 8, C + 16, C + 4, (Nk + 7) // 8 * 8 + 8) if wide else (C, C, C, (Nk + 7) // 8 * 8)
    q = torch.full((B, Nq, ldq), float("nan"), dtype=torch.float16)
    k = torch.full((B, Nk, ldk), float("nan"), dtype=torch.float16)
    vt = torch.full((B, C, ldvt), vt_pad, dtype=torch.float16)
    q[..., :C] = (torch.randn(B, Nq, C, generator=g) * 1.5).half()
    k[..., :C] = (torch.randn(B, Nk, C, generator=g) * 1.5).half()
    vt[..., :Nk] = torch.randn(B, C, Nk, generator=g).half()
    out = torch.full((B, Nq, ldo), 7.0, dtype=torch.float16)
    return q.cuda(), k.cuda(), vt.cuda(), out.cuda(), torch.tensor(counts, dtype=torch.int32).cuda()


def _attn_run(q, k, vt, out, counts, H, d, scale, fused=False):
    from invertible_cd_amd import _lib
    lib = _lib.load()
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if fused:
        _lib.check(lib.icd_attention_fused(p(q), p(k), p(vt), p(out), B, H, Nq, Nk, d, q.stride(1), k.stride(1), vt.stride(1), out.stride(1),
                                           vt.stride(0), scale, st), "icd_attention_fused")
    else:
        _lib.check(lib.icd_attention_masked(p(q), p(k), p(vt), p(out), p(counts), B, H, Nq, Nk, d, q.stride(1), k.stride(1), vt.stride(1),
                                            out.stride(1), vt.stride(0), scale, st), "icd_attention_masked")
    torch.cuda.synchronize()
    return out


def _attn_ref(q, k, vt, counts, H, d, scale, dtype):
    """softmax(scale q k^T with the scores of keys >= count at -inf) v in `dtype` on the operands' device -> [B, Nq, H d]; a sample
    without keys gives zeros"""
    B, Nq, Nk, C = q.shape[0], q.shape[1], k.shape[1], H * d
    heads = lambda t, n: t[..., :C].to(dtype).reshape(B, n, H, d).permute(0, 2, 1, 3)
    v = vt[..., :Nk].to(dtype).reshape(B, H, d, Nk).transpose(-1, -2)
    s = heads(q, Nq) @ heads(k, Nk).transpose(-1, -2) * scale
    kc = counts.clamp(0, Nk).to(s.device)
    dead = torch.arange(Nk, device=s.device)[None, :] >= kc[:, None]
    s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    p = torch.nan_to_num(s.softmax(-1), nan=0.0)                 # a row of -inf only: zeros
    return (p @ v).permute(0, 2, 1, 3).reshape(B, Nq, C)


def _attn_check(name, B, H, Nq, Nk, d, counts, seed, wide=False, against_fused=False):
    scale = d ** -0.5
    # (icd_attention_fused asks for zeros in the pad columns of V^T, as ops.project_vt writes them; the masked kernel reads past none)
    q, k, vt, out, kc = _attn_case(B, H, Nq, Nk, d, counts, seed, wide, vt_pad=0.0 if against_fused else float("nan"))
    got = _attn_run(q, k, vt, out, kc, H, d, scale)
    C = H * d
    assert bool((got[..., C:] == 7.0).all()), "the padding of out was written"
    got = got[..., :C]
    assert bool(torch.isfinite(got).all())
    want = _attn_ref(q.cpu(), k.cpu(), vt.cpu(), kc.cpu(), H, d, scale, torch.float64)
    low = _attn_ref(q, k, vt, kc, H, d, scale, torch.float16).cpu()
    fused = None
    if against_fused:
        fused = _attn_run(q, k, vt, torch.full_like(out, 7.0), kc, H, d, scale, fused=True)[..., :C].cpu()
    for b in range(B):
        n = min(max(int(counts[b]), 0), Nk)
        if n == 0:
            assert int(got[b].count_nonzero()) == 0
            _record(f"[attention_masked {name}] sample {b} count {counts[b]}: zeros")
            continue
        e, floor = rel_l2(got[b].cpu(), want[b]), rel_l2(low[b], want[b])
        line = f"[attention_masked {name}] sample {b} count {counts[b]}: rel-L2 {e:.3e}, fp16 torch {floor:.3e}, bound {1.5 * floor:.3e}"
        if fused is not None:
            ef = rel_l2(got[b].cpu(), fused[b])
            line += f", against icd_attention_fused {ef:.3e}"
        _record(line)
        assert e <= 1.5 * floor, line
        if fused is not None:
            assert ef <= 1.5 * floor, line


def test_attention_masked_at_the_text_towers_shape():
    _attn_check("35x35 d64", 6, 2, 35, 35, 64, [1, 2, 31, 32, 33, 35], seed=1)


@pytest.mark.parametrize("N", [1, 32, 33, 64, 65, 128])
def test_attention_masked_at_every_key_tile_edge(N):
    _attn_check(f"{N}x{N} d64", 4, 2, N, N, 64, [1, N, N, 1], seed=N)


@pytest.mark.parametrize("d", [8, 40, 64, 128])
def test_attention_masked_head_dims(d):
    _attn_check(f"35x35 d{d}", 3, 2, 35, 35, d, [5, 35, 17], seed=d)


def test_attention_masked_more_queries_than_keys():
    _attn_check("200x35 d64", 2, 2, 200, 35, 64, [35, 9], seed=7)


def test_attention_masked_zero_and_oversized_counts():
    _attn_check("35x35 d64 counts 0, -3, 36, 1000", 5, 2, 35, 35, 64, [0, -3, 36, 1000, 12], seed=8)


def test_attention_masked_ignores_the_padding_of_wide_operands():
    _attn_check("35x35 d64 wide", 3, 2, 35, 35, 64, [3, 35, 20], seed=9, wide=True)
    _attn_check("65x65 d40 wide", 2, 3, 65, 65, 40, [64, 65], seed=10, wide=True)


@pytest.mark.parametrize("N,d", [(35, 64), (128, 64), (33, 40)])
def test_attention_masked_with_full_counts_is_attention_fused(N, d):
    _attn_check(f"{N}x{N} d{d} full", 3, 2, N, N, d, [N, N, N], seed=N + d, against_fused=True)


# ------------------------------------------------------------------------------------------------ 2. icd_layernorm_f32
def _ulp16(x):
    """the spacing of fp16 at |x| (float64 tensor), the subnormal spacing below 2^-14"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return 2.0 ** (e - 10)


@pytest.mark.parametrize("C", [8, 768, 1024, 4096])
@pytest.mark.parametrize("rows", [1, 35, 1000])
def test_layernorm_f32_against_float64(rows, C):
    from invertible_cd_amd import ops
    g = torch.Generator().manual_seed(rows * 7 + C)
    for name, x in (("unit", torch.randn(rows, C, generator=g) * 2 + 0.3), ("mean 100, std 0.1", 100 + 0.1 * torch.randn(rows, C, generator=g))):
        if name != "unit" and (rows, C) != (35, 768):
            continue
        gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        eps = 1e-12
        o16, o32 = ops.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), eps)
        xd = x.double()
        mu = xd.mean(1, keepdim=True)
        want = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + eps) * gamma.double() + beta.double()
        e32 = rel_l2(o32.cpu(), want)
        worst = float((o32.cpu().double() - want).abs().max() / want.abs().max())
        ulps = float(((o16.cpu().double() - want).abs() / _ulp16(want)).max())
        _record(f"[layernorm_f32 {rows} x {C}, {name}] fp32 rel-L2 {e32:.3e}, max |err| / max |ref| {worst:.3e}; fp16 output within {ulps:.3f} ulp")
        assert e32 < 1e-5 and worst < 1e-5
        assert ulps <= 1.0
        only16, none32 = ops.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), eps, want32=False)
        none16, only32 = ops.layernorm_f32(x.cuda(), gamma.cuda(), beta.cuda(), eps, want16=False)
        assert none32 is None and none16 is None and torch.equal(only16, o16) and torch.equal(only32, o32)


# ------------------------------------------------------------------------------------------------ 3. preprocessing at 224
def _images(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n, h // 8, w // 8, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(base, 8, 1), 8, 2).astype(np.int64) + rng.integers(-40, 41, (n, h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _pixel_values(imgs, size):
    """ImageReward's transform on the host: Resize(size, BICUBIC) (the long edge to int(size * long / short)), CenterCrop(size), CLIP's
    mean / std -> fp32 [B, 3, size, size] and the uint8 crop"""
    from PIL import Image
    from invertible_cd_amd import resample
    out = []
    for im in imgs:
        h, w = im.shape[:2]
        rh, rw = (int(size * h / w), size) if w <= h else (size, int(size * w / h))
        r = np.asarray(Image.fromarray(im).resize((rw, rh), Image.BICUBIC))
        top, left = int(round((rh - size) / 2.0)), int(round((rw - size) / 2.0))
        out.append(r[top:top + size, left:left + size])
    u8 = torch.from_numpy(np.stack(out)).permute(0, 3, 1, 2)
    mean, std = torch.tensor(resample.CLIP_MEAN).reshape(1, 3, 1, 1), torch.tensor(resample.CLIP_STD).reshape(1, 3, 1, 1)
    return (u8.float() / 255 - mean) / std, u8


@pytest.mark.parametrize("h,w", [(96, 64), (64, 96)])
def test_preprocess_at_224_equals_pillow_resize_crop_and_normalise(h, w):
    from invertible_cd_amd import blip
    imgs = _images(2, h, w, seed=h)
    full = blip.BlipVisionModel.__new__(blip.BlipVisionModel)      # the preprocessing reads the configuration and the device only
    full.cfg, full.device = blip.IMAGEREWARD_VISION, torch.device("cuda")
    pm = full.preprocess(torch.from_numpy(imgs).cuda()).cpu()
    assert pm.dtype == torch.float16 and tuple(pm.shape) == (2 * 196, 768)
    px = pm.reshape(2, 14, 14, 3, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(2, 3, 224, 224)
    want, _ = _pixel_values(imgs, 224)
    assert torch.equal(px, want.to(torch.float16))


# ------------------------------------------------------------------------------------------------ 4. the towers, reduced
def _configs(full=False):
    from invertible_cd_amd import blip
    if full:
        return blip.IMAGEREWARD_VISION, blip.IMAGEREWARD_TEXT
    vcfg = blip.BlipVisionConfig(hidden_size=192, intermediate_size=768, num_hidden_layers=2, num_attention_heads=3, image_size=64)
    tcfg = blip.BlipTextConfig(vocab_size=200, hidden_size=128, encoder_hidden_size=192, intermediate_size=512, num_hidden_layers=2,
                               num_attention_heads=2, max_position_embeddings=40)
    return vcfg, tcfg


def _prompts(counts, T, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab, (len(counts), T), generator=g)
    mask = (torch.arange(T)[None, :] < torch.tensor(counts)[:, None]).long()
    return ids * mask, mask                                     # pad id 0 at the masked positions


@functools.lru_cache(maxsize=2)
def _setup(full=False):
    """(model, state dict, images, ids, mask, the oracle's image tokens, text states, scores) - the oracle runs once per width"""
    from invertible_cd_amd import blip
    vcfg, tcfg = _configs(full)
    sd = blip_ref.make_state_dict(vcfg, tcfg, seed=11 if full else 5)
    counts = [7, 35] if full else [4, 20, 35]
    imgs = _images(len(counts), 256 if full else 80, 320 if full else 64, seed=2)
    ids, mask = _prompts(counts, 35, tcfg.vocab_size, seed=3)
    vis, txt = blip_ref.vision_oracle(vcfg, sd), blip_ref.text_oracle(tcfg, sd)
    pv, _ = _pixel_values(imgs, vcfg.image_size)
    with torch.no_grad():
        vis_out = vis(pixel_values=pv, output_hidden_states=True)
    img_ref = vis_out.last_hidden_state
    txt_ref = blip_ref.text_forward(txt, ids, mask, img_ref)
    probs = blip_ref.first_layer_probs(txt, ids, mask)
    peaked = float((probs.max(-1).values > 0.5).float().mean())
    model = blip.ImageReward(vcfg, tcfg, sd)
    score_ref = blip_ref.head_ref(sd, txt_ref[:, 0], blip.REWARD_MEAN, blip.REWARD_STD)
    return dict(model=model, sd=sd, imgs=imgs, ids=ids, mask=mask, img_ref=img_ref, txt_ref=txt_ref, score_ref=score_ref, peaked=peaked,
                img_hidden=vis_out.hidden_states)


def test_oracle_attention_rows_are_peaked():
    s = _setup(False)
    _record(f"[blip reduced] share of first-layer self-attention rows with a maximum probability above 0.5: {s['peaked']:.2f}")
    assert s["peaked"] > 0.25


def test_reduced_towers_match_transformers():
    s = _setup(False)
    m = s["model"]
    img = m.vision_model(torch.from_numpy(s["imgs"]).cuda()).last_hidden_state
    assert img.is_cuda and img.dtype == torch.float16 and tuple(img.shape) == (3, 17, 192)
    out = m.text_encoder(s["ids"], s["mask"], img)
    txt = out.last_hidden_state
    assert txt.is_cuda and txt.dtype == torch.float16 and tuple(txt.shape) == (3, 35, 128) and out.last_hidden_state_f32.dtype == torch.float32
    e_img, e_txt = rel_l2(img.float().cpu(), s["img_ref"]), rel_l2(txt.float().cpu(), s["txt_ref"])       # every text row, padded ones too
    e_32 = rel_l2(out.last_hidden_state_f32.cpu(), s["txt_ref"])
    _record(f"[blip reduced] image tokens rel-L2 {e_img:.3e}; text last_hidden_state rel-L2 {e_txt:.3e} (fp32 copy {e_32:.3e})")
    assert e_img < 1e-3 and e_txt < 1e-3


def test_the_padding_mask_matters():
    """a padded prompt scored under its true mask against the same ids under a mask of ones: the difference must dwarf the parity error"""
    s = _setup(False)
    m = s["model"]
    dev = torch.from_numpy(s["imgs"]).cuda()
    true = m.score(s["ids"], s["mask"], dev).cpu().double()
    ones = m.score(s["ids"], torch.ones_like(s["mask"]), dev).cpu().double()
    parity = float((true - s["score_ref"]).abs().max())
    moved = (true - ones).abs()
    _record(f"[blip reduced] score parity max |score - oracle| {parity:.3e}; |true mask - all-ones mask| per sample "
            + " ".join(f"{float(v):.3e}" for v in moved))
    assert float(moved[:2].min()) > 10 * parity                 # samples 0 and 1 are padded (4 and 20 of 35 tokens)
    assert float(moved[2]) == 0.0                               # sample 2 has no padding: the same launch, the same bits


def test_calc_ir_on_the_device_is_the_models_score():
    from invertible_cd_amd import metrics
    s = _setup(False)
    dev = torch.from_numpy(s["imgs"]).cuda()
    want = s["model"].score(s["ids"], s["mask"], dev)
    assert want.is_cuda and want.dtype == torch.float32 and tuple(want.shape) == (3,)
    got = metrics.calc_ir(dev, (s["ids"], s["mask"]), "cuda", batch_size=2, model=s["model"])
    assert isinstance(got, list) and all(type(v) is float for v in got)
    two, one = s["model"].score(s["ids"][:2], s["mask"][:2], dev[:2]), s["model"].score(s["ids"][2:], s["mask"][2:], dev[2:])
    assert got == torch.cat([two, one]).cpu().tolist()
    mixed = s["model"].score(s["ids"], s["mask"], [s["imgs"][0], _images(1, 64, 96, seed=9)[0], s["imgs"][2]])
    assert torch.equal(mixed[[0, 2]], s["model"].score(s["ids"][[0, 2]], s["mask"][[0, 2]], dev[[0, 2]]))


# ------------------------------------------------------------------------------------------------ 5. full width, once
@pytest.mark.slow
def test_full_width_features_and_score_match_transformers():
    """ImageReward-v1.0's sizes (ViT-L/16 at 224: 24 x 1024, 197 tokens; BERT-base with cross-attention: 12 x 768), B = 2, counts 7 and 35.

    Measured on an MI355X (profiles/r15_blip_parity.txt): image tokens 9.41e-4, text class token 7.50e-4.  The image tower needs both
    precision options of encoder.run_blocks for it: with neither the image tokens are at 1.148e-3, with the LayerNorms on the fp32
    stream at 1.006e-3, with q and k carried as fp16 + error carry as well at 9.41e-4.  The per-layer errors are printed."""
    s = _setup(True)
    m = s["model"]
    vout = m.vision_model(torch.from_numpy(s["imgs"]).cuda(), output_hidden_states=True)
    img = vout.last_hidden_state
    _record("[blip full width] image tower rel-L2 per layer (embeddings first): "
            + " ".join(f"{rel_l2(g.float().cpu(), r):.1e}" for g, r in zip(vout.hidden_states, s["img_hidden"])))
    assert tuple(img.shape) == (2, 197, 1024)
    cls = m.text_encoder(s["ids"], s["mask"], img).last_hidden_state_f32[:, 0]
    score = (cls @ m.head_w + m.head_c).cpu().double()
    e_img, e_cls = rel_l2(img.float().cpu(), s["img_ref"]), rel_l2(cls.cpu(), s["txt_ref"][:, 0])
    bound = 1e-3 * float(m.head_w64.norm()) * s["txt_ref"][:, 0].double().norm(dim=1)
    diff = (score - s["score_ref"]).abs()
    _record(f"[blip full width] peaked first-layer rows {s['peaked']:.2f}; image tokens rel-L2 {e_img:.3e}; text class token rel-L2 {e_cls:.3e}")
    _record("[blip full width] |score - oracle| " + " ".join(f"{float(v):.3e}" for v in diff) + "; bounds "
            + " ".join(f"{float(v):.3e}" for v in bound) + "; scores " + " ".join(f"{float(v):.4f}" for v in score))
    assert torch.equal(m.score(s["ids"], s["mask"], torch.from_numpy(s["imgs"]).cuda()).cpu().double(), score)
    assert e_img < 1e-3 and e_cls < 1e-3
    assert bool((diff <= bound).all())
