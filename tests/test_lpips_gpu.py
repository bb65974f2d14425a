"""LPIPS on the device against its oracles (tests/lpips_ref.py: plain torch on the CPU, and its fp16-storage emulation).

Bars.  Ingest, ReLU, max-pool: exact equality (integer arithmetic, one rounding, comparisons).  icd_lpips_layer against the fp32 torch
expression on the same fp16 inputs: 1e-5 relative per sample - the order of an fp32 sum of at most 1600 * 520 terms of one sign, not a
rounding of the data.  Taps: rel-L2 < 1e-3 against the fp32 oracle, the project's bar for every encoder.  Scores, per sample:
|got - want| <= 4 * max_batch |emulation - want| + 1e-6; the emulation makes the device path's roundings in another summation order, so
both errors are draws of one size, the batch maximum stands in for a sample whose own floor is tiny by accident, and 4 covers the spread
(a layout or indexing bug moves scores by percent).  profiles/r10_lpips_parity.txt keeps one run's printout."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2
import lpips_ref

pytestmark = pytest.mark.gpu

REDUCED = dict(widths=(32, 32, 64, 96, 96), size=40)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------------ 1. ingest
@pytest.mark.parametrize("H,W,S,odd", [(64, 64, 40, False), (57, 91, 40, True), (100, 150, 224, False), (224, 300, 224, False),
                                       (512, 512, 224, False)])
def test_ingest_equals_pillows_resize_and_the_fp32_normalisation_bit_for_bit(H, W, S, odd):
    """Down- and upscaling, an identity axis (224 of 224 x 300), odd sizes; `odd`: the batch is a slice that starts at an odd byte."""
    from invertible_cd_amd import ops
    B = 3
    rng = np.random.default_rng(H * 1000 + W)
    imgs = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    if odd:
        flat = torch.zeros(1 + imgs.size, dtype=torch.uint8, device="cuda")
        flat[1:] = torch.from_numpy(imgs).cuda().flatten()
        dev = flat[1:].view(B, H, W, 3)
        assert dev.data_ptr() % 2 == 1
    else:
        dev = torch.from_numpy(imgs).cuda()
    out = ops.image_resize_norm(dev, S, MEAN, STD)
    assert out.is_cuda and out.dtype == torch.float16 and tuple(out.shape) == (B * S * S, 8)
    out = out.cpu().reshape(B, S, S, 8)
    assert int(out[..., 3:].count_nonzero()) == 0
    mean, std = torch.tensor(MEAN), torch.tensor(STD)
    ref = torch.from_numpy(lpips_ref.resize(imgs, S))
    got_u = torch.round((out[..., :3].float() * std + mean) * 255)
    assert torch.equal(got_u, ref.float()), f"{int((got_u != ref.float()).sum())} resized bytes differ from PIL"
    want = ((ref.float() / 255 - mean) / std).half()                         # fp32 arithmetic, one rounding to fp16
    assert torch.equal(out[..., :3], want)


# ------------------------------------------------------------------------------------------------ 2. ReLU, max-pool
@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 8), (1, 40, 40, 24), (2, 14, 14, 512)])
def test_relu_and_maxpool_are_torchs_bit_for_bit(B, H, W, C):
    """Odd H / W: floor mode drops the last row / column.  Half of the values are negative."""
    from invertible_cd_amd import ops
    g = torch.Generator().manual_seed(B * 100 + C)
    x = torch.randn(B, H, W, C, generator=g).half()
    assert bool((x < 0).any())
    dev = x.cuda().reshape(B * H * W, C)
    assert torch.equal(ops.relu(dev).cpu().reshape(x.shape), torch.relu(x.float()).half())
    assert torch.equal(dev.cpu().reshape(x.shape), x)                        # out of place: the input is untouched
    inplace = dev.clone()
    assert ops.relu(inplace, inplace=True) is inplace and torch.equal(inplace.cpu().reshape(x.shape), torch.relu(x.float()).half())
    pooled = torch.nn.functional.max_pool2d(x.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).half()
    assert tuple(pooled.shape) == (B, H // 2, W // 2, C)
    for relu in (False, True):
        got = ops.maxpool2x2(dev, B, H, W, relu=relu)
        assert tuple(got.shape) == (B * (H // 2) * (W // 2), C)
        want = torch.relu(pooled) if relu else pooled
        assert torch.equal(got.cpu().reshape(want.shape), want), relu
    assert bool((pooled < 0).any())                                          # ... so the flag was visible


# ------------------------------------------------------------------------------------------------ 3. the distance head
def _head_ref(f, B, HW, C, w, relu):
    """the fp32 torch expression on the same fp16 inputs"""
    x = f[:, :C].float()
    if relu:
        x = torch.relu(x)
    a, b = x[:B * HW].reshape(B, HW, C), x[B * HW:].reshape(B, HW, C)
    n1 = a / (torch.sqrt((a ** 2).sum(-1, keepdim=True)) + 1e-10)
    n2 = b / (torch.sqrt((b ** 2).sum(-1, keepdim=True)) + 1e-10)
    return ((n1 - n2) ** 2 * w).sum(-1).mean(-1)


@pytest.mark.parametrize("B,HW,C,ldf", [(2, 1, 8, 8), (3, 25, 24, 24), (2, 1600, 64, 64), (1, 196, 136, 144), (2, 49, 512, 512),
                                        (1, 9, 520, 520)])
def test_lpips_layer_matches_the_fp32_expression(B, HW, C, ldf):
    """One lane per pixel (C = 8), idle lanes in a group (24: 3 of 4, 136: 17 of 32), several blocks per sample (1600 pixels), a whole
    wave per pixel (512) and its loop (520); ldf > C with NaN in the pad columns."""
    from invertible_cd_amd import ops
    g = torch.Generator().manual_seed(HW * 1000 + C)
    f = torch.randn(2 * B * HW, ldf, generator=g).half()
    f[:, C:] = float("nan")
    w = torch.rand(C, generator=g)
    dev, wd = f.cuda(), w.cuda()
    for relu in (False, True):
        want = _head_ref(f, B, HW, C, w, relu)
        got = ops.lpips_layer(dev[:, :C], B, HW, wd, relu=relu)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (B,)
        rel = ((got.cpu() - want).abs() / want).max()
        print(f"[lpips_layer B {B} HW {HW} C {C} relu {int(relu)}] max relative difference {float(rel):.2e}")
        assert float(rel) <= 1e-5
        again = ops.lpips_layer(dev[:, :C], B, HW, wd, relu=relu)
        assert torch.equal(again, got)                                       # two calls: equal bits
        acc = got.clone()
        ops.lpips_layer(dev[:, :C], B, HW, wd, out=acc, relu=relu, accumulate=True)
        assert torch.equal(acc, got + got)                                   # accumulate adds
    # identical halves: exactly zero; and a sample's value does not depend on its place in the batch
    same = torch.cat([dev[:B * HW], dev[:B * HW]])
    assert torch.equal(ops.lpips_layer(same[:, :C], B, HW, wd, relu=True).cpu(), torch.zeros(B))
    if B > 1:
        last = torch.cat([dev[(B - 1) * HW:B * HW], dev[(2 * B - 1) * HW:]])
        assert torch.equal(ops.lpips_layer(last[:, :C], 1, HW, wd)[0], ops.lpips_layer(dev[:, :C], B, HW, wd)[B - 1])


def test_lpips_layer_refuses_bad_arguments_before_any_launch():
    from invertible_cd_amd import _lib
    lib = _lib.load()
    INVALID = -1
    B, HW, C = 2, 25, 24
    f = torch.ones(2 * B * HW, C, device="cuda", dtype=torch.float16)
    f[B * HW:] = 0
    w = torch.ones(C, device="cuda")
    need = lib.icd_lpips_layer_workspace_bytes(B, HW, C)
    ws = torch.zeros(need // 4, device="cuda")
    out = torch.zeros(B, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(f=p(f), ldf=C, B=B, HW=HW, C=C, w=p(w), relu=0, acc=0, ws=p(ws), ws_bytes=need, out=p(out)):
        return lib.icd_lpips_layer(f, ldf, B, HW, C, w, relu, acc, ws, ws_bytes, out, None)
    for kwargs, word in [(dict(f=None), "null"), (dict(w=None), "null"), (dict(ws=None), "null"), (dict(out=None), "null"),
                         (dict(B=0), "positive"), (dict(B=-1), "positive"), (dict(HW=0), "positive"), (dict(C=20), "multiple of 8"),
                         (dict(C=0), "multiple of 8"), (dict(ldf=16), "ldf"), (dict(ldf=28), "ldf"), (dict(relu=3), "relu"),
                         (dict(acc=2), "accumulate"), (dict(f=ctypes.c_void_p(f.data_ptr() + 2)), "aligned"),
                         (dict(w=ctypes.c_void_p(w.data_ptr() + 4)), "aligned"), (dict(ws_bytes=need - 4), "too small")]:
        assert call(**kwargs) == INVALID, kwargs
        assert word.encode() in lib.icd_last_error(), (kwargs, lib.icd_last_error())
    torch.cuda.synchronize()
    assert int(out.count_nonzero()) == 0 and int(ws.count_nonzero()) == 0    # nothing was launched on the outputs
    assert call() == 0
    torch.cuda.synchronize()
    # a = ones: a / |a| = 1 / sqrt(24) per channel, b = 0 -> 0; sum_c w (a_c / |a|)^2 = 1
    assert torch.allclose(out.cpu(), torch.ones(B), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------ 4. / 5. the model
@functools.lru_cache(maxsize=None)
def _case(full, seed):
    """(cfg, state dict, lin, images_1, images_2, fp32 taps of both, fp32 scores, emulated scores): the CPU side, computed once"""
    from invertible_cd_amd import lpips, synthetic
    cfg = lpips.LPIPS_VGG16 if full else lpips.LpipsConfig(**REDUCED)
    sd, lin = synthetic.synthetic_lpips_state(cfg, seed=seed)
    sd = lpips_ref.rounded(sd)
    a, b = lpips_ref.six_pairs(512, 512, seed) if full else lpips_ref.six_pairs(64, 64, seed)
    t1, t2 = lpips_ref.taps(cfg, sd, a), lpips_ref.taps(cfg, sd, b)
    want = lpips_ref.distance(t1, t2, lin)
    emu = lpips_ref.lpips(cfg, sd, lin, a, b, emulate=True)
    return cfg, sd, lin, a, b, t1, t2, want, emu


def _check_model(name, full, seed):
    from invertible_cd_amd import lpips
    cfg, sd, lin, a, b, t1, t2, want, emu = _case(full, seed)
    m = lpips.Lpips(cfg, sd, lin)
    s = cfg.size
    taps = m.features(torch.from_numpy(np.concatenate([a, b])).cuda())
    assert len(taps) == 5
    errs = []
    for level, (got, r1, r2) in enumerate(zip(taps, t1, t2)):
        ref = torch.cat([r1, r2]).permute(0, 2, 3, 1)
        assert got.is_cuda and got.dtype == torch.float16 and tuple(got.shape) == tuple(ref.shape) == (12, s >> level, s >> level, cfg.widths[level])
        assert float(got.min()) >= 0
        errs.append(rel_l2(got.float().cpu(), ref))
    print(f"[{name}] tap rel-L2 vs the fp32 oracle: " + " ".join(f"{e:.2e}" for e in errs) + f"; max activation {max(float(t.max()) for t in t1):.1f}")
    got = m(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (6,)
    got = got.cpu()
    floor = float((emu - want).abs().max())
    print(f"[{name}] scores        " + " ".join(f"{float(v):.6f}" for v in got))
    print(f"[{name}] oracle        " + " ".join(f"{float(v):.6f}" for v in want))
    print(f"[{name}] |got - want|  " + " ".join(f"{float(v):.2e}" for v in (got - want).abs()))
    print(f"[{name}] |emu - want|  " + " ".join(f"{float(v):.2e}" for v in (emu - want).abs()) + f"  (batch maximum {floor:.2e}, "
          f"{float(((emu - want).abs() / want.clamp_min(1e-30))[[0, 1, 2, 3, 5]].max()):.1e} relative)")
    assert all(e < 1e-3 for e in errs), errs
    assert bool(((got - want).abs() <= 4 * floor + 1e-6).all())
    assert float(got[4]) == 0.0 and float(want[4]) == 0.0                    # the identical pair
    assert bool((got[[0, 1, 2, 3, 5]] > 0).all()) and float(got[5]) < float(got[:4].min())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reduced_model_matches_the_oracle(seed):
    """widths 32, 32, 64, 96, 96 at size 40: spatial sizes 40, 20, 10, 5, 2 (an odd size into a floor-mode pool)"""
    _check_model(f"lpips reduced, seed {seed}", False, seed)


def test_full_width_model_matches_the_oracle():
    """VGG16's own widths at 224 x 224 on 512 x 512 images"""
    _check_model("lpips vgg16 224", True, 4)


# ------------------------------------------------------------------------------------------------ 6. metrics.calculate_lpips
@functools.lru_cache(maxsize=1)
def _scorer():
    from invertible_cd_amd import lpips
    cfg, sd, lin = _case(False, 1)[:3]
    return lpips.Lpips(cfg, sd, lin)


def test_calculate_lpips_routes(monkeypatch):
    from PIL import Image
    from invertible_cd_amd import metrics
    model = _scorer()
    cfg, sd, lin = _case(False, 1)[:3]
    N = 5
    a, b = lpips_ref.structured_images(N, 64, 64, seed=20), lpips_ref.structured_images(N, 64, 64, seed=21)
    b[0] = a[0]
    want = lpips_ref.lpips(cfg, sd, lin, a, b)
    floor = float((lpips_ref.lpips(cfg, sd, lin, a, b, emulate=True) - want).abs().max())
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    crossed = []                                                             # the device-tensor route: only the scores cross to the host
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
        got = metrics.calculate_lpips(da, db, "cuda", batch_size=2, model=model)
    assert crossed == [2, 2, 1], crossed                                     # three batches of scores; no image among them
    assert not got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (N,)
    print("[calculate_lpips] scores " + " ".join(f"{float(s):.6f}" for s in got) + f"; max |score - oracle| {float((got - want).abs().max()):.2e}")
    assert bool(((got - want).abs() <= 4 * floor + 1e-6).all()) and float(got[0]) == 0.0
    # host arrays, PIL images and a stacked array take the same route after an upload; the batch size changes nothing
    host = metrics.calculate_lpips(list(a), list(b), "cuda", batch_size=50, model=model)
    pil = metrics.calculate_lpips([Image.fromarray(x) for x in a], [Image.fromarray(x) for x in b], "cuda", model=model)
    stacked = metrics.calculate_lpips(a, b, "cuda", batch_size=3, model=model)
    whole = metrics.calculate_lpips(da, db, "cuda", batch_size=50, model=model)
    assert torch.equal(host, got) and torch.equal(pil, got) and torch.equal(stacked, got) and torch.equal(whole, got)


def test_calculate_lpips_of_a_list_of_mixed_sizes_keeps_the_callers_order():
    from invertible_cd_amd import metrics
    model = _scorer()
    a, b = lpips_ref.structured_images(3, 64, 96, seed=3)[:, :-7, :-5], lpips_ref.structured_images(3, 64, 96, seed=4)[:, :-7, :-5]      # 57 x 91
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    c, d = lpips_ref.structured_images(2, 64, 64, seed=5), lpips_ref.structured_images(2, 64, 64, seed=6)
    odd = metrics.calculate_lpips(list(a), list(b), "cuda", model=model)
    small = metrics.calculate_lpips(list(c), list(d), "cuda", model=model)
    la, lb = [a[0], c[0], a[1], c[1], a[2]], [b[0], d[0], b[1], d[1], b[2]]
    mixed = metrics.calculate_lpips(la, lb, "cuda", model=model)
    assert torch.isfinite(mixed).all() and len(set(mixed.tolist())) == 5
    assert torch.equal(mixed[0::2], odd) and torch.equal(mixed[1::2], small)


# ------------------------------------------------------------------------------------------------ 7. the loader
def test_load_lpips_from_disk_gives_the_scores_of_the_state_dict(tmp_path):
    from safetensors.torch import save_file
    from invertible_cd_amd import loading
    cfg, sd, lin, a, b = _case(False, 1)[:5]
    torch.save(sd, tmp_path / "vgg16.pth")
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "vgg16.safetensors"))
    torch.save(lin, tmp_path / "lpips_weights.pt")
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    want = _scorer()(da, db)
    for name in ("vgg16.pth", "vgg16.safetensors"):
        m = loading.load_lpips(str(tmp_path / name), str(tmp_path / "lpips_weights.pt"), config=cfg)
        got = m(da, db)
        assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got, want)
