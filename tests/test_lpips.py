"""Host side of LPIPS (lpips.py, synthetic.synthetic_lpips_state, loading.load_lpips, metrics.calculate_lpips / calc_inversion) and the
argument checks of its C entries: no GPU.  The oracle (tests/lpips_ref.py) is checked for the properties a distance must have."""
import ctypes
import json

import numpy as np
import pytest
import torch

import lpips_ref

REDUCED = dict(widths=(32, 32, 64, 96, 96), size=40)


def test_synthetic_state_has_torchvisions_vgg16_layout():
    from invertible_cd_amd import lpips, synthetic
    cfg = lpips.LPIPS_VGG16
    assert cfg.conv_keys() == [f"features.{i}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)]
    sd, lin = synthetic.synthetic_lpips_state(cfg, seed=1)
    assert set(sd) == {f"{k}.{p}" for k in cfg.conv_keys() for p in ("weight", "bias")}
    assert tuple(sd["features.0.weight"].shape) == (64, 3, 3, 3) and tuple(sd["features.5.weight"].shape) == (128, 64, 3, 3)
    assert tuple(sd["features.17.weight"].shape) == (512, 256, 3, 3) and tuple(sd["features.28.bias"].shape) == (512,)
    assert [tuple(w.shape) for w in lin] == [(1, c, 1, 1) for c in (64, 128, 256, 512, 512)]
    assert all(float(w.min()) >= 0 and float(w.max()) <= 1 for w in lin)
    # He statistics: std^2 = 2 / (9 Cin)
    w = sd["features.19.weight"]
    assert abs(float(w.std()) / (2 / (9 * 512)) ** 0.5 - 1) < 0.01
    sd2, lin2 = synthetic.synthetic_lpips_state(cfg, seed=1)
    assert all(torch.equal(sd[k], sd2[k]) for k in sd) and all(torch.equal(a, b) for a, b in zip(lin, lin2))
    sd3, _ = synthetic.synthetic_lpips_state(cfg, seed=2)
    assert not torch.equal(sd["features.0.weight"], sd3["features.0.weight"])


def test_model_packs_the_weights_once_and_refuses_bad_ones():
    """device='cpu': construction only.  The first conv's Cin is padded 3 -> 8 with zeros (K = 72), tap-major, channel-minor."""
    from invertible_cd_amd import lpips, synthetic
    cfg = lpips.LpipsConfig(**REDUCED)
    sd, lin = synthetic.synthetic_lpips_state(cfg, seed=3)
    m = lpips.Lpips(cfg, sd, lin, device="cpu")
    assert [len(b) for b in m.convs] == [2, 2, 3, 3, 3]
    w0, b0 = m.convs[0][0]
    assert w0.dtype == torch.float16 and tuple(w0.shape) == (32, 72) and b0.dtype == torch.float32
    w0 = w0.reshape(32, 3, 3, 8)
    assert torch.equal(w0[..., :3], sd["features.0.weight"].permute(0, 2, 3, 1).half()) and int(w0[..., 3:].count_nonzero()) == 0
    assert tuple(m.convs[4][2][0].shape) == (96, 9 * 96)
    assert all(l.dtype == torch.float32 and tuple(l.shape) == (c,) for l, c in zip(m.lin, cfg.widths))
    with pytest.raises(KeyError, match="features.28"):
        lpips.Lpips(cfg, {k: v for k, v in sd.items() if not k.startswith("features.28.")}, lin, device="cpu")
    bad = dict(sd)
    bad["features.2.weight"] = torch.zeros(32, 31, 3, 3)
    with pytest.raises(ValueError, match="features.2.weight"):
        lpips.Lpips(cfg, bad, lin, device="cpu")
    with pytest.raises(ValueError, match="lin weight"):
        lpips.Lpips(cfg, sd, lin[:4] + [torch.rand(1, 95, 1, 1)], device="cpu")
    with pytest.raises(ValueError, match="multiples of 8"):
        lpips.Lpips(lpips.LpipsConfig(widths=(32, 32, 60, 96, 96), size=40), sd, lin, device="cpu")
    with pytest.raises(ValueError, match="multiple of 4"):
        lpips.Lpips(lpips.LpipsConfig(widths=cfg.widths, size=42), sd, lin, device="cpu")


def test_load_lpips_round_trips_pt_and_safetensors_files(tmp_path):
    from safetensors.torch import save_file
    from invertible_cd_amd import loading, lpips, synthetic
    cfg = lpips.LpipsConfig(**REDUCED)
    sd, lin = synthetic.synthetic_lpips_state(cfg, seed=4)
    full = dict(sd)
    full["classifier.0.weight"] = torch.zeros(4, 4)              # a whole torchvision vgg16 carries its classifier: ignored
    torch.save(full, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lpips_weights.pt")
    save_file({k: v.contiguous() for k, v in full.items()}, str(tmp_path / "vgg16.safetensors"))
    direct = lpips.Lpips(cfg, sd, lin, device="cpu")
    for vgg in ("vgg16.pth", "vgg16.safetensors", full):
        m = loading.load_lpips(str(tmp_path / vgg) if isinstance(vgg, str) else vgg, str(tmp_path / "lpips_weights.pt"), device="cpu", config=cfg)
        assert m.cfg == cfg
        for blk, ref in zip(m.convs, direct.convs):
            assert all(torch.equal(w, rw) and torch.equal(b, rb) for (w, b), (rw, rb) in zip(blk, ref))
        assert all(torch.equal(a, b) for a, b in zip(m.lin, direct.lin))
    m = loading.load_lpips(sd, lin, device="cpu", config=cfg)
    assert all(torch.equal(a, b) for a, b in zip(m.lin, direct.lin))
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        loading.load_lpips(str(tmp_path / "nowhere.pth"), lin, device="cpu", config=cfg)
    with pytest.raises(KeyError, match="lacks"):                 # without a config the full-width defaults do not fit these weights
        loading.load_lpips({k: v for k, v in sd.items() if k != "features.0.bias"}, lin, device="cpu")


def test_the_oracle_is_a_distance():
    """exactly 0 for identical inputs, symmetric, positive otherwise - in fp32 and in the fp16-storage emulation"""
    from invertible_cd_amd import lpips, synthetic
    cfg = lpips.LpipsConfig(**REDUCED)
    sd, lin = synthetic.synthetic_lpips_state(cfg, seed=5)
    sd = lpips_ref.rounded(sd)
    a, b = lpips_ref.six_pairs(64, 64, seed=1)
    for emulate in (False, True):
        d = lpips_ref.lpips(cfg, sd, lin, a, b, emulate)
        assert d.dtype == torch.float32 and tuple(d.shape) == (6,)
        assert torch.equal(lpips_ref.lpips(cfg, sd, lin, a, a, emulate), torch.zeros(6))
        assert float(d[4]) == 0.0 and bool((d[[0, 1, 2, 3, 5]] > 0).all())
        assert torch.equal(lpips_ref.lpips(cfg, sd, lin, b, a, emulate), d)
        assert float(d[5]) < float(d[:4].min())                  # the 90 / 10 blend is closer than an unrelated image
    sizes = [tuple(t.shape[1:]) for t in lpips_ref.taps(cfg, sd, a)]
    assert sizes == [(32, 40, 40), (32, 20, 20), (64, 10, 10), (96, 5, 5), (96, 2, 2)]


def test_the_ingest_geometry_is_pillows_default_resize():
    """PIL.Image.resize without a filter is BICUBIC, stretches both axes and does not crop: resample.resize_emulated with the tables the
    device kernel reads equals it byte for byte (the kernel itself is compared on the GPU)."""
    from invertible_cd_amd import resample
    rng = np.random.default_rng(0)
    for h, w, s in [(64, 64, 40), (57, 91, 40), (100, 150, 224), (224, 300, 224), (224, 224, 224)]:
        img = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
        assert np.array_equal(resample.resize_emulated(img[0], s, s), lpips_ref.resize(img, s)[0]), (h, w, s)
    f, c, k = resample.resample_tables(224, 224)                 # an axis that keeps its size: exact [0, 1, 0] taps
    assert all(int(k[i, :c[i]].sum()) == 1 << 22 and int(np.count_nonzero(k[i])) == 1 for i in range(224))


def test_calculate_lpips_refuses_a_missing_model_and_batches_through_it():
    from invertible_cd_amd import metrics
    imgs = np.zeros((5, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="model="):
        metrics.calculate_lpips(imgs, imgs, "cuda")
    with pytest.raises(ValueError, match="model="):
        metrics.calculate_lpips(imgs, imgs, "cuda", model=None)
    calls = []

    def stub(a, b):
        calls.append((len(a), len(b)))
        return torch.arange(len(a), dtype=torch.float32) + 10 * len(calls)
    got = metrics.calculate_lpips(imgs, list(imgs), "cpu", batch_size=2, model=stub)
    assert calls == [(2, 2), (2, 2), (1, 1)]
    assert not got.is_cuda and got.dtype == torch.float32 and got.tolist() == [10, 11, 20, 21, 30]


def test_calc_inversion_writes_the_references_report(tmp_path, monkeypatch):
    """Stub models on four tiny PNGs: the directory layout, the sorted pairing, batch_size 16, the three keys and their string format."""
    from PIL import Image
    from invertible_cd_amd import metrics
    rng = np.random.default_rng(1)
    (tmp_path / "generated_images").mkdir()
    (tmp_path / "real_images").mkdir()
    pix = {}
    for d, names in (("generated_images", ["b.png", "a.png"]), ("real_images", ["y.png", "x.png"])):
        for n in names:
            pix[n] = rng.integers(0, 256, (12, 12, 3), dtype=np.uint8)
            Image.fromarray(pix[n]).save(tmp_path / d / n)
    seen = {}

    class Dino:
        def get_image_features(self, images):
            assert all(im.size == (512, 512) for im in images)   # load_512 + to_pil_images
            e = torch.stack([torch.from_numpy(np.asarray(im)).float().mean((0, 1)) for im in images])
            seen.setdefault("dino", []).append(e)
            return e

    def lp(a, b):
        seen["lpips"] = (a, b)
        return torch.tensor([0.25, 0.5])
    with pytest.raises(ValueError, match="dinov2_model="):
        metrics.calc_inversion(str(tmp_path), "cpu", lpips_model=lp)
    with pytest.raises(ValueError, match="lpips_model="):
        metrics.calc_inversion(str(tmp_path), "cpu", dinov2_model=Dino())
    from invertible_cd_amd import ops
    monkeypatch.setattr(ops, "cosine_rows", lambda a, b: torch.nn.functional.cosine_similarity(a, b))      # the kernel's stand-in without a GPU
    res = metrics.calc_inversion(str(tmp_path), "cpu", dinov2_model=Dino(), lpips_model=lp)
    with open(tmp_path / "preservation_metrics_values.json") as f:
        assert json.load(f) == res
    assert list(res) == ["preservation_dinov2", "preservation_psnr", "preservation_lpips"]
    assert all(isinstance(v, str) and v.startswith("[") and v.endswith("]") for v in res.values())
    assert res["preservation_lpips"] == str(list(np.array(torch.tensor([0.25, 0.5]))))
    # sorted pairing: a.png with x.png, b.png with y.png - whatever order the file system lists them in
    a, b = seen["lpips"]
    assert len(a) == len(b) == 2
    up = lambda n: np.array(Image.fromarray(pix[n]).resize((512, 512)))
    assert np.array_equal(np.asarray(a[0]), up("a.png")) and np.array_equal(np.asarray(b[0]), up("x.png"))
    assert np.array_equal(np.asarray(a[1]), up("b.png")) and np.array_equal(np.asarray(b[1]), up("y.png"))
    want = []
    for x, y in (("a.png", "x.png"), ("b.png", "y.png")):
        mse = np.mean((up(x).astype(np.float64) - up(y).astype(np.float64)) ** 2)
        want.append(20 * np.log10(255.0 / np.sqrt(mse)))
    got = [float(t.split("(")[-1].rstrip(")")) for t in res["preservation_psnr"][1:-1].split(", ")]
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert len(res["preservation_dinov2"][1:-1].split(", ")) == 2


def test_the_new_entries_refuse_bad_arguments_without_a_gpu():
    """Every check runs before any HIP call: host pointers (never dereferenced) are enough."""
    from invertible_cd_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    P = lambda off=0: ctypes.c_void_p(base + off)
    INVALID = -1

    def refused(status, word):
        assert status == INVALID, word
        assert word.encode() in lib.icd_last_error(), (word, lib.icd_last_error())
    # icd_relu
    refused(lib.icd_relu(None, 8, P(), None), "null")
    refused(lib.icd_relu(P(), 8, None, None), "null")
    refused(lib.icd_relu(P(), 12, P(), None), "multiple of 8")
    refused(lib.icd_relu(P(), 0, P(), None), "positive")
    refused(lib.icd_relu(P(2), 8, P(), None), "aligned")
    # icd_maxpool2x2
    refused(lib.icd_maxpool2x2(None, 1, 4, 4, 8, 0, P(1024), None), "null")
    refused(lib.icd_maxpool2x2(P(), 0, 4, 4, 8, 0, P(1024), None), "positive")
    refused(lib.icd_maxpool2x2(P(), 1, 1, 4, 8, 0, P(1024), None), "at least 2")
    refused(lib.icd_maxpool2x2(P(), 1, 4, 4, 12, 0, P(1024), None), "multiple of 8")
    refused(lib.icd_maxpool2x2(P(), 1, 4, 4, 8, 2, P(1024), None), "relu")
    refused(lib.icd_maxpool2x2(P(), 1, 4, 4, 8, 0, P(1028), None), "aligned")
    refused(lib.icd_maxpool2x2(P(), 1, 4, 4, 8, 0, P(), None), "in-place")
    # icd_lpips_layer
    need = lib.icd_lpips_layer_workspace_bytes(2, 25, 24)
    assert need == 2 * 4                                         # 25 pixels of 4 lanes: one block per sample
    assert lib.icd_lpips_layer_workspace_bytes(100, 224 * 224, 64) == 100 * 196 * 4
    assert lib.icd_lpips_layer_workspace_bytes(0, 25, 24) == 0

    def layer(f=P(), ldf=24, B=2, HW=25, C=24, w=P(2048), relu=1, acc=0, ws=P(3072), ws_bytes=need, out=P(3584)):
        return lib.icd_lpips_layer(f, ldf, B, HW, C, w, relu, acc, ws, ws_bytes, out, None)
    for kwargs, word in [(dict(f=None), "null"), (dict(w=None), "null"), (dict(ws=None), "null"), (dict(out=None), "null"),
                         (dict(B=0), "positive"), (dict(HW=0), "positive"), (dict(C=20, ldf=24), "multiple of 8"), (dict(C=0), "multiple of 8"),
                         (dict(ldf=16), "ldf"), (dict(ldf=28), "ldf"), (dict(relu=2), "relu"), (dict(acc=-1), "accumulate"),
                         (dict(f=P(8)), "aligned"), (dict(w=P(2052)), "aligned"), (dict(ws_bytes=need - 1), "too small")]:
        refused(layer(**kwargs), word)
    # icd_image_resize_norm
    from invertible_cd_amd import resample
    mean, std = (ctypes.c_float * 3)(*resample.IMAGENET_MEAN), (ctypes.c_float * 3)(*resample.IMAGENET_STD)

    def ingest(img=P(1), B=1, H=6, W=6, S=4, tab=P(1024), ht=resample.tap_width(6, 4), vt=resample.tap_width(6, 4), mean=mean, std=std,
               tmp=P(2048), out=P(3072)):
        return lib.icd_image_resize_norm(img, B, H, W, S, tab, tab, tab, ht, tab, tab, tab, vt, mean, std, tmp, out, None)
    zero_std = (ctypes.c_float * 3)(0.2, 0.0, 0.2)
    for kwargs, word in [(dict(img=None), "null"), (dict(tmp=None), "null"), (dict(out=None), "null"), (dict(tab=None), "null"),
                         (dict(B=0), "positive"), (dict(H=0), "positive"), (dict(S=6), "multiple of 4"), (dict(S=0), "multiple of 4"),
                         (dict(W=5000, ht=resample.tap_width(5000, 4)), "exceeds"), (dict(ht=5), "tables do not match"),
                         (dict(tmp=P(2049)), "aligned"), (dict(out=P(3080)), "aligned"), (dict(std=zero_std), "std must be positive")]:
        refused(ingest(**kwargs), word)
