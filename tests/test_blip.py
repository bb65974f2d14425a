"""ImageReward without a GPU: the folded head against the unfolded one, the ImageReward package's key names against the oracle's, the
host-side refusals of the text tower, the argument checks of the two new kernels through the C ABI, and calc_ir / calc_all /
load_benchmark on stub models."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import blip_ref

GOLDEN_CSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "editing_benchmark_3rows.csv")


def _reduced():
    from invertible_cd_amd import blip
    vcfg = blip.BlipVisionConfig(hidden_size=192, intermediate_size=768, num_hidden_layers=2, num_attention_heads=3, image_size=64)
    tcfg = blip.BlipTextConfig(vocab_size=200, hidden_size=128, encoder_hidden_size=192, intermediate_size=512, num_hidden_layers=2,
                               num_attention_heads=2, max_position_embeddings=40)
    return vcfg, tcfg


# ------------------------------------------------------------------------------------------------ the head
def test_folded_head_is_the_five_linears_and_the_normalisation():
    from invertible_cd_amd import blip
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(shp, generator=g) * (shp[-1] ** -0.5 if k.endswith("weight") else 0.3) for k, shp in blip.head_shapes(768).items()}
    w, c = blip.fold_head(sd)
    assert w.dtype == torch.float64 and tuple(w.shape) == (768,) and isinstance(c, float)
    x = torch.randn(64, 768, generator=g)
    want = blip_ref.head_ref(sd, x, blip.REWARD_MEAN, blip.REWARD_STD)
    got = x.double() @ w + c
    assert float((got - want).abs().max() / want.abs().max()) < 1e-12
    assert blip.REWARD_MEAN == 0.16717362830052426 and blip.REWARD_STD == 1.0333394966054072


# ------------------------------------------------------------------------------------------------ key names
def test_package_key_names_load_to_the_same_prepared_tensors():
    from invertible_cd_amd import blip, loading
    vcfg, tcfg = _reduced()
    sd = blip_ref.make_state_dict(vcfg, tcfg, seed=3)
    pkg = blip_ref.to_package_names(sd)
    assert all(k.startswith(("blip.visual_encoder.", "blip.text_encoder.", "mlp.layers.")) for k in pkg)
    assert "blip.visual_encoder.blocks.1.attn.qkv.weight" in pkg and "blip.visual_encoder.pos_embed" in pkg
    a = loading.load_imagereward(sd, "cpu", config=(vcfg, tcfg))
    b = loading.load_imagereward(pkg, "cpu", config=(vcfg, tcfg))
    for ma, mb in ((a.vision_model, b.vision_model), (a.text_encoder, b.text_encoder)):
        assert sorted(ma.w) == sorted(mb.w) and len(ma.w) > 20
        for k in ma.w:
            assert ma.w[k].dtype == mb.w[k].dtype and torch.equal(ma.w[k], mb.w[k]), k
    assert torch.equal(a.head_w64, b.head_w64) and a.head_c64 == b.head_c64
    with pytest.raises(KeyError, match="lacks"):
        loading.load_imagereward({k: v for k, v in pkg.items() if not k.endswith("blocks.0.attn.proj.bias")}, "cpu", config=(vcfg, tcfg))


# ------------------------------------------------------------------------------------------------ host validation
def test_text_tower_refuses_bad_masks_and_lengths_on_the_host():
    from invertible_cd_amd import blip
    vcfg, tcfg = _reduced()
    sd = blip_ref.make_state_dict(vcfg, tcfg, seed=1)
    m = blip.ImageReward(vcfg, tcfg, sd, device="cpu").text_encoder
    enc = torch.zeros(2, 17, 192, dtype=torch.float16)
    ids = torch.ones(2, 6, dtype=torch.long)
    with pytest.raises(ValueError, match="right-padded"):
        m(ids, torch.tensor([[1, 1, 0, 1, 0, 0], [1, 1, 1, 1, 1, 1]]), enc)
    with pytest.raises(ValueError, match="right-padded"):
        m(ids, torch.tensor([[0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]]), enc)
    with pytest.raises(ValueError, match="all-zero row"):
        m(ids, torch.tensor([[1, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0]]), enc)
    with pytest.raises(ValueError, match="position table"):
        m(torch.ones(2, 41, dtype=torch.long), torch.ones(2, 41, dtype=torch.long), enc)
    with pytest.raises(ValueError, match="zeros and ones"):
        m(ids, torch.full((2, 6), 2), enc)
    assert blip.key_counts_of(torch.tensor([[1, 1, 1, 0], [1, 0, 0, 0], [1, 1, 1, 1]])).tolist() == [3, 1, 4]


# ------------------------------------------------------------------------------------------------ C ABI argument checks
def test_new_kernels_refuse_bad_arguments_without_a_gpu():
    from invertible_cd_amd import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED = -1, -2
    buf = (ctypes.c_char * 4096)()                              # host memory, 16-byte aligned below; never dereferenced
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)

    def attn(q=p, k=p, vt=p, out=p, counts=p, B=2, H=2, Nq=35, Nk=35, d=64, ldq=128, ldk=128, ldvt=40, ldo=128, vt_bs=0, scale=0.125):
        return lib.icd_attention_masked(q, k, vt, out, counts, B, H, Nq, Nk, d, ldq, ldk, ldvt, ldo, vt_bs, scale, None)
    for kwargs, status, word in [(dict(Nk=129, ldvt=136), UNSUPPORTED, "128 keys"), (dict(d=136, ldq=272, ldk=272, ldo=272), UNSUPPORTED, "head dim"),
                                 (dict(d=36, ldq=72, ldk=72, ldo=72), UNSUPPORTED, "head dim"), (dict(counts=None), INVALID, "key_counts"),
                                 (dict(q=None), INVALID, "null"), (dict(ldvt=32), INVALID, "ldvt"), (dict(ldq=120), INVALID, "H * d"),
                                 (dict(Nq=0), INVALID, "empty"), (dict(scale=0.0), INVALID, "scale")]:
        assert attn(**kwargs) == status, kwargs
        assert word.encode() in lib.icd_last_error(), (kwargs, lib.icd_last_error())

    def ln(x=p, rows=4, C=768, gamma=p, beta=p, eps=1e-12, o16=p, o32=p):
        return lib.icd_layernorm_f32(x, rows, C, gamma, beta, eps, o16, o32, None)
    for kwargs, status, word in [(dict(C=4104), UNSUPPORTED, "multiple of 8"), (dict(C=12), UNSUPPORTED, "multiple of 8"),
                                 (dict(C=0), UNSUPPORTED, "multiple of 8"), (dict(x=None), INVALID, "null"),
                                 (dict(o16=None, o32=None), INVALID, "both outputs"), (dict(rows=0), INVALID, "rows"),
                                 (dict(x=ctypes.c_void_p(p.value + 4)), INVALID, "aligned")]:
        assert ln(**kwargs) == status, kwargs
        assert word.encode() in lib.icd_last_error(), (kwargs, lib.icd_last_error())


# ------------------------------------------------------------------------------------------------ calc_ir / calc_all on stubs
class StubReward:
    """score = sum of the unmasked ids + the mean of the image bytes / 1000: a known function of both inputs"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    @staticmethod
    def expected(ids, mask, images):
        px = torch.tensor([float(np.asarray(im, dtype=np.float64).mean()) for im in images])
        return ((ids * mask).sum(1).double() + px.double() / 1000).float()

    def score(self, ids, mask, images):
        self.calls.append(len(images))
        assert ids.shape[0] == mask.shape[0] == len(images)
        return self.expected(ids, mask, images)


class Encoding(dict):
    input_ids = property(lambda self: self["input_ids"])


class StubTokenizer:
    def __init__(self):
        self.kwargs = None

    def __call__(self, prompts, **kw):
        self.kwargs = kw
        n = kw.get("max_length", 8)
        ids = torch.zeros(len(prompts), n, dtype=torch.long)
        mask = torch.zeros(len(prompts), n, dtype=torch.long)
        for i, p in enumerate(prompts):
            k = min(len(p.split()), n)
            ids[i, :k] = torch.tensor([len(wd) for wd in p.split()[:k]])
            mask[i, :k] = 1
        return Encoding(input_ids=ids, attention_mask=mask)


def test_calc_ir_batches_the_pairs_and_returns_python_floats_in_order():
    from invertible_cd_amd import metrics
    rng = np.random.default_rng(0)
    N = 7
    images = [rng.integers(0, 256, (8, 8, 3), dtype=np.uint8) for _ in range(N)]
    ids = torch.from_numpy(rng.integers(1, 50, (N, 5)))
    mask = torch.tensor([[1] * k + [0] * (5 - k) for k in (5, 1, 3, 2, 4, 5, 1)])
    stub = StubReward()
    got = metrics.calc_ir(images, (ids, mask), "cpu", batch_size=3, model=stub)
    assert stub.calls == [3, 3, 1]
    assert isinstance(got, list) and len(got) == N and all(type(g) is float for g in got)
    assert got == [float(v) for v in StubReward.expected(ids, mask, images)]
    # strings go through the tokenizer, called as the ImageReward package calls it
    tok = StubTokenizer()
    prompts = ["a b c", "dd", "e ff ggg hhhh", "i", "j k", "l", "m n o p q"]
    got = metrics.calc_ir(images, prompts, "cpu", batch_size=50, model=stub, tokenizer=tok)
    assert tok.kwargs == dict(padding="max_length", truncation=True, max_length=35, return_tensors="pt")
    enc = tok(prompts, max_length=35)
    assert got == [float(v) for v in StubReward.expected(enc["input_ids"], enc["attention_mask"], images)]
    with pytest.raises(ValueError, match="model="):
        metrics.calc_ir(images, (ids, mask), "cpu")
    with pytest.raises(ValueError, match="tokenizer="):
        metrics.calc_ir(images, prompts, "cpu", model=stub)


def test_load_benchmark_reads_the_csv_as_the_reference_does(tmp_path):
    from invertible_cd_amd import loading
    bench = loading.load_benchmark(GOLDEN_CSV, "/imgs")
    assert bench == [("/imgs/0.png", {"before": "a photo of a cat", "after": "a photo of a dog"}, "cat dog"),
                     ("/imgs/1.png", {"before": "a red car, parked", "after": "a blue car"}, "car car"),
                     ("/imgs/2.png", {"before": "a house in winter", "after": "a house in summer"}, "house house")]
    gen = tmp_path / "gen.csv"
    gen.write_text("caption,file_name\nhello,0.jpg\nworld,1.jpg\n")
    assert loading.load_benchmark(str(gen)) == (["hello", "world"], ["0.jpg", "1.jpg"])


class StubEncoder:
    """image features = channel means and a constant, text features = functions of the ids: fp32 [n, 4]"""
    device = torch.device("cpu")

    def get_image_features(self, images):
        return torch.tensor([[*np.asarray(im, dtype=np.float64).mean((0, 1)), 1.0] for im in images], dtype=torch.float32)

    def get_text_features(self, ids):
        ids = torch.as_tensor(ids).float()
        return torch.stack([ids.sum(1), ids[:, 0], ids.max(1).values, torch.ones(len(ids))], 1)


def test_calc_all_writes_the_four_keys_and_leaves_an_empty_directory_alone(tmp_path, monkeypatch):
    from PIL import Image
    from invertible_cd_amd import metrics, ops
    monkeypatch.setattr(ops, "cosine_rows", lambda a, b: torch.nn.functional.cosine_similarity(a.float(), b.float(), dim=1))
    rng = np.random.default_rng(1)
    orig, edited, out, empty = (tmp_path / n for n in ("orig", "edited", "out", "empty"))
    for d in (orig, edited, empty):
        d.mkdir()
    for i in range(3):
        Image.fromarray(rng.integers(0, 256, (32, 48, 3), dtype=np.uint8)).save(orig / f"{i}.png")
    for name in ("10.png", "2.png", "1.png"):                    # numeric order: 1, 2, 10
        Image.fromarray(rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)).save(edited / name)
    models = dict(clip_model=StubEncoder(), dinov2_model=StubEncoder(), ir_model=StubReward(), tokenizer=StubTokenizer(),
                  ir_tokenizer=StubTokenizer())
    assert metrics.calc_all(str(orig), str(empty), GOLDEN_CSV, str(out), "cpu", **models) is None
    assert empty.is_dir() and not out.exists()                    # the reference deletes the directory; this does not
    res = metrics.calc_all(str(orig), str(edited), GOLDEN_CSV, str(out), "cpu", **models)
    with open(out / "editing_metrics_values.json") as f:
        saved = json.load(f)
    keys = ["preservation_clip_score", "preservation_dinov2", "editing_clip_score", "editing_imagereward"]
    assert sorted(saved) == sorted(keys) and saved == res
    assert all(isinstance(saved[k], str) and saved[k].startswith("[") for k in keys)
    assert models["ir_model"].calls == [3]
    # the stub's reward of (edited image in numeric order, edited caption)
    from invertible_cd_amd.generation import load_512
    imgs = [load_512(str(edited / n)) for n in ("1.png", "2.png", "10.png")]
    enc = StubTokenizer()(["a photo of a dog", "a blue car", "a house in summer"], max_length=35)
    want = [float(v) for v in StubReward.expected(enc["input_ids"], enc["attention_mask"], imgs)]
    assert saved["editing_imagereward"] == str(want)
    with pytest.raises(ValueError, match="ir_model="):
        metrics.calc_all(str(orig), str(edited), GOLDEN_CSV, str(out), "cpu", clip_model=StubEncoder(), dinov2_model=StubEncoder())
