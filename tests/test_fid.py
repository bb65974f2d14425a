"""FID, the host side (no GPU): Lanczos tables against Pillow, the Frechet distance against closed forms, the streaming statistics, the
BatchNorm fold, the loader, and the oracle of tests/inception_ref.py itself."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
import inception_ref

SIZES = [(512, 512), (300, 400), (333, 250), (256, 320), (200, 260)]


@pytest.mark.parametrize("h,w", SIZES)
def test_lanczos_tables_reproduce_pillows_resize_byte_for_byte(h, w):
    """torchvision's Resize(256): down-scaling, both orientations, an image that is left alone (256 x 320) and up-scaling (200 x 260);
    also with the identity passes run (what the device does: Pillow skips them)."""
    from PIL import Image
    from invertible_cd_amd import resample
    img = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    rh, rw, top, left = resample.fid_geometry(h, w, 256)
    assert min(rh, rw) == 256 and max(rh, rw) == int(256 * max(h, w) / min(h, w))
    want = np.array(Image.fromarray(img).resize((rw, rh), Image.LANCZOS))
    assert np.array_equal(resample.resize_emulated(img, rh, rw, "lanczos"), want)
    assert np.array_equal(resample.resize_emulated(img, rh, rw, "lanczos", skip_identity=False), want)
    assert np.array_equal(want[top:top + 256, left:left + 256], inception_ref.loader([img], 256)[0])
    for n_in, n_out in ((w, rw), (h, rh)):
        assert resample.resample_tables(n_in, n_out, "lanczos")[2].shape[1] == 2 * int(np.ceil(3 * max(n_in / n_out, 1))) + 1


def test_the_default_tables_are_the_bicubic_ones_unchanged():
    from invertible_cd_amd import resample
    for n_in, n_out in ((512, 224), (300, 224), (100, 150)):
        a, b = resample.resample_tables(n_in, n_out), resample.resample_tables(n_in, n_out, filter="bicubic")
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert a[2].shape[1] == resample.tap_width(n_in, n_out) == int(np.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1
    with pytest.raises(ValueError):
        resample.resample_tables(8, 8, filter="box")


def test_the_device_table_cache_keeps_the_filters_apart():
    """ops._resample_tables_dev holds BICUBIC and LANCZOS tables in one cache: the filter is part of the key, so neither is handed out
    for the other, a second call uploads nothing, and the bicubic entry is resample.resample_tables as it stands."""
    from invertible_cd_amd import ops, resample
    n_in, n_out = 300, 256
    bic, lan = ops._resample_tables_dev(n_in, n_out, "cpu", "bicubic"), ops._resample_tables_dev(n_in, n_out, "cpu", "lanczos")
    assert all(a is b for a, b in zip(bic, ops._resample_tables_dev(n_in, n_out, "cpu", "bicubic")))
    assert all(a is b for a, b in zip(bic, ops._resample_tables_dev(n_in, n_out, "cpu")))                # bicubic is the default
    assert all(a is b for a, b in zip(lan, ops._resample_tables_dev(n_in, n_out, "cpu", "lanczos")))
    assert not torch.equal(bic[2], lan[2])                      # the coefficients: another support, another row length
    for filt, got in (("bicubic", bic), ("lanczos", lan)):
        want = resample.resample_tables(n_in, n_out, filt)
        assert len(got) == len(want) == 3
        assert all(g.dtype == torch.int32 and torch.equal(g, torch.from_numpy(w.copy())) for g, w in zip(got, want))


def _spd(rng, d, n=None):
    x = rng.standard_normal((n or 4 * d, d)) @ rng.standard_normal((d, d))
    return x.mean(0), np.cov(x, rowvar=False)


@pytest.mark.parametrize("d", [16, 64])
def test_frechet_distance_against_closed_forms(d):
    from invertible_cd_amd.metrics import calculate_frechet_distance as fd
    rng = np.random.default_rng(d)
    mu, s = _spd(rng, d)
    assert abs(fd(mu, s, mu, s)) < 1e-8
    a, b, m1, m2 = rng.uniform(0.5, 2, d), rng.uniform(0.5, 2, d), rng.standard_normal(d), rng.standard_normal(d)
    want = ((m1 - m2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(fd(m1, np.diag(a), m2, np.diag(b)) - want) < 1e-9 * want
    for _ in range(3):
        (mu1, s1), (mu2, s2) = _spd(rng, d), _spd(rng, d)
        want = inception_ref.frechet_eig(mu1, s1, mu2, s2)
        assert abs(fd(mu1, s1, mu2, s2) - want) < 1e-9 * want
    (mu1, s1), (mu2, s2) = _spd(rng, d, n=d // 2), _spd(rng, d, n=d // 2)      # fewer samples than dimensions: singular covariances
    got = fd(mu1, s1, mu2, s2)
    assert np.isfinite(got) and got > 0


def test_frechet_distance_retries_a_singular_product_with_eps(monkeypatch, capsys):
    """Whether scipy's sqrtm of a singular product comes back finite depends on its version, so the branch is entered by hand: the first
    root is replaced by a non-finite matrix; the retry must say so and return the distance of sigma + eps I."""
    import scipy.linalg
    from invertible_cd_amd.metrics import calculate_frechet_distance as fd
    d, eps = 16, 1e-3
    rng = np.random.default_rng(5)
    (mu1, s1), (mu2, s2) = _spd(rng, d, n=d // 2), _spd(rng, d, n=d // 2)
    real, calls = scipy.linalg.sqrtm, []

    def sqrtm(a, *args, **kw):
        calls.append(a.copy())
        return np.full_like(a, np.inf) if len(calls) == 1 else real(a, *args, **kw)
    monkeypatch.setattr(scipy.linalg, "sqrtm", sqrtm)
    got = fd(mu1, s1, mu2, s2, eps=eps)
    assert "singular product" in capsys.readouterr().out and len(calls) == 2
    ridge = eps * np.eye(d)
    assert np.array_equal(calls[0], s1 @ s2) and np.allclose(calls[1], (s1 + ridge) @ (s2 + ridge), rtol=1e-14, atol=0)
    # the traces in the sum stay those of sigma itself, only the root sees the offset (as in the reference)
    want = inception_ref.frechet_eig(mu1, s1 + ridge, mu2, s2 + ridge) - 2 * d * eps
    assert abs(got - want) < 1e-9 * abs(want)
    monkeypatch.setattr(scipy.linalg, "sqrtm", lambda a, *args, **kw: real(a, *args, **kw) + 0.01j * np.eye(len(a)))
    with pytest.raises(ValueError, match="imaginary"):
        fd(mu1, s1, mu2, s2)
    monkeypatch.setattr(scipy.linalg, "sqrtm", lambda a, *args, **kw: real(a, *args, **kw) + 1e-5j * np.eye(len(a)))
    assert isinstance(fd(mu1, s1, mu2, s2), float)


def _sums(x):
    x = np.asarray(x, np.float64)
    return len(x), x.sum(0), x.T @ x


def test_statistics_finalize_and_merge():
    from invertible_cd_amd.metrics import FidStatistics
    x = np.random.default_rng(0).standard_normal((100, 24)).astype(np.float32) * 0.3 + 0.5
    mu, sigma = FidStatistics().add(*_sums(x)).finalize()
    assert np.abs(mu - np.mean(x.astype(np.float64), 0)).max() < 1e-12
    assert np.abs(sigma - np.cov(x.astype(np.float64), rowvar=False)).max() < 1e-12
    halves = FidStatistics().add(*_sums(x[:37])).merge(FidStatistics().add(*_sums(x[37:])))
    mu2, sigma2 = halves.finalize()
    assert halves.n == 100 and np.abs(mu2 - mu).max() < 1e-14 and np.abs(sigma2 - sigma).max() < 1e-14
    with pytest.raises(ValueError):
        FidStatistics().finalize()


def test_calculate_fid_refuses_other_dims(tmp_path):
    from invertible_cd_amd import metrics
    with pytest.raises(ValueError, match="2048"):
        metrics.calculate_fid([], str(tmp_path), dims=768, model=object())


@pytest.fixture(scope="module")
def reduced():
    from invertible_cd_amd import inception, synthetic
    cfg = inception.FID_INCEPTION_REDUCED
    return cfg, synthetic.synthetic_inception_state(cfg, seed=1)


def test_the_batchnorm_fold_equals_explicit_batchnorm(reduced):
    from invertible_cd_amd import inception
    cfg, sd = reduced
    folded = {}
    for name in cfg.convs():
        w, b = inception.fold_batchnorm(*(sd[name + k] for k in (".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean",
                                                                 ".bn.running_var")))
        folded[name] = (w.float(), b.float())
    x = inception_ref.network_input(inception_ref.structured_images(2, 75, 75, seed=3), 0)
    for a, b in zip(inception_ref.Net(folded).blocks(x), inception_ref.Net(sd).blocks(x)):
        assert rel_l2(a, b) < 1e-6
    assert tuple(a.shape) == (2, cfg.dims) and cfg.dims == 48
    assert all(c[0] % 8 == 0 for c in cfg.convs().values())
    kernels = {c[2:4] for c in cfg.convs().values()}
    assert {(5, 5), (1, 7), (7, 1), (1, 3), (3, 1), (3, 3), (1, 1)} <= kernels


def test_load_inception_reads_pth_and_safetensors_and_ignores_the_head(reduced, tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from invertible_cd_amd import inception, loading
    cfg, sd = reduced
    assert "fc.weight" in sd and any(k.endswith("num_batches_tracked") for k in sd)
    seen = []
    monkeypatch.setattr(inception, "FidInception", lambda c, s, device: seen.append((c, s)) or "model")
    torch.save(sd, tmp_path / "inception.pth")
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "inception.safetensors"))
    for name in ("inception.pth", "inception.safetensors"):
        assert loading.load_inception(str(tmp_path / name), device="cpu", config=cfg) == "model"
    assert loading.load_inception(sd, device="cpu", config=cfg) == "model"
    for c, s in seen:
        assert c is cfg and set(s) == set(cfg.state_dict_shapes())
        assert all(torch.equal(s[k], sd[k]) for k in s)
    with pytest.raises(FileNotFoundError):
        loading.load_inception(str(tmp_path / "missing.pth"))
    with pytest.raises(KeyError):
        inception.folded_weights(cfg, {k: v for k, v in sd.items() if k != "Mixed_7c.branch_pool.conv.weight"})


def test_the_recorded_emulation_error_of_the_full_network_reproduces():
    """inception_ref.EMU_FULL sets the device's bar in tests/test_fid_gpu.py: the pooled-feature rel-L2 of the fp16-storage emulation
    against the fp32 oracle, weight seeds 0 .. 2, each on structured_images(2, 96, 128, seed=10 + weight seed).  Recomputed here (the
    order of a CPU convolution's sums may move the last digits: 3 %)."""
    from invertible_cd_amd import inception, synthetic
    cfg = inception.FID_INCEPTION
    for seed, (recorded, max_act) in enumerate(zip(inception_ref.EMU_FULL_BY_SEED, inception_ref.MAX_ACT_BY_SEED)):
        w = inception.folded_weights(cfg, synthetic.synthetic_inception_state(cfg, seed=seed))
        x = inception_ref.network_input(inception_ref.loader(inception_ref.structured_images(2, 96, 128, seed=10 + seed), 256), 299)
        oracle, emulation = inception_ref.Net(w), inception_ref.Net(w, True)
        got = rel_l2(emulation.blocks(x)[-1], oracle.blocks(x)[-1])
        assert abs(got - recorded) < 0.03 * recorded, (seed, got, recorded)
        assert abs(oracle.max_abs - max_act) < 0.01 * max_act, (seed, oracle.max_abs)
    assert inception_ref.EMU_FULL == max(inception_ref.EMU_FULL_BY_SEED)


def test_oracle_shapes_at_full_width():
    from invertible_cd_amd import inception, synthetic
    cfg = inception.FID_INCEPTION
    assert cfg.dims == 2048 and len(cfg.convs()) == 94
    sd = synthetic.synthetic_inception_state(cfg, seed=0)
    x = inception_ref.network_input(inception_ref.loader(inception_ref.structured_images(1, 96, 128, seed=0), 256), 299)
    assert tuple(x.shape) == (1, 3, 299, 299)
    net = inception_ref.Net(sd)
    t = net.blocks(x)
    assert [tuple(a.shape[1:]) for a in t] == [(64, 73, 73), (192, 35, 35), (768, 17, 17), (2048,)]
    assert net.max_abs < 100                                                 # far inside fp16
