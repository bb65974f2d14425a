"""Host side of the shared encoder module (encoder.py): the one weight fold behind the three towers and the grouping by image size: no GPU."""
import pytest
import torch


def test_fold_output_is_the_fold_of_every_tower():
    """The image tower folds the V bias in float64 without a LayerScale, DINOv2 with one, the text tower in fp32: a LayerScale of ones is
    the fold without one bit for bit (a product with 1.0 is exact), and the fp32 fold is the plain fp32 expression."""
    from invertible_cd_amd import dinov2, encoder
    g = torch.Generator().manual_seed(7)
    C = 40
    W, b, v, lam = torch.randn(C, C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    w0, b0 = encoder.fold_output(W, b, v, lam=None)
    w1, b1 = encoder.fold_output(W, b, v, lam=torch.ones(C))
    assert w0.dtype == b0.dtype == w1.dtype == b1.dtype == torch.float64
    assert torch.equal(w0, w1) and torch.equal(b0, b1)
    assert torch.equal(w0, W.double()) and torch.equal(b0, W.double() @ v.double() + b.double())
    w32, b32 = encoder.fold_output(W, b, v, dtype=torch.float32)
    assert w32.dtype == b32.dtype == torch.float32 and torch.equal(w32, W) and torch.equal(b32, W @ v + b)
    # without a V bias and a LayerScale nothing is folded; dinov2.fold_layer_scale is the same function under its earlier name
    wn, bn = encoder.fold_output(W, b)
    assert torch.equal(wn, W.double()) and torch.equal(bn, b.double())
    wl, bl = encoder.fold_output(W, b, v, lam)
    wd, bd = dinov2.fold_layer_scale(W, b, lam, v)
    assert torch.equal(wl, wd) and torch.equal(bl, bd)
    assert torch.equal(wl, lam.double()[:, None] * W.double()) and torch.equal(bl, lam.double() * b0)


def test_run_by_size_runs_each_group_once_and_keeps_the_callers_order():
    from invertible_cd_amd import encoder
    sizes = [(8, 8), (4, 6), (8, 8), (2, 2), (4, 6)]
    calls = []

    def run(idx):
        calls.append(list(idx))
        return torch.tensor([[float(i), 10.0 * i] for i in idx])
    out = encoder.run_by_size(len(sizes), lambda i: sizes[i], run)
    assert calls == [[0, 2], [1, 4], [3]]
    assert torch.equal(out, torch.tensor([[float(i), 10.0 * i] for i in range(5)]))
    calls.clear()
    one = encoder.run_by_size(3, lambda i: (8, 8), run)          # one size: one call, its result as it is
    assert calls == [[0, 1, 2]] and tuple(one.shape) == (3, 2)
    assert encoder.image_size(torch.zeros(5, 7, 3)) == (5, 7)


def test_checks_name_the_model_and_the_key():
    from invertible_cd_amd import encoder
    sd = {"a.weight": torch.zeros(2, 3), "a.bias": torch.zeros(2)}
    encoder.check_state_dict(sd, {"a.weight": (2, 3), "a.bias": (2,)}, "Toy")
    with pytest.raises(KeyError, match="Toy state dict lacks 1 tensors"):
        encoder.check_state_dict(sd, {"a.weight": (2, 3), "b.weight": (2,)}, "Toy")
    with pytest.raises(ValueError, match="a.bias"):
        encoder.check_state_dict(sd, {"a.weight": (2, 3), "a.bias": (3,)}, "Toy")
    encoder.check_widths("Toy", 128, 2, 512, "gelu", extra=(64,))
    for bad in (dict(hidden=128, heads=3), dict(hidden=120, heads=10), dict(hidden=1024, heads=4), dict(intermediate=510), dict(extra=(60,))):
        kw = dict(dict(hidden=128, heads=2, intermediate=512, extra=()), **bad)
        with pytest.raises(ValueError, match="Toy: head dim must be a multiple of 8 and <= 160"):
            encoder.check_widths("Toy", kw["hidden"], kw["heads"], kw["intermediate"], "gelu", kw["extra"])
    with pytest.raises(ValueError, match="hidden_act"):
        encoder.check_widths("Toy", 128, 2, 512, "relu")
