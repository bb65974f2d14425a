"""invertible_cd_amd.sampling: the one copy of what the SD1.5 and the SDXL sampler share, on the CPU.  The loops themselves are held bit
for bit to the reference's vectors by tests/test_generation_golden.py; here: the helpers are one object under both module names, the
boundary coefficients reproduce predicted_origin, the endpoint rule, the constant cache, and the two contexts."""
import json
import os
import types

import numpy as np
import pytest
import torch

from invertible_cd_amd import generation as G
from invertible_cd_amd import generation_sdxl as X
from invertible_cd_amd import sampling as S
from stubs import StubModel, StubPipe, StubScheduler, sdxl_emb_fn


def test_the_numeric_helpers_are_one_object_under_both_module_names():
    for name in ("extract_into_tensor", "guidance_scale_embedding", "predicted_origin", "linear_schedule_old"):
        assert getattr(G, name) is getattr(X, name) is getattr(S, name), name


def test_boundary_coefficients_reproduce_predicted_origin_bit_for_bit(golden_dir):
    """What the device branch hands to icd_x0_step, evaluated as the kernel's fp32 expression: equal to predicted_origin, and so to the
    reference's vectors, at every golden (t, s) pair, s == 0 among them."""
    po = np.load(os.path.join(golden_dir, "predicted_origin.npz"))
    tab = np.load(os.path.join(golden_dir, "alphas_cumprod.npz"))
    alpha, sigma = torch.from_numpy(tab["alpha_table"]), torch.from_numpy(tab["sigma_table"])
    x, eps = torch.from_numpy(po["x"]), torch.from_numpy(po["eps"])
    pairs = po["pairs"].tolist()
    assert any(s == 0 for _, s in pairs)
    for (t, s), ref in zip(pairs, po["out"]):
        coef = S.boundary_coefficients(t, s, alpha, sigma)
        assert len(coef) == 4 and all(type(c) is float for c in coef)
        alpha_t, sigma_t, alpha_s, sigma_s = coef
        if s == 0:
            assert (alpha_s, sigma_s) == (1.0, 0.0)
        got = alpha_s * ((x - sigma_t * eps) / alpha_t) + sigma_s * eps
        assert got.dtype == torch.float32
        assert torch.equal(got, S.predicted_origin(eps, torch.tensor([t, t]), torch.tensor([s, s]), x, "epsilon", alpha, sigma))
        assert torch.equal(got, torch.from_numpy(ref))
        # the host branch of boundary_step is that expression, cast to the caller's dtype
        step = S.boundary_step(eps, t, s, x, "epsilon", alpha, sigma, torch.float16, S.ConstCache())
        assert step.dtype == torch.float16 and torch.equal(step, got.half())


def test_endpoint_rule_reproduces_both_reference_tables(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "timesteps.json")))
    grid = torch.from_numpy(S.ddim_grid(50)).long()
    assert grid.tolist() == g["ddimsolver_1"]["ddim_timesteps"]
    for k in (1, 2, 3, 4):
        ends, inv_ends = S.interval_endpoints(grid, k, 49)
        d, e = g[f"ddimsolver_{k}"], g[f"default_{k}"]
        assert ends.tolist() == d["endpoints"] and inv_ends.tolist() == d["inverse_endpoints"]
        assert inv_ends.flip(0).tolist() == e["reverse_timesteps"] and ends.flip(0).tolist() == e["reverse_boundary"]
        assert [19] + ends.tolist()[1:] == e["forward_timesteps"] and inv_ends.tolist() == e["forward_boundary"]


def test_const_cache_keeps_clears_and_tells_schedules_apart():
    cache, made = S.ConstCache(), []

    def make():
        made.append(1)
        return object()
    first = cache.get("k", make)
    assert cache.get("k", make) is first and len(made) == 1
    for i in range(1, 256):
        cache.get(("fill", i), make)
    assert len(cache.entries) == 256 and cache.get("k", make) is first
    cache.get("entry 257", make)                                        # the bound: the cache empties, then takes the new entry
    assert list(cache.entries) == ["entry 257"]
    assert cache.get("k", make) is not first
    # one process-wide cache, two schedulers: the same (t, s, B) must not hand the first scheduler's coefficients to the second
    a1, s1 = S.schedules(StubScheduler())
    other = types.SimpleNamespace(alphas_cumprod=StubScheduler().alphas_cumprod ** 2)
    a2, s2 = S.schedules(other)
    cache = S.ConstCache()
    c1 = S.coefficient_rows(259, 19, 2, "cpu", a1, s1, cache)
    c2 = S.coefficient_rows(259, 19, 2, "cpu", a2, s2, cache)
    assert c1 is not c2 and len(cache.entries) == 2 and not torch.equal(c1, c2)
    assert S.coefficient_rows(259, 19, 2, "cpu", a1, s1, cache) is c1
    assert c1.dtype == torch.float32 and c1.tolist() == [list(torch.tensor(S.boundary_coefficients(259, 19, a1, s1)).tolist())] * 2


class _Unet:
    def __init__(self, cond_only):
        self.attn_cond_only, self.depth = cond_only, 0

    def editing(self):
        unet = self

        class Ctx:
            def __enter__(self):
                unet.depth += 1

            def __exit__(self, *exc):
                unet.depth -= 1
        return Ctx()


@pytest.mark.parametrize("prior", [False, True])
def test_cond_only_restores_the_prior_value_when_the_body_raises(prior):
    unet = _Unet(prior)
    with pytest.raises(RuntimeError):
        with S.cond_only(unet):
            assert unet.attn_cond_only is True
            raise RuntimeError("body")
    assert unet.attn_cond_only is prior                                 # a prior True stays True: restored, not reset
    with S.cond_only(unet, on=False):
        assert unet.attn_cond_only is prior
    with S.cond_only(object(), on=False):                               # off: the UNet is not touched (a foreign one has no such attribute)
        pass


def test_editing_restores_the_prior_state_when_the_body_raises():
    model = types.SimpleNamespace(unet=_Unet(False))
    with pytest.raises(RuntimeError):
        with S.editing(model, True):
            assert model.unet.depth == 1
            raise RuntimeError("body")
    assert model.unet.depth == 0
    with S.editing(model, False):
        assert model.unet.depth == 0
    with S.editing(types.SimpleNamespace(unet=object()), True):        # a UNet without editing(): no-op
        pass
    with S.editing(object(), True):
        pass


def _count_makes(monkeypatch):
    made = []
    get = S.ConstCache.get

    def counting(self, key, make):
        return get(self, key, lambda: (made.append(key), make())[1])
    monkeypatch.setattr(S.ConstCache, "get", counting)
    return made


def test_a_second_run_builds_no_new_constant(monkeypatch):
    made = _count_makes(monkeypatch)
    m = StubModel()
    s = G.Generator(m, 50, StubScheduler(), forward_cons_model=m, reverse_cons_model=m, reverse_timesteps=[259, 519, 779, 999],
                    forward_timesteps=[19, 259, 519, 779])
    s.context = torch.zeros(4, 77, 8)
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(0))
    run = lambda: s.cons_generation(lat, guidance_scale=19.0, w_embed_dim=512, dynamic_guidance=True, tau1=0.8, tau2=0.8)[-1]
    a = run()
    assert len(made) == 2                                               # w = 0 above tau, then [0, 0, 0, gs]
    b = run()
    assert len(made) == 2 and torch.equal(a, b)

    del made[:]
    X._CONSTS.entries.clear()
    p = StubPipe()
    run = lambda: X.sample_deterministic(p, ["aa", "bb"], num_inference_steps=3, generator=torch.Generator().manual_seed(1),
                                         guidance_scale=19.0, is_sdxl=True, timesteps=[339, 699, 999], compute_embeddings_fn=sdxl_emb_fn,
                                         use_dynamic_guidance=True, tau1=0.7, tau2=0.7, return_latent=True)[1]
    a = run()
    assert len(made) == 2                                               # the static embedding (gs) and w = 0 at t = 999
    b = run()
    assert len(made) == 2 and torch.equal(a, b)
