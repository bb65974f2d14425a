"""Prompt-to-prompt on the SDXL sampling path, host side (no GPU): the controllers' counters on SDXL's 140 modules in the whole-batch
layout, LocalBlend's map selection on SD1.5- and SDXL-shaped stores, and `generation_sdxl.sample_deterministic(controller=)` on a stub
pipe.  The `controller=` tests raise TypeError before the sampler took the argument; the `controller=None` case passes there by design."""
import os

import numpy as np
import pytest
import torch

from invertible_cd_amd import generation_sdxl as X
from invertible_cd_amd import p2p
from invertible_cd_amd.unet_config import SD15, SDXL
from stubs import StubPipe, StubTokenizer, sdxl_emb_fn

STEPS = 3
PAIR = ["a cat sitting on a bench", "a dog sitting on a bench"]


@pytest.fixture(autouse=True)
def _globals():
    p2p.tokenizer = StubTokenizer()
    p2p.device = "cpu"
    p2p.NUM_DDIM_STEPS = STEPS
    p2p.LOW_RESOURCE = False
    yield


def _walk(cfg, latent):
    """(place, is_cross, queries) of every Attention module of `cfg` in execution order at latent x latent."""
    levels = len(cfg.block_out_channels)
    queries = [(latent >> i) ** 2 for i in range(levels)]
    out = []
    for i in range(levels):
        if cfg.down_has_attn[i]:
            out += [("down", False, queries[i]), ("down", True, queries[i])] * (2 * cfg.transformer_layers[i])
    out += [("mid", False, queries[-1]), ("mid", True, queries[-1])] * cfg.transformer_layers[-1]
    for i in range(levels):
        lvl = levels - 1 - i
        if cfg.up_has_attn[i]:
            out += [("up", False, queries[lvl]), ("up", True, queries[lvl])] * (3 * cfg.transformer_layers[lvl])
    assert len(out) == cfg.num_attention_layers
    return out


def test_walks_have_the_reference_module_counts():
    assert len(_walk(SD15, 64)) == 32 and len(_walk(SDXL, 128)) == 140
    # SDXL at 128 x 128 latents: level 1 works at 64 x 64 (4096 queries, never stored), level 2 and the mid block at 32 x 32
    n = [q for _, _, q in _walk(SDXL, 128)]
    assert sorted(set(n)) == [1024, 4096] and n.count(1024) == 120 and n.count(4096) == 20


def _drive(controller, walk, rows, steps, heads=2):
    """The executor's whole-batch (cond-only) layout: every row of every materialised layer goes to call_cond_only, the other layers
    tick."""
    gen = torch.Generator().manual_seed(0)
    for step in range(steps):
        for place, is_cross, n in walk:
            if not controller.needs_probs(is_cross, n, place):
                controller.tick()
                continue
            P = torch.softmax(torch.randn(rows * heads, n, 77 if is_cross else n, generator=gen), dim=-1)
            assert controller.call_cond_only(P, is_cross, place) is P
        assert controller.cur_att_layer == 0 and controller.cur_step == step + 1          # one tick per step, on the last module


class _Stub140:
    """What register_attention_control needs of a UNet: SDXL's module count."""
    num_attention_layers = 140
    attn_controller = None


def test_counters_tick_once_per_step_on_sdxl_for_store_and_edit_controllers():
    walk = _walk(SDXL, 128)

    class M:
        unet = _Stub140()
    store = p2p.AttentionStore()
    p2p.register_attention_control(M, store)
    assert store.num_att_layers == 140 and M.unet.attn_controller is store
    # the N <= 32^2 rule keeps SDXL's 1024-query layers: 60 self + 60 cross maps per step (20 down, 10 mid, 30 up of each kind)
    kept = [(p, c) for p, c, n in walk if store.needs_probs(c, n, p)]
    assert len(kept) == 120 and sum(c for _, c in kept) == 60
    # (the counters and the store's structure depend on which side of 32^2 a layer is, not on its size: 1024 -> 16, 4096 -> 1025 queries)
    small = [(p, c, 1025 if n > 1024 else 16) for p, c, n in walk]
    _drive(store, small, 2, STEPS)
    assert {k: len(v) for k, v in store.attention_store.items()} == {"down_cross": 20, "mid_cross": 10, "up_cross": 30, "down_self": 20,
                                                                     "mid_self": 10, "up_self": 30}
    edit = p2p.make_controller(PAIR, True, 0.5, 0.5)
    p2p.register_attention_control(M, edit)
    # an edit controller also needs the 4096-query cross-attention layers (edited, not stored): 60 + 70
    assert sum(edit.needs_probs(c, n, p) for p, c, n in walk) == 130
    _drive(edit, small, 2, STEPS)
    assert len(edit.attention_store["down_cross"]) == 20 and len(edit.attention_store["up_cross"]) == 30


def _store_from(walk, n_prompts, heads, gen):
    """A store of the walk's <= 32^2-query layers; every word column carries a spatial pattern of its own (else the normalised heat is flat)."""
    store, pattern = p2p.AttentionStore.get_empty_store(), {}
    for place, is_cross, n in walk:
        if n <= 1024:
            if n not in pattern:
                pattern[n] = torch.rand(1, n, 77, generator=gen) ** 3
            m = torch.rand(n_prompts * heads, n, 77, generator=gen) * pattern[n] if is_cross else torch.rand(n_prompts * heads, n, 1, generator=gen)
            store[f"{place}_{'cross' if is_cross else 'self'}"].append(m)
    return store


def test_local_blend_selects_the_five_sd15_maps_and_the_fifty_sdxl_maps():
    gen = torch.Generator().manual_seed(1)
    lb = p2p.LocalBlend(PAIR, (("cat",), ("dog",)))
    s15 = _store_from(_walk(SD15, 64), 2, 2, gen)
    maps, side = lb.select_maps(s15, torch.zeros(2, 4, 64, 64))
    want = s15["down_cross"][2:4] + s15["up_cross"][:3]
    assert side == (16, 16) and len(maps) == 5 and all(a is b for a, b in zip(maps, want))
    sxl = _store_from(_walk(SDXL, 128), 2, 1, gen)
    maps, side = lb.select_maps(sxl, torch.zeros(2, 4, 128, 128))
    assert side == (32, 32) and len(maps) == 50 and len(sxl["mid_cross"]) == 10
    assert all(a is b for a, b in zip(maps, sxl["down_cross"] + sxl["up_cross"])) and all(m.shape[1] == 1024 for m in maps)
    # reduced SDXL (what the GPU loop test runs): 68 x 68 latents -> level 1 at 34 x 34 (not stored), level 2 at 17 x 17
    maps, side = lb.select_maps(_store_from(_walk(SDXL, 68), 2, 1, gen), torch.zeros(2, 4, 68, 68))
    assert side == (17, 17) and len(maps) == 50
    with pytest.raises(ValueError, match="quarter"):
        lb.select_maps(sxl, torch.zeros(2, 4, 64, 64))


def test_local_blend_on_the_golden_inputs_is_the_reference_slice_bit_for_bit(golden_dir):
    """The generalised selection against the code it replaces (down_cross[2:4] + up_cross[:3] as 16 x 16, written out here) on the
    store that the reference's golden run builds, and on an SD1.5-shaped store: the same latents, bit for bit."""
    g = np.load(os.path.join(golden_dir, "p2p.npz"))
    walk = list(zip(g["walk_place"].tolist(), [bool(x) for x in g["walk_cross"]], g["walk_n"].tolist()))
    x = torch.from_numpy(g["refine_lat_in"])
    for wk in (walk, _walk(SD15, 64)):
        gen = torch.Generator().manual_seed(2)
        store = _store_from(wk, 2, 2, gen)
        lb = p2p.LocalBlend(["a cat sitting on a bench", "a fluffy cat sitting on a red bench"], (("cat",), ("cat",)),
                            substruct_words=(("bench",), ("bench",)), th=(0.3, 0.4))
        got = lb.blend(x, store)
        layers = store["down_cross"][2:4] + store["up_cross"][:3]
        maps = torch.cat([m.reshape(2, -1, 1, 16, 16, 77) for m in layers], dim=1)
        mask = lb.get_mask(maps, lb.alpha_layers, True, x) * ~lb.get_mask(maps, lb.substruct_layers, False, x)
        want = x[:1] + mask.float() * (x - x[:1])
        assert torch.equal(got, want) and 0.0 < mask.float().mean() < 1.0


class _Recorder(p2p.EmptyControl):
    def __init__(self):
        self.seen = []

    def step_callback(self, x_t):
        self.seen.append(x_t.clone())
        return x_t + 1.0


def _sample(controller=None, prompts=("aa", "bb"), latents=None, **kw):
    pipe = StubPipe()
    extra = {} if controller is None and not kw.pop("pass_none", False) else {"controller": controller}
    _, lat = X.sample_deterministic(pipe, list(prompts), latents=latents, num_inference_steps=STEPS,
                                    generator=torch.Generator().manual_seed(3), guidance_scale=7.0, is_sdxl=True,
                                    timesteps=[339, 699, 999], compute_embeddings_fn=sdxl_emb_fn, return_latent=True, **extra)
    return pipe, lat


def test_sampler_calls_step_callback_once_per_step():
    rec = _Recorder()
    pipe, lat = _sample(rec)
    assert len(rec.seen) == STEPS == len(pipe.unet.calls)
    # the UNet of step k + 1 sees what step_callback returned after step k
    for k in range(1, STEPS):
        assert torch.equal(pipe.unet.calls[k]["x"], rec.seen[k - 1] + 1.0)
    assert torch.equal(lat, rec.seen[-1] + 1.0)
    assert rec.num_att_layers == 0                       # registered on the stub (a foreign UNet has no modules to hook)


def test_sampler_without_a_controller_is_unchanged(golden_dir):
    g = np.load(os.path.join(golden_dir, "sdxl_loops.npz"))
    pipe = StubPipe()
    _, lat = X.sample_deterministic(pipe, ["aa", "bb", "cc"], num_inference_steps=4, generator=torch.Generator().manual_seed(0),
                                    guidance_scale=7.0, is_sdxl=True, timesteps=[249, 499, 699, 999], compute_embeddings_fn=sdxl_emb_fn,
                                    return_latent=True)
    assert torch.equal(lat, torch.from_numpy(g["rev_B3_out"]))


def test_controller_none_and_empty_control_give_the_plain_latents():
    _, plain = _sample()
    _, none = _sample(None, pass_none=True)
    _, empty = _sample(p2p.EmptyControl())
    assert torch.equal(plain, none) and torch.equal(plain, empty)


def test_one_latent_is_expanded_over_the_prompts_and_groups_are_flattened():
    one = torch.randn(1, 4, 2, 2, generator=torch.Generator().manual_seed(4))
    rec = _Recorder()
    pipe, lat = _sample(rec, latents=one)
    assert lat.shape == (2, 4, 2, 2) and torch.equal(pipe.unet.calls[0]["x"][0], one[0]) and torch.equal(pipe.unet.calls[0]["x"][1], one[0])
    # prompt groups: G lists of P prompts, a ControllerBatch of G members, one latent per group
    batch = p2p.ControllerBatch([p2p.make_controller(PAIR, True, 0.5, 0.5), p2p.make_controller(PAIR, False, 0.5, 0.5)])
    two = torch.randn(2, 4, 2, 2, generator=torch.Generator().manual_seed(5))
    pipe, lat = _sample(batch, prompts=(PAIR, PAIR), latents=two)
    x0 = pipe.unet.calls[0]["x"]
    assert x0.shape == (4, 4, 2, 2) and torch.equal(x0[0], two[0]) and torch.equal(x0[1], two[0]) and torch.equal(x0[3], two[1])
    with pytest.raises(ValueError, match="ControllerBatch"):
        _sample(p2p.make_controller(PAIR, True, 0.5, 0.5), prompts=(PAIR, PAIR), latents=two)
    with pytest.raises(ValueError, match="3 latents for 2 prompts"):
        _sample(_Recorder(), latents=torch.zeros(3, 4, 2, 2))
