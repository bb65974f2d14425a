"""Batched prompt-to-prompt editing on the host (no GPU): p2p.ControllerBatch, runner with prompt groups and invert with one seed per
image must give every group exactly - bit for bit - what its controller gives when it runs alone on its own rows."""
import numpy as np
import pytest
import torch

from invertible_cd_amd import generation as G
from invertible_cd_amd import inversion, p2p
from stubs import StubModel, StubScheduler, StubTokenizer

HEADS = 2
STEPS = 4


@pytest.fixture(autouse=True)
def _globals():
    p2p.tokenizer = StubTokenizer()
    p2p.device = "cpu"
    p2p.NUM_DDIM_STEPS = STEPS
    p2p.LOW_RESOURCE = False
    yield


def _sd15_walk():
    """(place, is_cross, queries) of SD1.5's 32 Attention modules in execution order at 64 x 64 latents."""
    walk = []
    for n in (4096, 1024, 256):
        walk += [("down", False, n), ("down", True, n)] * 2
    walk += [("mid", False, 64), ("mid", True, 64)]
    for n in (256, 1024, 4096):
        walk += [("up", False, n), ("up", True, n)] * 3
    assert len(walk) == 32
    return walk


def _drive(batch, alone, n_prompts, seed, blend=True):
    """Drive the batch and the lone members through the same probabilities (cond rows only, as the executor hands them over when the
    dead unconditional half is eliminated) and the same latents; check every edited row and every latent on the way."""
    gen = torch.Generator().manual_seed(seed)
    n_groups = len(alone)
    rows = n_prompts * HEADS
    walk = _sd15_walk()
    batch.num_att_layers = len(walk)
    for c in alone:
        c.num_att_layers = len(walk)
    x = torch.randn(n_groups * n_prompts, 4, 64, 64, generator=gen)
    xs = [x[g * n_prompts:(g + 1) * n_prompts].clone() for g in range(n_groups)]
    n_edited = 0
    for _ in range(STEPS):
        for place, is_cross, n in walk:
            need = batch.needs_probs(is_cross, n, place)
            assert all(c.needs_probs(is_cross, n, place) == need for c in alone)
            if not need:
                batch.tick()
                for c in alone:
                    c.tick()
                continue
            m = 77 if is_cross else n
            P = torch.softmax(torch.randn(n_groups * rows, n, m, generator=gen) * 2.0, dim=-1)
            before = P.clone()
            batch.call_cond_only(P, is_cross, place)
            for g, c in enumerate(alone):
                Pg = before[g * rows:(g + 1) * rows].clone()
                c.call_cond_only(Pg, is_cross, place)
                assert torch.equal(P[g * rows:(g + 1) * rows], Pg), (place, is_cross, n, g)
            n_edited += not torch.equal(P, before)
        if blend:
            x = batch.step_callback(x)
            for g, c in enumerate(alone):
                xs[g] = c.step_callback(xs[g])
                assert torch.equal(x[g * n_prompts:(g + 1) * n_prompts], xs[g]), g
    assert batch.cur_step == STEPS
    for g, c in enumerate(alone):
        mb = batch.members[g]
        assert mb.cur_step == c.cur_step == STEPS and mb.cur_att_layer == c.cur_att_layer == 0
        assert mb.attention_store.keys() == c.attention_store.keys()
        for key in c.attention_store:
            assert len(mb.attention_store[key]) == len(c.attention_store[key])
            for a, b in zip(mb.attention_store[key], c.attention_store[key]):
                assert torch.equal(a, b), (g, key)
        avg_b, avg_a = mb.get_average_attention(), c.get_average_attention()
        for key in avg_a:
            assert all(torch.equal(a, b) for a, b in zip(avg_b[key], avg_a[key])), (g, key)
        if getattr(mb, "local_blend", None) is not None:
            assert mb.local_blend.counter == c.local_blend.counter == STEPS
    return n_edited


PAIR_A = ["a cat sitting on a bench", "a dog sitting on a bench"]
PAIR_B = ["a red car on the road", "a red fast car on the road"]
PAIR_C = ["a bird on a tree", "a crow on a tree"]
PAIR_D = ["a red car on the road", "a red bus on the road"]


def _three_groups():
    """Replace; Refine + LocalBlend with substruct words (its own self window); Reweight chained on Replace with a LocalBlend."""
    replace = p2p.make_controller(PAIR_A, True, 0.5, 0.5)
    lb = p2p.LocalBlend(PAIR_B, (("car",), ("car",)), substruct_words=(("road",), ("road",)), start_blend=0.2, th=(0.3, 0.4))
    refine = p2p.AttentionRefine(PAIR_B, STEPS, cross_replace_steps={"default_": 0.8, "fast": (0.0, 0.5)}, self_replace_steps=0.25,
                                 local_blend=lb)
    reweight = p2p.make_controller(PAIR_C, True, 0.8, 0.6, blend_words=(("bird",), ("crow",)),
                                   equilizer_params={"words": ("crow",), "values": (4.0,)})
    return [replace, refine, reweight]


def test_controller_batch_matches_each_member_alone_bit_for_bit():
    batch = p2p.ControllerBatch(_three_groups())
    assert batch.n_groups == 3 and batch.n_prompts == 2 and batch.is_edit
    assert isinstance(batch, p2p.AttentionControl)
    assert batch.self_window(0) is True and batch.self_window(1) is None and batch.self_window(3) is False
    n = _drive(batch, _three_groups(), 2, seed=3)
    assert n > 0


def test_controller_batch_of_three_prompt_groups():
    def make():
        prompts = ["a cat sitting on a bench", "a dog sitting on a bench", "a fox sitting on a bench"]
        return [p2p.make_controller(prompts, True, 0.5, 0.5, blend_words=(("cat",), ("dog",), ("fox",))),
                p2p.make_controller(["a cat on a mat", "a cat on a rug", "a cat on a bed"], True, 0.7, 0.4)]
    batch = p2p.ControllerBatch(make())
    assert batch.n_prompts == 3
    _drive(batch, make(), 3, seed=4)


def test_controller_batch_of_attention_stores():
    batch = p2p.ControllerBatch([p2p.AttentionStore() for _ in range(3)])
    assert not batch.is_edit
    _drive(batch, [p2p.AttentionStore() for _ in range(3)], 2, seed=5, blend=False)


def test_controller_batch_refuses_unequal_groups_and_mixed_kinds():
    with pytest.raises(ValueError):
        p2p.ControllerBatch([p2p.make_controller(PAIR_A, True, 0.5, 0.5),
                             p2p.make_controller(PAIR_A + ["a fox sitting on a bench"], True, 0.5, 0.5)])
    with pytest.raises(ValueError):
        p2p.ControllerBatch([p2p.AttentionStore(), p2p.make_controller(PAIR_A, True, 0.5, 0.5)])
    with pytest.raises(ValueError):
        p2p.ControllerBatch([])


# ------------------------------------------------------------------------------------------------ runner / invert on the stubs
def _solver(model=None):
    m = model or StubModel()
    s = G.Generator(m, 50, StubScheduler(), forward_cons_model=m, reverse_cons_model=m,
                    reverse_timesteps=[259, 519, 779, 999], forward_timesteps=[19, 259, 519, 779])

    def init_prompt(prompt, unc=None):
        n = len(prompt)
        s.context, s.prompt = torch.zeros(2 * n, 77, 8), prompt
    s.init_prompt = init_prompt
    return m, s


@pytest.mark.parametrize("tau", [0.8, 1.0])
def test_runner_with_prompt_groups_equals_one_call_per_group(tau):
    groups = [PAIR_A, PAIR_D, PAIR_C]
    kw = dict(is_cons_forward=True, num_inference_steps=50, guidance_scale=19.0, return_type="latent", dynamic_guidance=True,
              tau1=tau, tau2=tau, w_embed_dim=512)
    m, s = _solver()
    batch = p2p.ControllerBatch([p2p.make_controller(p, True, 0.5, 0.5) for p in groups])
    out, lat = G.runner(model=m, prompt=groups, controller=batch, solver=s, generator=torch.Generator().manual_seed(21), latent=None, **kw)
    init = torch.randn((3, 4, 64, 64), generator=torch.Generator().manual_seed(21))
    assert torch.equal(lat, init) and out.shape == (6, 4, 64, 64)
    assert s.prompt_groups is None
    for g, p in enumerate(groups):
        m1, s1 = _solver()
        o1, l1 = G.runner(model=m1, prompt=p, controller=p2p.make_controller(p, True, 0.5, 0.5), solver=s1, latent=init[g:g + 1], **kw)
        assert torch.equal(out[2 * g:2 * g + 2], o1), g
        # the reference's w vector of a lone pair ([0, 0, 0, gs] for the CFG-doubled batch of 4) is kept per group
        for cb, c1 in zip(m.unet.calls, m1.unet.calls):
            assert torch.equal(cb["cond"][6 + 2 * g:8 + 2 * g], c1["cond"][2:])


def test_runner_with_prompt_groups_and_per_step_uncond_embeddings():
    groups = [PAIR_A, PAIR_C]
    m, s = _solver()
    unc = [torch.randn(2, 77, 8, generator=torch.Generator().manual_seed(i)) for i in range(50)]
    seen = []
    orig = s.init_prompt

    def init_prompt(prompt, u=None):
        seen.append(None if u is None else u.clone())
        orig(prompt, u)
    s.init_prompt = init_prompt
    lat = torch.randn((2, 4, 64, 64), generator=torch.Generator().manual_seed(2))
    batch = p2p.ControllerBatch([p2p.make_controller(p, True, 0.5, 0.5) for p in groups])
    out, _ = G.runner(model=m, prompt=groups, controller=batch, solver=s, is_cons_forward=False, num_inference_steps=3, guidance_scale=1.0,
                      latent=lat, uncond_embeddings=unc, return_type="latent")
    assert seen[0] is None and len(seen) == 4
    for i, u in enumerate(seen[1:]):
        assert torch.equal(u, unc[i].repeat_interleave(2, 0))
    for g, p in enumerate(groups):
        m1, s1 = _solver()
        o1, _ = G.runner(model=m1, prompt=p, controller=p2p.make_controller(p, True, 0.5, 0.5), solver=s1, is_cons_forward=False,
                         num_inference_steps=3, guidance_scale=1.0, latent=lat[g:g + 1], uncond_embeddings=[u[g:g + 1] for u in unc],
                         return_type="latent")
        assert torch.equal(out[2 * g:2 * g + 2], o1), g


def test_runner_refuses_mismatched_groups():
    m, s = _solver()
    batch = p2p.ControllerBatch([p2p.make_controller(p, True, 0.5, 0.5) for p in (PAIR_A, PAIR_D)])
    kw = dict(solver=s, is_cons_forward=True, return_type="latent", w_embed_dim=512, tau1=1.0, tau2=1.0)
    with pytest.raises(ValueError):                                  # latent batch != G
        G.runner(model=m, prompt=[PAIR_A, PAIR_D], controller=batch, latent=torch.zeros(3, 4, 64, 64), **kw)
    with pytest.raises(ValueError):                                  # unequal group sizes
        G.runner(model=m, prompt=[PAIR_A, PAIR_D + ["x y"]], controller=batch, **kw)
    with pytest.raises(ValueError):                                  # G != members
        G.runner(model=m, prompt=[PAIR_A, PAIR_D, PAIR_C], controller=batch, **kw)
    with pytest.raises(ValueError):                                  # groups without a ControllerBatch
        G.runner(model=m, prompt=[PAIR_A, PAIR_D], controller=p2p.AttentionStore(), **kw)


def test_invert_with_a_seed_list_equals_one_inversion_per_image(monkeypatch):
    images = {f"img{g}.png": np.random.default_rng(g).standard_normal((4, 64, 64)).astype(np.float32) for g in range(2)}
    monkeypatch.setattr(inversion, "load_512", lambda path, *offsets: images[path])

    def solver():
        m, s = _solver()
        s.image2latent = lambda im: (torch.stack([torch.from_numpy(i) for i in im]) if isinstance(im, list) else torch.from_numpy(im)[None])
        s.latent2image = lambda z, return_type="np": np.zeros((1,))
        return m, s
    kw = dict(stop_step=50, is_cons_inversion=True, inv_guidance_scale=3.0, w_embed_dim=512, do_npi=True)
    m, s = solver()
    _, lat, npi = inversion.invert(s, image_path=list(images), prompt=["a cat", "a dog"], seed=[5, 9], **kw)
    assert lat.shape == (2, 4, 64, 64) and len(npi) == 50 and npi[0].shape == (2, 77, 8)
    for g, path in enumerate(images):
        m1, s1 = solver()
        _, l1, _ = inversion.invert(s1, image_path=path, prompt=["a cat", "a dog"][g], seed=[5, 9][g], **kw)
        assert torch.equal(lat[g:g + 1], l1), g
    # an int seed keeps the one batch-wide draw (and the reference's w vector of the whole batch)
    m2, s2 = solver()
    _, l2, _ = inversion.invert(s2, image_path=list(images), prompt=["a cat", "a dog"], seed=5, **kw)
    noise = torch.randn((2, 4, 64, 64), generator=torch.Generator().manual_seed(5))
    x0 = s2.noise_scheduler.add_noise(torch.stack([torch.from_numpy(i) for i in images.values()]), noise, torch.tensor([19]))
    assert torch.equal(m2.unet.calls[0]["x"][:2], x0)
    with pytest.raises(ValueError):
        inversion.invert(solver()[1], image_path=list(images), prompt=["a cat", "a dog"], seed=[5], **kw)


def test_the_epilogue_struct_keeps_its_size_and_names_group_count():
    from invertible_cd_amd import _lib
    import ctypes
    assert ctypes.sizeof(_lib.ProbsEpilogue) == 48
    assert [f for f, _ in _lib.ProbsEpilogue._fields_][-1] == "group_count"


def test_a_mismatched_group_count_is_refused_before_any_launch():
    """Argument validation of icd_attention_probs_ex returns INVALID_ARG before any HIP call (host pointers are never dereferenced)."""
    from invertible_cd_amd import _lib
    import ctypes
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)

    def call(edit_count, group_count, first=0):
        e = _lib.ProbsEpilogue()
        e.first_cond_sample, e.self_from_base, e.edit_count, e.group_count = first, 1, edit_count, group_count
        return lib.icd_attention_probs_ex(fake, None, fake, None, fake, 6, 2, 64, 77, 40, 80, 80, 80, 0.1, ctypes.byref(e), None)
    assert call(0, 2) == -1 and b"edit_count" in lib.icd_last_error()
    assert call(1, 2) == -1 and b"groups" in lib.icd_last_error()
    assert call(1, 2, first=1) == -1 and call(2, 3) == -1
