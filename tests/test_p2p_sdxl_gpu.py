"""Prompt-to-prompt on the SDXL sampling path on the MI355X: the widened device entries (icd_accumulate_multi_n, icd_local_blend_groups_ws)
at SDXL's counts, and `generation_sdxl.sample_deterministic(controller=)` on a reduced-width SDXL UNet (all 140 Attention modules, head
dim 64) against the fp32 oracle driving the same controller classes on the CPU."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from p2p_sdxl_inputs import blend_inputs, blend_masks, blend_with

pytestmark = pytest.mark.gpu

MASK_CAP = 5e-3            # a threshold of rounded values: at most 0.5 % of the mask may differ (the cap of test_p2p_gpu.py)


# ------------------------------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("n_tensors", [33, 130, 37])
def test_accumulate_multi_past_32_tensors_is_torch_inplace_add(n_tensors):
    """One launch (icd_accumulate_multi_n: pointer table on the device) for 33 / 130 (an SDXL step's stores and then some) / 37 tensors of
    mixed sizes - counts that are no multiple of 8 among them: tails, a single element, maps of SDXL's 17 x 17 test level -, bit-equal to
    torch's fp16 `+=`.  Before the entry existed the front end split such a list into launches of 32."""
    from invertible_cd_amd import ops
    gen = torch.Generator().manual_seed(8)
    shapes = [(8, 289, 77), (8, 289, 289), (3, 5, 7), (16, 256, 77), (1, 1, 1), (2, 1024, 80), (5, 9)]
    shapes = [shapes[i % len(shapes)] for i in range(n_tensors)]
    dst = [torch.rand(s, generator=gen).half().cuda() for s in shapes]
    src = [torch.rand(s, generator=gen).half().cuda() for s in shapes]
    want = [d.clone() for d in dst]
    for w, s_ in zip(want, src):
        w += s_
    ops.accumulate_multi(dst, src)
    for d, w in zip(dst, want):
        assert torch.equal(d, w)


def _check_blend(got, maps_dev, alpha, sub, x, use_sub):
    """got against the torch expression of LocalBlend.__call__ evaluated in fp32 on the same fp16 maps: every element is one of the two
    values the blend can give (mask 0 / mask 1), exactly; elements on the other side of the mask than the fp32 evaluation: <= 0.5 %."""
    main, cleared = blend_masks(maps_dev, alpha, sub, 0.3, x.shape[2:], torch.float32)
    mask = cleared if use_sub else main
    want = blend_with(mask, x)
    off, on = blend_with(torch.zeros_like(mask), x), blend_with(torch.ones_like(mask), x)
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
    assert bool(((got == off) | (got == on)).all())                           # bit-exact wherever the masks agree ...
    bad = (got != want).float().mean().item()                                  # ... and they disagree on a few border pixels at most
    frac = mask.float().mean().item()
    print(f"[local blend {len(maps_dev)} layers res {int(maps_dev[0].shape[1] ** 0.5)} sub={use_sub}] mask on {frac:.3f}, elements off {bad * 100:.4f} %")
    assert bad <= MASK_CAP and not (got[0] != want[0]).any()
    assert 0.02 < frac < 0.98                                                  # both branches of the mask are exercised
    return mask


def test_local_blend_at_sdxl_size_matches_the_torch_expression():
    """res 32, 50 layers x 20 heads, P = 2, latent 128 x 128 (what LocalBlend selects on SDXL at 1024 x 1024 images), with and without
    substruct words.  Seed 43: evaluating the torch expression itself with fp16 operands instead of fp32 moves 0 of the 32768 mask
    elements on the CPU (asserted below on the device as well), so the cap is not spent on the inputs."""
    from invertible_cd_amd import ops
    maps, alpha, sub, x = blend_inputs(seed=43, P=2, heads=20, n_layers=50, res=32, latent=128)
    dev = [m.cuda() for m in maps]
    del maps
    x = x.cuda()
    m16 = blend_masks(dev, alpha, sub, 0.3, x.shape[2:], torch.float16)
    m32 = blend_masks(dev, alpha, sub, 0.3, x.shape[2:], torch.float32)
    for a, b in zip(m16, m32):
        assert (a != b).float().mean().item() <= MASK_CAP
    for use_sub in (False, True):
        got = ops.local_blend(dev, alpha, sub if use_sub else None, 0.3, 0.3, x, res=32)
        _check_blend(got, dev, alpha, sub, x, use_sub)


def test_local_blend_at_sd15_size_gives_the_bits_of_the_one_launch_kernel(golden_dir):
    """res 16, 5 layers x 8 heads, P = 3: tests/golden/p2p_sdxl_blend16.npz holds what ops.local_blend returned for these inputs before
    the heat maps moved into a launch of their own (recorded on an MI355X from the parent commit).  Same bits: the terms are still added
    words first, then heads, then layers.  Also through the workspace-less C entry (icd_local_blend), which keeps the one-launch form."""
    import ctypes as C
    from invertible_cd_amd import _lib, ops
    g = np.load(os.path.join(golden_dir, "p2p_sdxl_blend16.npz"))
    maps, alpha, sub, x = blend_inputs(seed=41, P=3, heads=8, n_layers=5, res=16, latent=64)
    assert float(sum(m.double().sum() for m in maps)) == float(g["maps_checksum"][0])        # the inputs are the recorded run's
    dev, x = [m.cuda() for m in maps], x.cuda()
    for key, a_sub in (("plain", None), ("sub", sub)):
        got = ops.local_blend(dev, alpha, a_sub, 0.3, 0.3, x)
        assert torch.equal(got.cpu(), torch.from_numpy(g[key])), key
        _check_blend(got, dev, alpha, sub, x, a_sub is not None)
        ptrs, heads = (C.c_void_p * 5)(*[m.data_ptr() for m in dev]), (C.c_int32 * 5)(*[8] * 5)
        al, als = alpha.cuda().contiguous(), None if a_sub is None else a_sub.cuda().contiguous()
        out = torch.empty_like(got)
        _lib.check(_lib.load().icd_local_blend(ptrs, heads, 5, 3, 16, 77, dev[0].stride(1), ops._p(al), ops._p(als), 0.3, 0.3, ops._p(x), 0, 4, 64,
                                               64, ops._p(out), ops._stream()), "icd_local_blend")
        assert torch.equal(out, got), key


def test_local_blend_groups_with_an_odd_side_and_an_inactive_group():
    """The loop test's geometry (17 x 17 maps: 289 pixels, no multiple of the reduce launch's 16-pixel tile; 68 x 68 latents) for two prompt
    groups, the second without substruct words and the first one also run alone: each group is what a call of its own gives, an inactive
    group comes back unchanged."""
    from invertible_cd_amd import ops
    maps, alpha, sub, x = blend_inputs(seed=47, P=4, heads=4, n_layers=7, res=17, latent=68)
    dev, x = [m.cuda() for m in maps], x.cuda()
    both = ops.local_blend_groups(dev, alpha, (sub, [True, False]), [0.3, 0.3], [0.3, 0.3], [True, True], x, 2, res=17)
    for g, use_sub in ((0, True), (1, False)):
        rows = slice(2 * g, 2 * g + 2)
        part = [m[2 * g * 4:(2 * g + 2) * 4] for m in dev]
        alone = ops.local_blend(part, alpha[rows], sub[rows] if use_sub else None, 0.3, 0.3, x[rows].contiguous(), res=17)
        assert torch.equal(both[rows], alone)
        _check_blend(alone, part, alpha[rows], sub[rows], x[rows], use_sub)
    off = ops.local_blend_groups(dev, alpha, None, [0.3, 0.3], [0.3, 0.3], [True, False], x, 2, res=17)
    assert torch.equal(off[2:], x[2:].float()) and torch.equal(off[:2], ops.local_blend([m[:8] for m in dev], alpha[:2], None, 0.3, 0.3,
                                                                                         x[:2].contiguous(), res=17))


# ------------------------------------------------------------------------------------------------------------------ loop
T_REV, S_REV = [999, 699, 339], [699, 339, 0]
PAIR = ["a cat sitting on a bench", "a dog sitting on a bench"]
PAIR_R = ["a cat sitting on a bench", "a fluffy cat sitting on a red bench"]


@pytest.fixture(scope="module")
def sdxl_small():
    """Reduced-width SDXL: three levels, transformer depths (1, 2, 10) as in the full model (140 Attention modules), head dim 64.
    68 x 68 latents: the smallest multiple of 4 whose first attention level (34 x 34 = 1156 queries) lies above 32^2 - its self-attention
    is neither stored nor materialised - while the second (17 x 17) is stored."""
    from invertible_cd_amd import generation_sdxl, p2p, synthetic, unet
    from invertible_cd_amd.pipelines import StableDiffusionXLPipeline
    from invertible_cd_amd.schedulers import DDIMScheduler
    from invertible_cd_amd.unet_config import SDXL
    from oracle import sched_ref, unet_ref
    cfg = SDXL.scaled((64, 128, 256), cross_dim=128, heads=(1, 2, 4))
    assert cfg.num_attention_layers == 140
    sd = {k: v.half().float() for k, v in synthetic.synthetic_state_dict(cfg, seed=31).items()}
    B, H = 2, 68
    inp = synthetic.synthetic_inputs(cfg, B, H, H, seed=31)
    lat, ctx = inp["latents"].half().float(), inp["context"].half().float()
    added = {"text_embeds": inp["text_embeds"].half().float(), "time_ids": inp["time_ids"]}
    u = unet.UNet2DConditionModel(cfg, sd, dtype=torch.float16)
    pipe = StableDiffusionXLPipeline(u, DDIMScheduler.sdxl())
    emb = lambda p, o, c: {"prompt_embeds": ctx.cuda().half(), "text_embeds": added["text_embeds"].cuda().half(),
                           "time_ids": added["time_ids"].cuda()}
    ocfg = dict(unet_ref.SDXL)
    ocfg.update(block_out_channels=cfg.block_out_channels, cross_dim=cfg.cross_dim, num_heads=cfg.num_heads, add_in_dim=cfg.add_in_dim)
    p2p.tokenizer = synthetic.SyntheticTokenizer()
    p2p.NUM_DDIM_STEPS = 3
    p2p.LOW_RESOURCE = False
    yield dict(cfg=cfg, sd=sd, lat=lat, ctx=ctx, added=added, pipe=pipe, emb=emb, ocfg=ocfg, X=generation_sdxl, p2p=p2p, S=sched_ref,
               U=unet_ref, B=B)
    p2p.register_attention_control(pipe, None)
    p2p.device = "cpu"


def _gpu_loop(E, controller, **kw):
    _, out = E["X"].sample_deterministic(E["pipe"], list(PAIR), latents=E["lat"].cuda().half(), num_inference_steps=3, guidance_scale=7.0,
                                         is_sdxl=True, timesteps=[339, 699, 999], compute_embeddings_fn=E["emb"], return_latent=True, **kw,
                                         **({} if controller is None else {"controller": controller}))
    return out


def _oracle_loop(E, controller):
    """_oracle_loop_xl of test_sampler_gpu.py (fp16 latents between steps) with the controller on the hook, on the whole batch."""
    S, U = E["S"], E["U"]
    ac = S.alphas_cumprod()
    alpha, sigma = np.sqrt(ac), np.sqrt(1 - ac)
    x, B = E["lat"].clone(), E["B"]
    wemb = torch.from_numpy(S.guidance_scale_embedding([7.0] * B, 512)).half().float()
    hook = lambda p, is_cross, place: controller.call_cond_only(p, is_cross, place)
    for t, s in zip(T_REV, S_REV):
        eps = U.unet_forward(E["sd"], E["ocfg"], x, t, E["ctx"], timestep_cond=wemb, added_cond=E["added"], hook=hook).half().float()
        x = torch.from_numpy(S.predicted_origin(eps.numpy(), [t] * B, [s] * B, x.numpy(), alpha, sigma)).half().float()
        x = controller.step_callback(x).half().float()
    return x


def _make(E, kind, dev):
    p2p = E["p2p"]
    p2p.device = dev
    try:
        if kind == "replace_blend":
            return p2p.make_controller(PAIR, True, 0.5, 0.5, blend_words=(("cat",), ("dog",)))
        if kind == "replace":
            return p2p.make_controller(PAIR, True, 0.5, 0.5)
        return p2p.make_controller(PAIR_R, False, {"default_": 0.6, "fluffy": (0.0, 0.4)}, 0.4)
    finally:
        p2p.device = "cpu"


@pytest.mark.parametrize("kind", ["replace_blend", "refine"])
def test_sdxl_edit_loop_against_the_oracle(sdxl_small, kind):
    """Two prompts, 3 steps, accurate level: AttentionReplace with LocalBlend, AttentionRefine.  The north star's bar, as on every SD1.5
    edit loop: final latents and EVERY tensor of controller.attention_store within rel-L2 < 1e-3 of the fp32 oracle driving the same
    controller class on the CPU.  Measured values: profiles/p2p_sdxl_loop.txt."""
    E = sdxl_small
    ctrl, ref_ctrl = _make(E, kind, "cuda"), _make(E, kind, "cpu")
    ref_ctrl.num_att_layers = 140
    out = _gpu_loop(E, ctrl)
    assert ctrl.num_att_layers == 140 and ctrl.cur_step == 3 and ctrl.cur_att_layer == 0 and out.dtype == torch.float16
    assert E["pipe"].unet.attn_cond_only is False                       # the whole-batch layout is the sampler's, for its own calls
    ref = _oracle_loop(E, ref_ctrl)
    assert ref_ctrl.cur_step == 3
    e = rel_l2(out, ref)
    errs = []
    for key, refs in ref_ctrl.attention_store.items():
        assert len(ctrl.attention_store[key]) == len(refs), key
        for i, (g, r) in enumerate(zip(ctrl.attention_store[key], refs)):
            assert tuple(g.shape) == tuple(r.shape)
            errs.append((rel_l2(g, r), key, i, tuple(r.shape)))
    errs.sort(reverse=True)
    print(f"[sdxl {kind}] rel-L2(latents) = {e:.3e}; {len(errs)} store tensors, worst rel-L2 = {errs[0][0]:.3e}; top: " +
          ", ".join(f"{k}[{i}]{sh} {v:.2e}" for v, k, i, sh in errs[:4]))
    assert len(errs) == 120                                              # 60 self + 60 cross maps of the 17 x 17 levels (20 down, 10 mid, 30 up)
    if kind == "replace_blend":
        assert len(E["p2p"].LocalBlend.select_maps(ctrl.attention_store, out)[0]) == 50
        # the blend ran on the 50 maps and is no identity: past the mask the edited sample is pulled back to the source's latents.  (On
        # these synthetic weights the heat is nearly flat and the mask keeps all but a few latent cells - measured 100.0 % to one
        # decimal; masks with both sides well populated are what the op tests above check.)
        unblended = ref_ctrl.local_blend.blend(torch.stack([ref[0], ref[1] + 1.0]), ref_ctrl.attention_store)
        kept = (unblended[1] != ref[0]).float().mean().item()
        print(f"[sdxl {kind}] LocalBlend keeps {kept * 100:.1f} % of the edited sample's latent")
        assert 0.0 < kept < 1.0
    assert e < 1e-3
    for v, k, i, sh in errs:
        assert v < 1e-3, (k, i, sh, v)


def test_empty_control_is_the_unhooked_run_bit_for_bit_and_materialised_layers_skip_the_fused_launch(sdxl_small):
    """(a) A hooked run with EmptyControl (no layer materialised) equals the un-hooked run at the same precision level, bit for bit.
    (b) The fused to_q + cross-attention launch (option xattn_fusion = 1: wherever it is eligible) stands aside exactly on the layers whose
    probabilities are materialised - the executor's launch records: un-hooked, every eligible cross-attention layer takes it; with an
    AttentionStore, only those above 32^2 queries, which the store does not read; with an edit controller, which reads every
    cross-attention layer, none."""
    from invertible_cd_amd import _lib
    E = sdxl_small
    p2p, u = E["p2p"], E["pipe"].unet
    p2p.register_attention_control(E["pipe"], None)
    with u.editing():                                                    # the level a run with a controller selects
        plain = _gpu_loop(E, None)
    hooked = _gpu_loop(E, p2p.EmptyControl())
    assert torch.equal(plain, hooked)
    p2p.register_attention_control(E["pipe"], None)
    # 64 x 64 latents: 1024 / 256 rows per sample, the fused launch's tile divides both
    lat = E["lat"][:, :, :64, :64].contiguous().cuda().half()
    kw = dict(encoder_hidden_states=E["ctx"].cuda().half(), timestep_cond=torch.zeros(2, 512).cuda().half(),
              added_cond_kwargs={"text_embeds": E["added"]["text_embeds"].cuda().half(), "time_ids": E["added"]["time_ids"].cuda()})

    def launches(controller, latents):
        p2p.register_attention_control(E["pipe"], controller)
        u.attn_cond_only = controller is not None
        _lib.profile_enable(True)
        try:
            with u.editing():
                u(latents, 499, **kw)
            torch.cuda.synchronize()
            return _lib.profile_read().get("xattn_fused", {"launches": 0})["launches"]
        finally:
            _lib.profile_enable(False)
            u.attn_cond_only = False
            p2p.register_attention_control(E["pipe"], None)
    u.set_option("xattn_fusion", 1)
    try:
        n_plain = launches(None, lat)
        n_store = launches(p2p.AttentionStore(), lat)
        big = torch.cat([torch.cat([lat, lat], 2), torch.cat([lat, lat], 2)], 3)            # 128 x 128: level 1 at 4096 queries, not stored
        n_plain_big = launches(None, big)
        n_store_big = launches(p2p.AttentionStore(), big)
        n_edit_big = launches(_make(E, "replace", "cuda"), big)
    finally:
        u.set_option("xattn_fusion", 2)
    print(f"[sdxl fused cross-attention launches] 64^2: plain {n_plain}, store {n_store}; 128^2: plain {n_plain_big}, store {n_store_big}, "
          f"edit {n_edit_big}")
    assert n_plain == 70 and n_plain_big == 70
    assert n_store == 0                          # 64 x 64 latents: every cross-attention layer has <= 32^2 queries and is stored
    assert n_store_big == 10                     # 128 x 128: the ten 4096-query layers are not stored and keep the fused launch
    assert n_edit_big == 0
