"""Batched prompt-to-prompt editing on the MI355X: the grouped kernels (icd_p2p_cross_edit_groups, icd_local_blend_groups, the probability
epilogue with group_count) against the torch expressions and the single-group kernels, and G = 3 edits in one batch end to end against the
fp32 oracle of each pair alone."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

STORE_BAR = 1e-3


def _pack_random_operators(n, gen):
    from invertible_cd_amd import ops
    T = 77
    A = torch.rand(n, T, T, generator=gen) * (torch.rand(n, T, T, generator=gen) < 0.05)
    D = torch.rand(n, T, generator=gen)
    At, Dp = ops.p2p_pack_operator(A.cuda(), D.cuda())
    return A, D, At, Dp


def _probs(rows, nq, gen, nk=77, ld=80):
    buf = torch.zeros(rows, nq, ld, dtype=torch.float16)
    buf[:, :, :nk] = torch.softmax(torch.randn(rows, nq, nk, generator=gen) * 2.0, dim=-1).half()
    return buf.cuda()


@pytest.mark.parametrize("G,P", [(1, 2), (3, 2), (4, 3)])
def test_cross_edit_groups_matches_the_torch_expression_per_group(G, P):
    from invertible_cd_amd import ops
    gen = torch.Generator().manual_seed(G * 10 + P)
    H, nq = 4, 256
    A, D, At, Dp = _pack_random_operators(G * (P - 1), gen)
    buf = _probs(G * P * H, nq, gen)
    src = buf.clone()
    ops.p2p_cross_edit_groups(buf[:, :, :77], G, P, At, Dp)
    got = buf[:, :, :77].float().cpu()
    x = src[:, :, :77].float().cpu().reshape(G, P, H, nq, 77)
    Ah, Dh = At[:, :77, :77].float().cpu().transpose(1, 2), Dp[:, :77].float().cpu()          # the fp16 operator the kernel reads
    for g in range(G):
        base = x[g, 0]
        want = [base]
        for e in range(P - 1):
            j = g * (P - 1) + e
            want.append(base @ Ah[j] + Dh[j] * x[g, e + 1])
        want = torch.stack(want).reshape(P * H, nq, 77)
        rows = got[g * P * H:(g + 1) * P * H]
        assert torch.equal(rows[:H], want[:H])                                        # base rows untouched
        assert (rows - want).abs().max() < 2e-3, (g, float((rows - want).abs().max()))
    assert torch.equal(buf[:, :, 77:].cpu(), torch.zeros_like(buf[:, :, 77:].cpu()))   # pad columns stay zero
    if G == 1:
        one = src.clone()
        ops.p2p_cross_edit(one[:, :, :77], P, At, Dp)
        assert torch.equal(one, buf)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("what", ["store", "edit", "self"])
def test_grouped_probability_epilogue_matches_the_separate_passes_bit_for_bit(what, split):
    """Modelled on test_sampler_gpu.py::test_fused_probability_epilogue_matches_the_separate_passes_bit_for_bit, at the kernel level: the
    probabilities of a launch whose conditional samples are G = 3 groups of P = 2 (behind b0 = 2 unrelated samples), with the store
    accumulation / the grouped cross edit / the per-group self replacement in the epilogue, against the plain probability kernel followed by
    the separate passes (torch add, icd_p2p_cross_edit_groups, per-group row copies)."""
    from invertible_cd_amd import ops
    gen = torch.Generator().manual_seed(7)
    G, P, b0, H = 3, 2, 2, 5
    B = b0 + G * P
    cross = what == "edit"
    Nq, Nk, d = (256, 77, 64) if cross else (256, 256, 64)
    ld = 80 if cross else 256
    q = (torch.randn(B * Nq, H * d, generator=gen) * 0.4).half().cuda()
    k = (torch.randn(B * Nk, H * d, generator=gen) * 0.4).half().cuda()
    qc = kc = None
    if split:                                        # finite carries: the high byte of an fp16 (e5m2) below 2, either sign
        carry = lambda t: (torch.randint(0, 0x3c, t.shape, generator=gen) | (torch.randint(0, 2, t.shape, generator=gen) << 7)).to(torch.uint8).cuda()
        qc, kc = carry(q), carry(k)
    scale = d ** -0.5
    plain = ops.attention_probs(q, k, B, H, Nq, Nk, d, scale, ld=ld, q_carry=qc, k_carry=kc)
    kw = dict(ld=ld, q_carry=qc, k_carry=kc, first_cond_sample=b0, edit_count=P - 1, group_count=G)
    cond = slice(b0 * H, B * H)
    if what == "store":
        acc0 = (torch.rand((G * P * H, Nq, ld), generator=gen) * 3).half().cuda()
        acc = acc0.clone()
        fused = ops.attention_probs(q, k, B, H, Nq, Nk, d, scale, acc=acc, **kw)
        want = acc0.clone()
        want += plain[cond]
        assert torch.isfinite(plain).all() and torch.equal(fused, plain) and torch.equal(acc, want)
    elif what == "edit":
        _, _, At, Dp = _pack_random_operators(G * (P - 1), gen)
        fused = ops.attention_probs(q, k, B, H, Nq, Nk, d, scale, edit=(At, Dp), **kw)
        want = plain.clone()
        ops.p2p_cross_edit_groups(want[cond][:, :, :Nk], G, P, At, Dp)
        assert torch.equal(fused, want)
        assert not torch.equal(fused, plain)
    else:
        fused = ops.attention_probs(q, k, B, H, Nq, Nk, d, scale, self_from_base=True, **kw)
        want = plain.clone()
        for g in range(G):
            r0 = (b0 + g * P) * H
            for e in range(1, P):
                want[r0 + e * H:r0 + (e + 1) * H] = plain[r0:r0 + H]
        assert torch.equal(fused, want)
    torch.cuda.synchronize()


def test_grouped_epilogue_with_one_group_is_the_single_group_epilogue():
    from invertible_cd_amd import ops
    gen = torch.Generator().manual_seed(8)
    B, H, Nq, Nk, d = 3, 4, 256, 77, 40
    q = (torch.randn(B * Nq, H * d, generator=gen) * 0.4).half().cuda()
    k = (torch.randn(B * Nk, H * d, generator=gen) * 0.4).half().cuda()
    _, _, At, Dp = _pack_random_operators(B - 1, gen)
    acc = torch.rand((B * H, Nq, 80), generator=gen).half().cuda()
    outs = []
    for gc in (0, 1):
        a = acc.clone()
        p = ops.attention_probs(q, k, B, H, Nq, Nk, d, d ** -0.5, ld=80, acc=a, edit=(At, Dp), edit_count=B - 1, group_count=gc)
        outs.append((p, a))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_a_mismatched_group_count_is_refused_through_the_c_abi():
    from invertible_cd_amd import _lib
    lib = _lib.load()
    B, H, Nq, Nk, d = 6, 2, 64, 77, 40
    q = torch.zeros(B * Nq, H * d, dtype=torch.float16, device="cuda")
    k = torch.zeros(B * Nk, H * d, dtype=torch.float16, device="cuda")
    p = torch.zeros(B * H, Nq, 80, dtype=torch.float16, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(edit_count, group_count, first=0, self_from_base=1):
        e = _lib.ProbsEpilogue()
        e.first_cond_sample, e.self_from_base, e.edit_count, e.group_count = first, self_from_base, edit_count, group_count
        return lib.icd_attention_probs_ex(ptr(q), None, ptr(k), None, ptr(p), B, H, Nq, Nk, d, q.stride(0), k.stride(0), 80, 0.1,
                                          ctypes.byref(e), None)
    assert call(0, 2) == -1 and b"edit_count" in lib.icd_last_error()              # groups without edits
    assert call(1, 2) == -1 and b"groups" in lib.icd_last_error()                  # 6 samples are not 2 groups of 2
    assert call(1, 2, first=1) == -1                                               # 5 conditional samples
    assert call(2, 3) == -1                                                        # 3 groups of 3 != 6
    assert call(1, 3) == 0 and call(2, 2) == 0 and call(1, 2, first=2) == 0       # 3 x 2, 2 x 3, [2 unrelated | 2 x 2]
    torch.cuda.synchronize()


def _blend_inputs(G, P, gen, x_dtype=torch.float32):
    heads = [8, 8, 8, 8, 8]
    maps = [torch.softmax(torch.randn(G * P * h, 256, 77, generator=gen) * 3.0, dim=-1).half().cuda() for h in heads]
    alpha = torch.zeros(G * P, 77)
    sub = torch.zeros(G * P, 77)
    for r in range(G * P):
        alpha[r, 1 + r % 5] = 1
        alpha[r, 3 + r % 4] = 1
        sub[r, 6 + r % 3] = 1
    x = torch.randn(G * P, 4, 64, 64, generator=gen).to(x_dtype).cuda()
    return maps, alpha, sub, x


def _blend_torch(maps, alpha, sub, th, x, P):
    import torch.nn.functional as nnf
    m = torch.cat([t.float().reshape(P, -1, 1, 16, 16, 77) for t in maps], dim=1)

    def mask_of(al, use_pool, thr):
        heat = (m * al.reshape(P, 1, 1, 1, 1, 77).cuda()).sum(-1).mean(1)
        if use_pool:
            heat = nnf.max_pool2d(heat, kernel_size=3, stride=1, padding=1)
        heat = nnf.interpolate(heat, size=x.shape[2:])
        heat = heat / heat.amax(dim=(2, 3), keepdim=True)
        on = heat.gt(thr)
        return on[:1] + on
    mask = mask_of(alpha, True, th[0])
    if sub is not None:
        mask = mask * ~mask_of(sub, False, th[1])
    return mask


@pytest.mark.parametrize("x_dtype", [torch.float32, torch.float16])
def test_local_blend_groups_matches_the_torch_expression_per_group(x_dtype):
    from invertible_cd_amd import ops
    G, P = 4, 2
    gen = torch.Generator().manual_seed(9)
    maps, alpha, sub, x = _blend_inputs(G, P, gen, x_dtype)
    th_pool, th_sub = [0.3, 0.25, 0.35, 0.3], [0.3, 0.4, 0.3, 0.3]
    active, has_sub = [True, True, False, True], [True, False, True, False]
    out = ops.local_blend_groups(maps, alpha, (sub, has_sub), th_pool, th_sub, active, x, G)
    flips = 0
    for g in range(G):
        rows = slice(g * P, (g + 1) * P)
        xg = x[rows]
        if not active[g]:
            assert torch.equal(out[rows], xg.float())
            continue
        mg = [t[g * P * 8:(g + 1) * P * 8] for t in maps]
        mask = _blend_torch(mg, alpha[rows], sub[rows] if has_sub[g] else None, (th_pool[g], th_sub[g]), xg, P)
        base = xg[:1]
        want = base + mask.float() * (xg - base)
        diff = (out[rows] - want).abs()
        flips += int((diff > 1e-6).any(dim=1).sum())
        assert torch.allclose(out[rows], want, rtol=0, atol=1e-6), g
    assert flips == 0
    # one group is icd_local_blend, bit for bit
    one = ops.local_blend([t[:P * 8] for t in maps], alpha[:P], sub[:P], 0.3, 0.3, x[:P].contiguous())
    grp = ops.local_blend_groups([t[:P * 8] for t in maps], alpha[:P], (sub[:P], [True]), [0.3], [0.3], [True], x[:P].contiguous(), 1)
    assert torch.equal(one, grp)
    one = ops.local_blend([t[:P * 8] for t in maps], alpha[:P], None, 0.3, 0.3, x[:P].contiguous())
    grp = ops.local_blend_groups([t[:P * 8] for t in maps], alpha[:P], None, [0.3], [0.3], [True], x[:P].contiguous(), 1)
    assert torch.equal(one, grp)


# ------------------------------------------------------------------------------------------------ end to end
PAIRS = [["a cat sitting on a bench", "a dog sitting on a bench"],
         ["a red car on the road", "a red bus on the road"],
         ["a bird on a tree", "a crow on a tree"]]
SEEDS = [5, 6, 7]


def _make(p2p, g, device):
    p2p.device = device
    try:
        if g == 1:                                   # a Reweight chained on a Replace, the shipped amplify edit
            return p2p.make_controller(PAIRS[g], True, 0.3, 0.6, equilizer_params={"words": ("bus",), "values": (4.0,)})
        return p2p.make_controller(PAIRS[g], True, 0.5, 0.5 if g == 0 else 0.25)
    finally:
        p2p.device = "cpu"


@pytest.mark.parametrize("lora", [False, True])
def test_three_pairs_inverted_and_edited_in_one_batch(lora):
    """G = 3 pairs on the reduced SD1.5 of test_sd15_inversion_then_replace_edit: one batched consistency inversion (one seed per image)
    and one batched edit (ControllerBatch, dynamic guidance tau 0.8, gs 19).  Every group against the fp32 oracle of its pair alone
    with a reference-style controller (latents and every stored tensor < 1e-3 rel-L2), and against the same pair edited alone on the GPU."""
    from test_sampler_gpu import FWD_S, FWD_T, REV_S, REV_T, _env, _oracle_loop, _sd15_setup, _tables
    E = _env()
    p2p = E["p2p"]
    G, P = 3, 2
    cfg, sd, lat, ctx, model, solver = _sd15_setup(E, G * P, 32, 32, seed=31, lora=lora)
    alpha, sigma = _tables(E["sched_ref"])
    solver.latent2image = lambda z, return_type="np": np.zeros((1,))
    # ---- batched inversion of G images, one seed each; base prompts' contexts
    imgs, ctx_inv = lat[:G], ctx[0::P]
    solver.context = torch.cat([torch.zeros_like(ctx_inv), ctx_inv]).cuda().half()
    _, inv = solver.cons_inversion(imgs.cuda(), guidance_scale=0.0, w_embed_dim=512, seed=SEEDS)
    ref_inv = []
    for g in range(G):
        noise = torch.randn((1, *lat.shape[1:]), generator=torch.Generator().manual_seed(SEEDS[g]))
        x0 = float(alpha[19]) * imgs[g:g + 1] + float(sigma[19]) * noise
        ref_inv.append(_oracle_loop(E, sd, cfg, x0, ctx_inv[g:g + 1], list(zip(FWD_T, FWD_S)), [[0.0]] * 4))
        e = rel_l2(inv[0][g:g + 1], ref_inv[g])
        print(f"[batched inversion, lora={lora}] group {g}: rel-L2 = {e:.3e}")
        assert e < 1e-3
    # ---- batched edit from the oracle's inverted latents, each repeated for the P prompts of its group
    p2p.tokenizer = E["synthetic"].SyntheticTokenizer()
    p2p.NUM_DDIM_STEPS = 4
    start = torch.cat([r.expand(P, *r.shape[1:]) for r in ref_inv])
    batch = p2p.ControllerBatch([_make(p2p, g, "cuda") for g in range(G)])
    p2p.register_attention_control(model, batch)
    solver.context = torch.cat([torch.zeros_like(ctx), ctx]).cuda().half()
    solver.prompt_groups = (G, P)
    try:
        outs = solver.cons_generation(start.cuda(), guidance_scale=19.0, w_embed_dim=512, dynamic_guidance=True, tau1=0.8, tau2=0.8,
                                      controller=batch)
    finally:
        solver.prompt_groups = None
        p2p.register_attention_control(model, None)
    got = outs[-1].float().cpu()
    stores = [{k: [t.float().cpu() for t in v] for k, v in m.attention_store.items()} for m in batch.members]
    assert batch.cur_step == 4 and all(m.cur_step == 4 for m in batch.members)
    ws = [[0.0, 0.0]] + [[0.0, 19.0]] * 3           # per pair: the w vector of a lone CFG-doubled batch of 4
    for g in range(G):
        ref_ctrl = _make(p2p, g, "cpu")
        ref_ctrl.num_att_layers = 32
        ref = _oracle_loop(E, sd, cfg, start[g * P:(g + 1) * P].clone(), ctx[g * P:(g + 1) * P], list(zip(REV_T, REV_S)), ws,
                           controller=ref_ctrl)
        e = rel_l2(got[g * P:(g + 1) * P], ref)
        worst = max(rel_l2(a, b) for k in ref_ctrl.attention_store for a, b in zip(stores[g][k], ref_ctrl.attention_store[k]))
        print(f"[batched edit, lora={lora}] group {g}: latents rel-L2 = {e:.3e}, worst store tensor = {worst:.3e}")
        assert e < 1e-3 and worst < STORE_BAR
        assert sum(len(v) for v in ref_ctrl.attention_store.values()) == sum(len(v) for v in stores[g].values()) > 0
        # the same pair alone on the GPU
        alone = _make(p2p, g, "cuda")
        p2p.register_attention_control(model, alone)
        solver.context = torch.cat([torch.zeros_like(ctx[g * P:(g + 1) * P]), ctx[g * P:(g + 1) * P]]).cuda().half()
        try:
            o1 = solver.cons_generation(start[g * P:(g + 1) * P].cuda(), guidance_scale=19.0, w_embed_dim=512, dynamic_guidance=True,
                                        tau1=0.8, tau2=0.8, controller=alone)
        finally:
            p2p.register_attention_control(model, None)
        e1 = rel_l2(got[g * P:(g + 1) * P], o1[-1].float().cpu())
        w1 = max(rel_l2(a, b.float().cpu()) for k in alone.attention_store for a, b in zip(stores[g][k], alone.attention_store[k]))
        print(f"[batched edit, lora={lora}] group {g}: vs the pair alone on the GPU: latents {e1:.3e}, worst store tensor {w1:.3e}")
        assert e1 < 1e-3 and w1 < 1e-3
