"""icd_attention_wide (csrc/attention_wide.hip: flash attention at head dims 168 ... 512, the head dim split over the waves of a block)
against fp64 torch, judged per element with the bound test_attn_edges.py derives for the fused output (a function of d and Nk,
established there on the reference alone): worst error / bound <= 1.

Shapes are the smallest at which each part can go wrong: d in 168, 256, 264, 384, 392, 512 (a ragged last slice of 40 columns, one of 8,
exact slices, every NW = 2, 3, 4); Nk in 1, 63, 64, 65, 129 (no full tile, either side of a tile edge, two tiles and a ragged one); Nq in
1, 33, 64 (one row, a ragged second tile, two full tiles); B = 2 with H in 1, 2 (the head offset h d and the V^T batch stride).  Every
launch calls the C entry directly, under the guards of test_attn_edges_gpu.py.  Then: every stride non-minimal with NaN in the pad
columns of V^T, a running maximum that grows tile by tile, determinism, the memory the call allocates, and the VAE on both of its
arithmetic paths with a 192-channel mid-block."""
import pytest
import torch

from conftest import rel_l2
import test_attn_edges as cpu
import test_attn_edges_gpu as edges

pytestmark = pytest.mark.gpu
NAN = float("nan")


def launch_wide(q, k, v, H, d, scale, strided=False):
    """One icd_attention_wide launch under guards -> (out [B, Nq, H d] on the CPU, its bytes on the device).  strided: q and k are
    column slices of wider NaN-filled tensors, the output rows have 4 foreign columns between them, V^T is a block at row 24 of a taller
    buffer (vt_batch_stride > H d ldvt) with 64 pad columns beyond round8(Nk), and every pad column of V^T holds NaN."""
    L = edges._L()
    B, Nq, Cc = q.shape
    Nk = k.shape[1]
    qbuf, qv = edges.rows_slab(q, 16 if strided else 0)
    kbuf, kv = edges.rows_slab(k, 16 if strided else 0)
    ldvt = (Nk + 7) // 8 * 8 + (64 if strided else 0)
    vbuf, vv = edges.vt_block(v, H, d, ldvt, *((24, 8) if strided else (0, 0)), pad_value=NAN)
    obuf, ov = edges.out_slab(B * Nq, Cc, 4 if strided else 0)
    st = L.load().icd_attention_wide(qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), ov.data_ptr(), B, H, Nq, Nk, d, qbuf.stride(0), kbuf.stride(0),
                                     ldvt, obuf.stride(0), vbuf.stride(0) if strided else 0, scale, None)
    L.check(st, "icd_attention_wide")
    torch.cuda.synchronize()
    assert edges.guard_intact(obuf, ov), "the kernel wrote outside its output"
    return ov.cpu().reshape(B, Nq, Cc), ov.clone()


def judge(name, got, q, k, v, H, d):
    ref, bound = cpu.fused_ref_bound(q, k, v, H, d, d ** -0.5 * cpu.LOG2E, device="cuda")
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    ratio, i = cpu.worst(got, ref, bound)
    B, Nq, Cc = ref.shape
    b, rem = divmod(i, Nq * Cc)
    n, col = divmod(rem, Cc)
    assert ratio <= 1.0, (f"{name}: worst error / bound {ratio:.3f} at sample {b}, head {col // d}, query row {n}, column {col % d} "
                          f"(wave {col % d // 128}), {(k.shape[1] + 63) // 64} key tiles, {k.shape[1] % 64} keys in the last")
    assert rel_l2(got, ref) < cpu.TOL, name
    return ratio


@pytest.mark.parametrize("d", [168, 256, 264, 384, 392, 512])
def test_every_slice_shape_at_every_key_and_query_edge(d):
    ratios = []
    for H in (1, 2):
        for Nk in (1, 63, 64, 65, 129):
            for Nq in (1, 33, 64):
                q, k, v = cpu.attn_inputs(2, H, Nq, Nk, d)
                got, _ = launch_wide(q, k, v, H, d, d ** -0.5)
                ratios.append(judge(f"d={d} H={H} Nq={Nq} Nk={Nk}", got, q, k, v, H, d))
    print(f"[attn-wide] d={d}: worst error / bound {max(ratios):.3f} over {len(ratios)} launches")


@pytest.mark.parametrize("d", [168, 512])
def test_every_stride_non_minimal_and_nan_in_the_pad_columns_of_vt(d):
    q, k, v = cpu.attn_inputs(2, 2, 33, 65, d, seed=910)
    got, _ = launch_wide(q, k, v, 2, d, d ** -0.5, strided=True)
    r = judge(f"strided d={d}", got, q, k, v, 2, d)
    print(f"[attn-wide] strided d={d}: worst error / bound {r:.3f}")


@pytest.mark.parametrize("d", [264, 512])
def test_a_running_maximum_that_grows_tile_by_tile(d):
    """spread inputs: the row maximum of key tile t + 1 outgrows the running offset by more than 2^8 in most rows, so the rescale fires"""
    q, k, v = cpu.attn_inputs(2, 2, 33, 193, d, spread=True)
    got, _ = launch_wide(q, k, v, 2, d, d ** -0.5)
    r = judge(f"spread d={d}", got, q, k, v, 2, d)
    print(f"[attn-wide] spread d={d} Nk=193: worst error / bound {r:.3f}")


def test_the_same_call_twice_gives_the_same_bytes():
    from invertible_cd_amd import ops
    for d in (264, 512):
        q, k, v = (t.cuda() for t in cpu.attn_inputs(2, 2, 257, 449, d, seed=920))
        qm, km = q.reshape(-1, 2 * d), k.reshape(-1, 2 * d)
        vt = torch.zeros(2, 2 * d, 456, dtype=torch.float16, device="cuda")
        vt[:, :, :449] = v.transpose(1, 2)
        outs = [ops.attention_wide(qm, km, vt, 2, 2, 257, 449, d, d ** -0.5) for _ in range(3)]
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_n_8192_at_d_512_allocates_the_output_and_nothing_else():
    """B = 1, H = 1, N = 8192, d = 512: the materialised path holds 256 MiB of fp32 scores (and 128 MiB of probabilities); this call may
    grow the peak by its 8 MiB output plus the allocator's rounding (2 MiB blocks).  64 sampled rows against fp64 under the same bound."""
    from invertible_cd_amd import ops
    N, d = 8192, 512
    g = torch.Generator().manual_seed(930)
    q, k, v = (torch.randn(1, N, d, generator=g).half().cuda() for _ in range(3))
    vt = v.transpose(1, 2).contiguous()
    ops.attention_wide(q[0, :64], k[0, :64], vt[:, :, :64].contiguous(), 1, 1, 64, 64, d, d ** -0.5)       # (code object loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = ops.attention_wide(q[0], k[0], vt, 1, 1, N, N, d, d ** -0.5)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"[attn-wide] N=8192 d=512: peak memory grew by {grown / 2 ** 20:.2f} MiB (output {out.numel() * 2 / 2 ** 20:.0f} MiB)")
    assert out.shape == (N, d) and grown <= (8 + 2) << 20
    rows = torch.randperm(N, generator=g)[:64].sort().values
    ref, bound = cpu.fused_ref_bound(q[:, rows.cuda()], k, v, 1, d, d ** -0.5 * cpu.LOG2E, device="cuda")
    got = out[rows.cuda()].cpu()[None]
    ratio, i = cpu.worst(got, ref, bound)
    print(f"[attn-wide] N=8192 d=512: worst error / bound {ratio:.3f} over 64 sampled rows")
    assert torch.isfinite(out).all() and ratio <= 1.0, (ratio, int(rows[i // d]), i % d)


# ------------------------------------------------------------------------------------------------- the VAE with a 192-channel mid-block
WIDTHS = (32, 64, 192, 192)                         # 32 GroupNorm groups; the mid-block attention has one head of 192 channels
LATENT = (2, 4, 4, 12)                              # N = 48 mid-block tokens: one ragged key tile, a ragged second query tile


@pytest.fixture(scope="module")
def vae_case():
    """weights, inputs and the oracle's answers for both arithmetic paths, computed once (as tests/test_vae_gpu.py sets them up)"""
    from invertible_cd_amd import synthetic, vae
    from oracle import vae_ref
    z = torch.randn(*LATENT, generator=torch.Generator().manual_seed(5)) * 1.5
    x = torch.rand(2, 3, 32, 96, generator=torch.Generator().manual_seed(6)) * 2 - 1
    case = {}
    for path, base, obase, seed in (("fp16", vae.SD_VAE, vae_ref.SD_VAE, 3), ("fp32", vae.SDXL_VAE, vae_ref.SDXL_VAE, 13)):
        cfg, ocfg = base.scaled(WIDTHS), dict(obase, block_out_channels=WIDTHS)
        sd = synthetic.synthetic_vae_state_dict(cfg, seed=seed)
        zz, xx = z, x
        if path == "fp16":                          # fp16-representable weights and inputs, genuine fp32 ones on the fp32-fidelity path
            sd = {k: v.half().float() for k, v in sd.items()}
            zz, xx = z.half().float(), x.half().float()
        mom = vae_ref.encode_moments(sd, ocfg, xx)
        case[path] = dict(cfg=cfg, sd=sd, z=zz, x=xx, dec=vae_ref.decode(sd, ocfg, zz), mean=mom[:, :4], logvar=mom[:, 4:].clamp(-30, 20))
    return case


@pytest.mark.parametrize("fused", [True, False], ids=["wide", "materialised"])
@pytest.mark.parametrize("path", ["fp16", "fp32"])
def test_vae_with_a_192_channel_mid_block_stays_inside_the_bars_of_test_vae_gpu(vae_case, path, fused, monkeypatch):
    """decode and encode with fused_attention True (the wide kernel) and False (materialised scores), each inside the bar tests/test_vae_gpu.py
    holds that path to against oracle/vae_ref.py: rel-L2 < 1e-3 on the fp16 path, < 3e-4 on the fp32-fidelity path."""
    from invertible_cd_amd import _lib, ops, vae
    import ctypes as C
    c = vae_case[path]
    calls = []
    real = ops.attention_wide
    monkeypatch.setattr(ops, "attention_wide", lambda *a: (calls.append(a[3:8]), real(*a))[1])
    m = vae.AutoencoderKL(c["cfg"], c["sd"], fused_attention=fused)
    bar = 1e-3
    if path == "fp32":
        m, bar = m.to(torch.float32), 3e-4
    got = m.decode(c["z"].cuda())["sample"].float().cpu()
    dist = m.encode(c["x"].cuda()).latent_dist
    e_dec, e_mean, e_lv = rel_l2(got, c["dec"]), rel_l2(dist.mean.float().cpu(), c["mean"]), rel_l2(dist.logvar.float().cpu(), c["logvar"])
    print(f"[attn-wide vae {path} fused={fused}] decode rel-L2 = {e_dec:.3e}  encode mean = {e_mean:.3e}  logvar = {e_lv:.3e}")
    assert got.shape == c["dec"].shape == (2, 3, 32, 96) and dist.mean.shape == (2, 4, 4, 12)
    assert e_dec < bar and e_mean < bar and e_lv < bar
    # True reached the new entry, once per pass, with the mid-block's shape; False never did
    assert calls == ([(2, 1, 48, 48, 192)] * 2 if fused else [])
    query, info = _lib.AttentionQuery(3, 2, 1, 48, 48, 192, 0, 0, 0, 0), _lib.AttentionInfo()
    assert _lib.load().icd_attention_plan(C.byref(query), C.byref(info)) == 0 and (info.family, info.NW, info.grid_x) == (4, 2, 4)
