"""CPU companion of test_norm_edges_gpu.py: the arithmetic of the fp16 GroupNorm kernels (csrc/norm.hip) and of the elementwise activations
restated in torch, so that the bounds the GPU tests assert are established on the reference alone, on any machine.

  * gn_emulate: fp32 sums of x and x^2 in the kernels' order, mean = S / n, var = max(Q / n - mean^2, 0), rstd = rsqrt(var + eps),
    y = x * sc + sh with sc = rstd * gamma, sh = beta - mean * sc, one rounding to fp16.  `fma` picks the contracted form of the three
    multiply-adds (what hipcc emits by default) or the separately rounded one; the tests below hold for both.
  * the DC-offset bound (GPU test A4): the emulation stays under TOL / 2 up to |mean| / std = 32.
  * the zero-variance bound (GPU test A5): |y - beta| of a constant group, and a constant whose raw variance Q / n - mean^2 comes out
    NEGATIVE in fp32 - the case the fmaxf(..., 0.f) clamp exists for.
  * the activation bound (GPU test D): the fp32 formulas of elementwise.hip land within 2 fp16 ulps of the fp64 value on [-4, 4].
"""
import math

import torch
import torch.nn.functional as F

from conftest import rel_l2

TOL = 1e-3
GN_THREADS = 512


# ----------------------------------------------------------------------------------------------------- shared inputs and references
def gn_ref64(x, B, HW, groups, gamma, beta, eps, silu=False):
    """F.group_norm in fp64 of token-major x [B*HW, C] (any float dtype: the values are taken as they are)."""
    Cc = x.shape[-1]
    r = F.group_norm(x.double().reshape(B, HW, Cc).permute(0, 2, 1), groups, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    return (F.silu(r) if silu else r).reshape(B * HW, Cc)


def dc_offset_input(ratio, B, HW, Cc, std=0.5, seed=70):
    """fp16 [B*HW, C] with std 0.5 and mean = ratio * std."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B * HW, Cc, generator=g) * std + ratio * std).half()


def affine(Cc, seed=22):
    g = 1 + 0.1 * torch.randn(Cc, generator=torch.Generator().manual_seed(seed))
    b = 0.1 * torch.randn(Cc, generator=torch.Generator().manual_seed(seed + 1))
    return g, b


DC_SHAPES = [(2, 256, 64), (2, 2048, 64)]             # small-map kernel / streaming kernels, 32 groups
DC_RATIOS_BOUND, DC_RATIOS_REPORTED = (0, 8, 32), (64, 128, 256)


def zero_variance_input(B, HW, Cc, groups, const_group, value, seed=71):
    """Ordinary data with one group of every sample held at `value` (an fp16 number)."""
    x = (torch.randn(B, HW, Cc, generator=torch.Generator().manual_seed(seed)) * 1.5 + 0.3).half()
    cpg = Cc // groups
    x[:, :, const_group * cpg:(const_group + 1) * cpg] = value
    return x.reshape(B * HW, Cc)


ZV_SHAPE = dict(B=2, C=32, groups=4, const_group=1)   # cpg 8; HW = 100 (small-map kernel) and 1090 (streaming kernels)
ZV_HW = (100, 1090)
ZV_EXACT = 3.0          # sums of 3 and 9 are exact in fp32: the raw variance is exactly 0
# 20.03125: the sums round, and the raw variance comes out as -6.1e-4 in the small-map kernel's order (HW = 100) and -8.5e-4 in the
# streaming order (HW = 1090), in both arithmetic forms: far below -eps, so without the clamp rsqrt sees a negative number
ZV_NEGATIVE = 20.03125


def fp16_ulp(v):
    """Spacing of the fp16 numbers at |v| (fp64 tensor); the subnormal spacing 2^-24 below 2^-14."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def act_ref64(kind, x):
    x = x.double()
    if kind == 0:
        return x * torch.sigmoid(x)
    if kind == 1:
        return x * torch.sigmoid(1.702 * x)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def act_fp32(kind, x):
    """The formulas of activation_kernel (silu_f, quick-GELU, gelu_erf_f) evaluated in fp32."""
    x = x.float()
    if kind == 0:
        return x / (1.0 + torch.exp(-x))
    if kind == 1:
        return x / (1.0 + torch.exp(torch.tensor(-1.702) * x))
    return torch.tensor(0.5) * x * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752)))


def act_inputs(lim, n=8 * 300):
    return torch.linspace(-lim, lim, n).half()


# ----------------------------------------------------------------------------------------------------------------- the emulation
def gn_pix_per_split(B, HW, tgt=768):
    target = max(tgt // max(B, 1), 1)
    most = max(HW // 64, 1)
    nsplit = min(target, most)
    return (HW + nsplit - 1) // nsplit


def gn_takes_small_path(B, HW, Cc, groups):
    cpg = Cc // groups
    gpb = 1
    while (gpb * cpg) % 8:
        gpb *= 2
    cb = gpb * cpg
    if not (HW <= 1024 and B * HW * Cc <= 12 * 1024 * 1024 and groups % gpb == 0 and cb <= GN_THREADS):
        return False, gpb, cb
    rpi = GN_THREADS // (cb // 8)
    return (rpi * cb * 2 + cb * 2 + gpb * 2) * 4 <= 64 * 1024, gpb, cb


def _seq(t):
    """Left-to-right fp32 sum over the last dimension."""
    acc = torch.zeros(t.shape[:-1], dtype=torch.float32)
    for i in range(t.shape[-1]):
        acc = acc + t[..., i]
    return acc


def _thread(t):
    """gn_accumulate over the values a thread meets (last dimension): groups of four as (a + b) + (c + d), then one by one."""
    acc = torch.zeros(t.shape[:-1], dtype=torch.float32)
    k, i = t.shape[-1], 0
    while i + 3 < k:
        acc = acc + ((t[..., i] + t[..., i + 1]) + (t[..., i + 2] + t[..., i + 3]))
        i += 4
    while i < k:
        acc = acc + t[..., i]
        i += 1
    return acc


def _tree16(t):
    """group_sum<16> over the last dimension (16 lanes): xor 1, xor 2, half mirror, mirror - a pairwise tree."""
    for _ in range(4):
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def _rows(v, rpi):
    """[B, P, C] -> [B, C, rpi, K]: thread (row slot r, channel c) meets pixels r, r + rpi, ...  Pixels past P are zeros (x + 0 is
    exact; only where P is no multiple of rpi does the grouping of the last additions differ from the kernel's tail loop)."""
    B, P, Cc = v.shape
    K = (P + rpi - 1) // rpi
    pad = torch.zeros(B, K * rpi, Cc, dtype=torch.float32)
    pad[:, :P] = v
    return pad.reshape(B, K, rpi, Cc).permute(0, 3, 2, 1)


def gn_group_sums(x, B, HW, groups):
    """(S, Q, small) of every (sample, group): fp32 sums of x and x^2 in the order the kernels add them."""
    Cc = x.shape[-1]
    cpg = Cc // groups
    f = x.float().reshape(B, HW, Cc)
    small, gpb, cb = gn_takes_small_path(B, HW, Cc, groups)
    out = []
    for v in (f, f * f):
        if small:                                     # gn_small_kernel: row slots per channel, then the group's channels
            chan = _seq(_thread(_rows(v, GN_THREADS // (cb // 8))))                     # [B, C]
            out.append(_seq(chan.reshape(B, groups, cpg)))
        else:                                         # gn_stats_kernel per slab (row slot outer, channel inner), gn_finish_sums on top
            pps = gn_pix_per_split(B, HW)
            nsplit = (HW + pps - 1) // pps
            rpi = GN_THREADS // (Cc // 8)
            ws = []
            for sp in range(nsplit):
                part = _thread(_rows(v[:, sp * pps:min(HW, (sp + 1) * pps)], rpi))      # [B, C, rpi]
                part = part.reshape(B, groups, cpg, rpi).permute(0, 1, 3, 2).reshape(B, groups, rpi * cpg)
                ws.append(_seq(part))
            lanes = torch.zeros(B, groups, 16, (nsplit + 15) // 16, dtype=torch.float32)
            for sp in range(nsplit):
                lanes[:, :, sp % 16, sp // 16] = ws[sp]
            out.append(_tree16(_seq(lanes)))
    return out[0], out[1], small


def _fma(a, b, c):
    """fp32 fma: a * b is exact in fp64 (24 x 24 bits)."""
    return (a.double() * b.double() + c.double()).float()


def gn_raw_variance(S, Q, n, fma):
    mean = S / n
    qn = Q / n
    return mean, (_fma(-mean, mean, qn) if fma else qn - mean * mean)


def gn_emulate(x, B, HW, groups, gamma, beta, eps, fma=True, clamp=True):
    """The fp16 GroupNorm kernels' arithmetic on fp16 x [B*HW, C] -> fp16 [B*HW, C] (no SiLU)."""
    Cc = x.shape[-1]
    cpg = Cc // groups
    S, Q, _ = gn_group_sums(x, B, HW, groups)
    mean, var = gn_raw_variance(S, Q, torch.tensor(float(HW)) * torch.tensor(float(cpg)), fma)
    if clamp:
        var = var.clamp_min(0.0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    mean_c, rstd_c = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)         # [B, C]
    sc = rstd_c * gamma.float()
    sh = _fma(-mean_c, sc, beta.float().expand_as(sc)) if fma else beta.float() - mean_c * sc
    f = x.float().reshape(B, HW, Cc)
    y = _fma(f, sc[:, None, :].expand_as(f), sh[:, None, :].expand_as(f)) if fma else f * sc[:, None, :] + sh[:, None, :]
    return y.half().reshape(B * HW, Cc)


def zero_variance_bound(HW, value, eps):
    """4 x the largest |y - beta| the emulation gives on the constant group (both arithmetic forms)."""
    s = ZV_SHAPE
    x = zero_variance_input(s["B"], HW, s["C"], s["groups"], s["const_group"], value)
    g, b = affine(s["C"])
    cpg = s["C"] // s["groups"]
    cols = slice(s["const_group"] * cpg, (s["const_group"] + 1) * cpg)
    dev = 0.0
    for fma in (True, False):
        y = gn_emulate(x, s["B"], HW, s["groups"], g, b, eps, fma=fma)
        assert torch.isfinite(y).all()
        dev = max(dev, float((y[:, cols].double() - b[cols].double()).abs().max()))
    return 4.0 * dev


# ---------------------------------------------------------------------------------------------------------------------- the tests
def test_emulation_is_a_groupnorm():
    """Sanity of the restatement itself: on ordinary data it sits at the fp16 output rounding, on both dispatch paths."""
    for B, HW, Cc in DC_SHAPES:
        x = dc_offset_input(0.6, B, HW, Cc)
        g, b = affine(Cc)
        assert gn_takes_small_path(B, HW, Cc, 32)[0] == (HW <= 1024)
        for fma in (True, False):
            e = rel_l2(gn_emulate(x, B, HW, 32, g, b, 1e-5, fma=fma), gn_ref64(x, B, HW, 32, g, b, 1e-5))
            assert 1e-4 < e < 3e-4, e


def test_raw_sum_groupnorm_holds_half_the_tolerance_up_to_a_dc_offset_of_32_sigma():
    """GPU test A4 asserts rel-L2 < TOL at |mean| / std = 0, 8, 32: the kernels' arithmetic alone stays under TOL / 2 there (about 2.1e-4,
    2.1e-4 and 2.4e-4; the fp16 output rounding is 2.1e-4 of that), and leaves TOL between 64 and 128."""
    for B, HW, Cc in DC_SHAPES:
        g, b = affine(Cc)
        for ratio in DC_RATIOS_BOUND + DC_RATIOS_REPORTED:
            x = dc_offset_input(ratio, B, HW, Cc)
            ref = gn_ref64(x, B, HW, 32, g, b, 1e-5)
            es = [rel_l2(gn_emulate(x, B, HW, 32, g, b, 1e-5, fma=fma), ref) for fma in (True, False)]
            print(f"[GroupNorm emulation HW={HW} mean/std={ratio}] rel-L2 {es[0]:.3e} (contracted) {es[1]:.3e}")
            if ratio in DC_RATIOS_BOUND:
                assert max(es) < TOL / 2, (HW, ratio, es)
        assert max(es) > TOL / 2                       # at 256 the raw-sum form is visibly out: the limit DESIGN.md states is real


def test_zero_variance_group_comes_out_as_beta_and_the_clamp_is_what_keeps_it_finite():
    """GPU test A5.  Emulated max |y - beta| on the constant group (x 4 = the bound the GPU test asserts), the same at HW = 100 and 1090:
         value 3.0       1.17e-4 (eps 1e-5)   1.18e-4 (eps 1e-6)     the sums are exact, the raw variance is exactly 0
         value 20.03125  1.64e-4 (eps 1e-5)   9.35e-4 (eps 1e-6)     the raw variance is -6.1e-4 / -8.5e-4: the unclamped form is NaN
       (half an fp16 ulp of beta, up to 6e-5, plus the fp32 rounding of the shift beta - mean * sc at the size of mean * rstd)."""
    s = ZV_SHAPE
    cpg = s["C"] // s["groups"]
    for HW in ZV_HW:
        for eps in (1e-5, 1e-6):
            for value in (ZV_EXACT, ZV_NEGATIVE):
                bound = zero_variance_bound(HW, value, eps)
                print(f"[zero variance HW={HW} value={value} eps={eps}] emulated max |y - beta| = {bound / 4:.3e}")
                assert 0 < bound < (1e-3 if value == ZV_EXACT else 4e-2)
        x = zero_variance_input(s["B"], HW, s["C"], s["groups"], s["const_group"], ZV_EXACT)
        S, Q, _ = gn_group_sums(x, s["B"], HW, s["groups"])
        n = torch.tensor(float(HW * cpg))
        for fma in (True, False):
            assert float(gn_raw_variance(S, Q, n, fma)[1][:, s["const_group"]].abs().max()) == 0.0
    # the constant that needs the clamp, in both kernels' orders
    g, b = affine(s["C"])
    for HW in ZV_HW:
        x = zero_variance_input(s["B"], HW, s["C"], s["groups"], s["const_group"], ZV_NEGATIVE)
        S, Q, small = gn_group_sums(x, s["B"], HW, s["groups"])
        assert small == (HW <= 1024)
        for fma in (True, False):
            var = gn_raw_variance(S, Q, torch.tensor(float(HW * cpg)), fma)[1][:, s["const_group"]]
            print(f"[zero variance HW={HW} value={ZV_NEGATIVE}] raw variance {var.tolist()} ({'contracted' if fma else 'separate'})")
            assert float(var.max()) < -4e-5
            y = gn_emulate(x, s["B"], HW, s["groups"], g, b, 1e-5, fma=fma, clamp=False)
            assert not torch.isfinite(y).all()


def test_fp32_activation_formulas_land_within_two_fp16_ulps():
    """GPU test D asserts |activation - fp64| <= 2 fp16 ulps of the fp64 value on [-4, 4]: the fp32 evaluation of the same formulas, rounded
    to fp16, meets it (gelu_erf_f is the erf form, not the polynomial of test_gelu_poly.py; its 1 + erf(x / sqrt 2) cancels in the negative
    tail, which is what the second ulp is for), and meets TOL on [-12, 12]."""
    for kind in (0, 1, 2):
        x = act_inputs(4.0)
        ref = act_ref64(kind, x)
        got = act_fp32(kind, x).half().double()
        worst = float(((got - ref).abs() / fp16_ulp(ref)).max())
        print(f"[activation kind {kind}, fp32 formula] max error {worst:.2f} fp16 ulps on [-4, 4]")
        assert worst <= 2.0
        x = act_inputs(12.0)
        assert rel_l2(act_fp32(kind, x).half(), act_ref64(kind, x)) < TOL


def test_fp32_silu_error_that_bounds_the_split_activation():
    """GPU test D (icd_split2_act, act = 1) allows 4 x the rel-L2 error of torch's fp32 SiLU at its inputs: that error is an fp32
    rounding (a few 1e-8), i.e. the bound asks for fp32 accuracy of hi + lo, not fp16's."""
    x = split2_inputs()
    e = rel_l2(F.silu(x), F.silu(x.double()))
    print(f"[fp32 SiLU at the split2_act inputs] rel-L2 {e:.3e}")
    assert 0 < e < 1e-7


def split2_inputs(rows=3, Cc=20):
    return torch.randn(rows, Cc, generator=torch.Generator().manual_seed(90)) * 3.0
