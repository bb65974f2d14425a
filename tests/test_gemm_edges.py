"""CPU companion of test_gemm_edges_gpu.py: the case tables of the GEMM entry's edge tests (icd_gemm, csrc/gemm.hip and the big tiles), the
plan each case is meant to take (icd_gemm_plan is a pure host function), the per-element error bound the GPU tests assert - established
here on the reference alone - and the argument refusals of gemm_run, which all happen before any HIP call.

The bound.  ref = the fp64 result, S = |a| @ |w|^T * |alpha| + |bias| + |rowbias| + |resid| in fp64, u = 2^-23:
    fp16 output    |got - ref| <= 0.5 * fp16_ulp(ref) + (K + 8) * u * S
    fp32 output    |got - ref| <= (K + 8) * u * S + 2^-24 * |ref|
    carried output |decode(out, carry) - ref| <= 2^-3 * 0.5 * fp16_ulp(ref) + 2^-31 + (K + 8) * u * S
(K + 8) * u * S is the textbook forward error of a length-K fp32 dot product in ANY summation order (gamma_K <= K * u) plus the handful of
fp32 operations of the epilogue (alpha, bias, rowbias, residual, carry); the first term is the one rounding of the output.  u is a whole
fp32 ulp, not half of one, because whether the MFMA's internal additions round to nearest has not been measured.  The carry term: the
epilogue stores bf8_e5m2((v - fp16(v)) * 2^14) (carry_of8, gemm_common.h); e5m2 has a 3-bit significand, so round-to-nearest leaves at most
2^-3 of the rounding error |v - fp16(v)| <= 0.5 ulp - the constant gemm_common.h states - as long as the scaled carry is a normal e5m2
number; below 2^-14 the e5m2 spacing is 2^-16, i.e. at most 2^-17 * 2^-14 = 2^-31 in value units, which is the extra absolute term.
GEGLU (out = h * gelu(g)): with e_h, e_g the accumulation bounds of the two halves, gelu' <= 1.13 and the 6.4e-7 absolute error of the
polynomial (test_gelu_poly.py):  0.5 ulp + e_h * (|gelu(g)| + 6.4e-7) + (|h| + e_h) * (1.13 * e_g + 6.4e-7) + 2^-23 * |ref|.

What is asserted here: torch's own fp32 arithmetic (a.float() @ w.float().t(), and a sum over 64-wide k chunks as the kernels' k-tiles
add), with the epilogue in fp32 and one rounding, stays inside the bound for every dense case - with u = 2^-24 even, the ratios printed
below; the GPU tests assert the kernels against the same bound with u = 2^-23.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from test_norm_edges import fp16_ulp

from invertible_cd_amd import _lib

TOL = 1e-3
U = 2.0 ** -23
GELU_POLY_ABS = 6.4e-7
GELU_SLOPE = 1.13

NO_BIG = 0x200000
WM2, WM4 = 0x240000, 0x280000                      # ICD_GEMM_TUNE_NO_BIG | ICD_GEMM_TUNE_WM2 / WM4
FORCE_BIG = 0x100000
HEIGHTS = [(WM2, 128), (WM4, 256)]                 # (flags, tile_m) of the two 128-wide dense kernels


def big_cfg(i):
    return (i + 1) << 24                           # ICD_GEMM_TUNE_BIG_CFG(i)


# ============================================================================================================ 1. case tables
# A. tile edges of the 128-wide dense kernels: (M, N, K), every one on both heights, plain and with the full epilogue
TILE_CASES = [(1, 8, 8),            # one row, one 8-column group, one ragged k-tile of one chunk
              (127, 120, 56),       # one short of a tile in M, ragged N, ragged k-tile
              (128, 128, 64),       # exactly one 128 x 128 tile and one k-tile
              (129, 136, 72),       # one past: a second m-tile of one row, a second n-tile of one column group, a k-tail of one chunk
              (255, 128, 200),      # one short of the 256-row tile; 3 k-tiles + tail (the 3-stage ring wraps)
              (256, 264, 64),       # exactly one 256-row tile, three n-tiles
              (257, 136, 136),      # one past the 256-row tile; 2 k-tiles + tail
              (513, 136, 520)]      # three / five m-tiles, the last of one row; 8 k-tiles + tail
TILE_EXTRA = [(129, 136, 72), (257, 136, 136)]     # also fp32 out, fp32 residual, out_f32, carries, GEGLU and (B.) every stride at once
GEGLU_N = (128, 192)                               # GEGLU on the 128-wide kernels: one tile, one and a half tiles
EPI_RPS = 50                                       # rows per sample of the full epilogue: sample boundaries inside tiles, last sample partial
STRIDE_PAD = dict(lda=24, ldw=8, ldo=16, ldr=8, ld_rowbias=8)      # B. leading dimension minus width

# C. split-K, unforced, workspace attached: (M, N, K) -> (kernel, tile_m, tile_n, ksplit)
SPLIT_CASES = [((385, 392, 1032), (0, 128, 128, 2)),     # K tail (1032 = 16 * 64 + 8) in the last split, ragged M and N
               ((255, 256, 1024), (0, 128, 128, 2)),
               ((127, 128, 8192), (0, 128, 128, 8)),     # split depth only: the accumulation term dominates the bound here
               ((300, 1280, 2048), (0, 256, 128, 4))]    # the 256 x 128 tile, split
SPLIT_EXTRA = (385, 392, 1032)                     # also out_f32, carries, fp32 residual, ldo > N through splitk_reduce_kernel
SPLIT_WS_PINS = [((385, 392, 1032), 1.0, 2), ((385, 392, 1032), 0.5, 1), ((385, 392, 1032), 0.0, 1),
                 ((127, 128, 8192), 1.0, 8), ((127, 128, 8192), 0.5, 4)]       # (shape, fraction of the requested bytes, ksplit)

# D. transposed output on the 128-wide kernels: (B, rps, ldo), N in TRANS_N, K = TRANS_K
TRANS_CASES = [(3, 77, 80),         # scalar path from sample 1 on (77 % 8), vector + scalar tail in sample 0; 3 pad columns
               (3, 77, 104),        # 27 pad columns
               (2, 100, 104),       # rps % 8 == 4: the switch between the paths inside one 8-row group
               (5, 52, 56),         # sample boundaries inside a tile
               (2, 256, 256),       # vector path only, no pad
               (2, 256, 272),       # vector path, zero fill behind key + 8 == rps
               (3, 77, 78)]         # ldo % 8 != 0: the vector path is refused everywhere
TRANS_N, TRANS_K = (136, 264), 72
TRANS_BIG = [(dict(M=1024, N=1280, K=320, rps=256, ldo=256), 1),      # -> kernel
             (dict(M=1024, N=1280, K=320, rps=256, ldo=272), 0),      # pad columns: the 128-wide kernel's general epilogue
             (dict(M=1024, N=1280, K=320, rps=77, ldo=256), 0)]       # a 32-row tile would straddle samples

# E. batched mode through the descriptors of attention_scores / attention_apply
ATT_B, ATT_H, ATT_NK = 2, 3, 77
ATT_NQ, ATT_LD, ATT_D = (1, 129), (80, 96), (8, 40, 64, 72, 160)

# F. every big-tile configuration: (bm, bn, geglu_ok) of BIG_TILES in gemm_common.h
BIG_SHAPE = (257, 1280, 128)
BIG_TILES = [(256, 256, True), (256, 320, False), (192, 256, True), (128, 320, False), (256, 256, True), (256, 320, False), (192, 256, True)]
BIG_PAD = dict(lda=24, ldo=16, ldr=8)

# G. conv mode: (name, geometry, flags -> tile_m)
CONV_FAST = [dict(B=3, H=9, W=7, C0=64, C1=0, Co=136, stride=1), dict(B=3, H=9, W=7, C0=64, C1=0, Co=136, stride=2)]
CONV_GENERAL = dict(B=3, H=9, W=7, C0=24, C1=8, Co=40, stride=1)
CONV_PHASE = dict(B=2, H=5, W=6, C0=16, C1=0, Co=24)
PHASE_TAP_BASE = (0, 1, 3, 4)


# ==================================================================================================== descriptors and the plan
_DUMMY = (C.c_char * 64)()                           # a host address that is never dereferenced by icd_gemm_plan


def dummy():
    return C.addressof(_DUMMY)


def dense_desc(M, N, K, flags=0, **fields):
    """Dense descriptor with dummy non-null operand pointers; `fields` overrides anything."""
    d = _lib.GemmDesc()
    d.a0 = d.w = d.out = dummy()
    d.M, d.N, d.K, d.Nw = M, N, K, N
    d.lda, d.ldw, d.ldo = K, K, N
    d.mode, d.batch, d.zdiv, d.alpha, d.flags = 0, 1, 1, 1.0, flags
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def conv_out_hw(c):
    s = c.get("stride", 1)
    return (c["H"] + s - 1) // s, (c["W"] + s - 1) // s


def conv_desc(c, flags=0, tap_base=None, **fields):
    """The descriptor ops.conv3x3 builds for geometry `c` (3 x 3, pad 1; one phase of the phase form when tap_base is given)."""
    Ho, Wo = conv_out_hw(c)
    Cin = c["C0"] + c["C1"]
    d = _lib.GemmDesc()
    d.a0 = d.w = d.out = dummy()
    d.a1 = dummy() if c["C1"] else None
    d.M, d.N, d.Nw, d.K = c["B"] * Ho * Wo, c["Co"], c["Co"], (9 if tap_base is None else 4) * Cin
    if tap_base is not None:
        py, px = tap_base // 3, tap_base % 3
        d.conv_tap_base, d.conv_ktaps, d.out_remap_w, d.out_remap_c = tap_base, 4, c["W"], 2 * py * c["W"] + px
    d.lda, d.ldw, d.ldo, d.rows_per_sample = 0, d.K, c["Co"], Ho * Wo
    d.mode, d.C0, d.C1 = 1, c["C0"], c["C1"]
    d.Hin, d.Win, d.Hout, d.Wout, d.ksize, d.stride, d.upsample = c["H"], c["W"], Ho, Wo, 3, c.get("stride", 1), 0
    d.batch, d.zdiv, d.alpha, d.flags = 1, 1, 1.0, flags
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def scores_desc(Nq, d_head, ld, B=ATT_B, H=ATT_H, Nk=ATT_NK, ldq=None, ldk=None, k_rows=None, **fields):
    """ops.attention_scores: S[b*H + h] = scale * q_h k_h^T, fp32 [B*H, Nq, ld], Nw = Nk < N = ld."""
    ldq, ldk, k_rows = ldq or H * d_head, ldk or H * d_head, k_rows or Nk
    return dense_desc(Nq, ld, d_head, _lib.ICD_GEMM_OUT_F32, Nw=Nk, lda=ldq, ldw=ldk, ldo=ld, batch=B * H, zdiv=H,
                      a_bs0=Nq * ldq, a_bs1=d_head, w_bs0=k_rows * ldk, w_bs1=d_head, o_bs0=H * Nq * ld, o_bs1=Nq * ld, alpha=d_head ** -0.5, **fields)


def apply_desc(Nq, d_head, ld, B=ATT_B, H=ATT_H, ldvt=None, ldo=None, **fields):
    """ops.attention_apply: out[b, n, h*d:(h+1)*d] = P[b*H + h] V_h, P [B*H, Nq, ld], vt [B, H*d, ldvt]."""
    ldvt, ldo = ldvt or ld, ldo or H * d_head
    kw = dict(Nw=d_head, lda=ld, ldw=ldvt, ldo=ldo, batch=B * H, zdiv=H, a_bs0=H * Nq * ld, a_bs1=Nq * ld, w_bs0=H * d_head * ldvt,
              w_bs1=d_head * ldvt, o_bs0=Nq * ldo, o_bs1=d_head)
    kw.update(fields)
    return dense_desc(Nq, d_head, ld, 0, **kw)


def plan(d):
    info = _lib.GemmPlanInfo()
    _lib.check(_lib.load().icd_gemm_plan(C.byref(d), C.byref(info)), "icd_gemm_plan")
    return info.kernel, info.tile_m, info.tile_n, info.ksplit


def ws_bytes(M, N, K):
    return int(_lib.load().icd_gemm_workspace_bytes(M, N, K))


# ============================================================================================== shared inputs, reference, bound
def r16(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).half()


def gemm_inputs(M, N, K, rps=EPI_RPS, seed=500):
    """fp16 a [M, K], w [N, K] (scaled so that a row of the product has unit variance), fp32 bias, fp16 residual and rowbias."""
    return dict(a=r16(M, K, seed=seed), w=r16(N, K, seed=seed + 1, scale=K ** -0.5),
                bias=torch.randn(N, generator=torch.Generator().manual_seed(seed + 2)),
                resid=r16(M, N, seed=seed + 3), rowbias=r16((M + rps - 1) // rps, N, seed=seed + 4), rps=rps)


def ref64(a, w, alpha=1.0, bias=None, rowbias=None, rps=0, resid=None):
    """(ref, S) in fp64; resid may be fp16, fp32 or an already decoded carried tensor: its values are taken as they are."""
    ref = alpha * (a.double() @ w.double().t())
    S = abs(alpha) * (a.double().abs() @ w.double().abs().t())
    M = a.shape[0]
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    if rowbias is not None:
        rb = rowbias.double()[torch.arange(M) // rps]
        ref, S = ref + rb, S + rb.abs()
    if resid is not None:
        ref, S = ref + resid.double(), S + resid.double().abs()
    return ref, S


def acc_term(S, K):
    return (K + 8) * U * S


def bound_f16(ref, S, K):
    return 0.5 * fp16_ulp(ref) + acc_term(S, K)


def bound_f32(ref, S, K):
    return acc_term(S, K) + 2.0 ** -24 * ref.abs()


def bound_carry(ref, S, K):
    return 2.0 ** -3 * 0.5 * fp16_ulp(ref) + 2.0 ** -31 + acc_term(S, K)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def geglu_ref_bound(a, w, alpha, bias, K):
    """(ref, bound) of out = h * gelu(g), [h | g] = alpha * a w^T + bias with w / bias in the natural (un-interleaved) order."""
    full, S = ref64(a, w, alpha, bias)
    (h, g), (Sh, Sg) = full.chunk(2, -1), S.chunk(2, -1)
    eh, eg = acc_term(Sh, K), acc_term(Sg, K)
    ref = h * gelu64(g)
    bound = 0.5 * fp16_ulp(ref) + eh * (gelu64(g).abs() + GELU_POLY_ABS) + (h.abs() + eh) * (GELU_SLOPE * eg + GELU_POLY_ABS) + 2.0 ** -23 * ref.abs()
    return ref, bound


def conv_ref64(x, w, stride=1, bias=None):
    """x [B, Cin, H, W], w [Co, Cin, 3, 3] (any float dtype) -> token-major (ref, S) of the 3 x 3 pad-1 conv in fp64."""
    def nhwc(t):
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    ref = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), stride=stride, padding=1)
    S = F.conv2d(x.double().abs(), w.double().abs(), None if bias is None else bias.double().abs(), stride=stride, padding=1)
    return nhwc(ref), nhwc(S)


def phase_weight_3x3(wq, Cin, tap_base):
    """The phase's [Co, 4 * Cin] tap-major weights laid into a 3 x 3 kernel: iterated tap u is tap tap_base + (u & 1) + 3 (u >> 1)."""
    w3 = torch.zeros(wq.shape[0], Cin, 3, 3, dtype=wq.dtype)
    for u in range(4):
        t = tap_base + (u & 1) + 3 * (u >> 1)
        w3[:, :, t // 3, t % 3] = wq[:, u * Cin:(u + 1) * Cin]
    return w3


def worst(got, ref, bound):
    """(largest error / bound, its flat index); a zero bound admits only a zero error."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(ratio.flatten().argmax())
    return float(ratio.flatten()[i]), i


def chunked_fp32(a, w, chunk=64):
    """a w^T in fp32, summed over 64-wide k chunks one after the other (the order of the kernels' k-tiles)."""
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k0 in range(0, a.shape[1], chunk):
        acc = acc + a[:, k0:k0 + chunk].float() @ w[:, k0:k0 + chunk].float().t()
    return acc


# ===================================================================================================================== the tests
def test_planner_pins_the_128_wide_kernels_at_both_heights():
    for flags, tm in HEIGHTS:
        for M, N, K in TILE_CASES + [s for s, _ in SPLIT_CASES] + [BIG_SHAPE]:
            assert plan(dense_desc(M, N, K, flags)) == (0, tm, 128, 1), (M, N, K, hex(flags))
            full = dense_desc(M, N, K, flags, bias=dummy(), resid=dummy(), rowbias=dummy(), rows_per_sample=EPI_RPS, ldr=N, ld_rowbias=N,
                              splitk_ws=dummy(), splitk_ws_bytes=1 << 40)
            assert plan(full) == (0, tm, 128, 1)       # the forced heights never split, workspace or not
        for M, N, K in TILE_EXTRA:
            p = STRIDE_PAD
            d = dense_desc(M, N, K, flags, lda=K + p["lda"], ldw=K + p["ldw"], ldo=N + p["ldo"], ldr=N + p["ldr"], ld_rowbias=N + p["ld_rowbias"],
                           bias=dummy(), resid=dummy(), rowbias=dummy(), rows_per_sample=EPI_RPS)
            assert plan(d) == (0, tm, 128, 1)
            for n in GEGLU_N:
                assert plan(dense_desc(M, n, K, flags | _lib.ICD_GEMM_GEGLU, ldo=n // 2)) == (0, tm, 128, 1)
        for B, rps, ldo in TRANS_CASES:
            for N in TRANS_N:
                d = dense_desc(B * rps, N, TRANS_K, flags | _lib.ICD_GEMM_OUT_TRANS, rows_per_sample=rps, ldo=ldo)
                assert plan(d) == (0, tm, 128, 1)
        for c in CONV_FAST:
            assert plan(conv_desc(c, flags)) == (0, tm, 128, 1)


def test_planner_pins_split_k_and_what_the_workspace_does_to_it():
    for (M, N, K), want in SPLIT_CASES:
        need = ws_bytes(M, N, K)
        assert need >= want[3] * M * N * 4
        assert plan(dense_desc(M, N, K, splitk_ws=dummy(), splitk_ws_bytes=need)) == want, (M, N, K)
        assert plan(dense_desc(M, N, K, splitk_ws=dummy(), splitk_ws_bytes=need, ldo=N + 16)) == want
        # no workspace: never split (and 300 x 1280 x 2048 loses the 256-row tile with it: plan_gemm takes it for the split alone)
        assert plan(dense_desc(M, N, K)) == (0, 128, 128, 1)
        # the last split of a ragged K is not empty: ceil(nk / ksplit) k-tiles per split cover K with the tail in the last one
        nk = (K + 63) // 64
        per = (nk + want[3] - 1) // want[3]
        assert (want[3] - 1) * per < nk <= want[3] * per
    for (M, N, K), frac, ksplit in SPLIT_WS_PINS:
        nbytes = int(ws_bytes(M, N, K) * frac)
        d = dense_desc(M, N, K, splitk_ws=dummy() if nbytes else None, splitk_ws_bytes=nbytes)
        assert plan(d)[3] == ksplit, (M, N, K, frac)


def test_planner_pins_the_transposed_batched_big_and_conv_cases():
    for c, kernel in TRANS_BIG:
        d = dense_desc(c["M"], c["N"], c["K"], FORCE_BIG | _lib.ICD_GEMM_OUT_TRANS, rows_per_sample=c["rps"], ldo=c["ldo"])
        got = plan(d)
        assert got[0] == kernel and got[3] == 1 and (kernel == 1) == (got[2] >= 256), (c, got)
    for Nq in ATT_NQ:
        for ld in ATT_LD:
            for dh in ATT_D:
                assert plan(scores_desc(Nq, dh, ld)) == (0, 128, 128, 1)
                assert plan(apply_desc(Nq, dh, ld)) == (0, 128, 128, 1)
    M, N, K = BIG_SHAPE
    for i, (bm, bn, geglu_ok) in enumerate(BIG_TILES):
        p = BIG_PAD
        d = dense_desc(M, N, K, big_cfg(i), lda=K + p["lda"], ldo=N + p["ldo"], ldr=N + p["ldr"], bias=dummy(), resid=dummy(), rowbias=dummy(),
                       rows_per_sample=EPI_RPS, ld_rowbias=N)
        assert plan(d) == (1, bm, bn, 1), i
        g = dense_desc(M, N, K, big_cfg(i) | _lib.ICD_GEMM_GEGLU, ldo=N // 2 + 16)
        assert plan(g) == ((1, bm, bn, 1) if geglu_ok else (0, 128, 128, 1)), i     # no GEGLU epilogue: the 128-wide kernel
        if i in (0, 4):
            assert plan(dense_desc(M, N, K, big_cfg(i), out_carry=dummy(), ldo=N + 16)) == (1, bm, bn, 1)
            assert plan(dense_desc(M, N, K, big_cfg(i), out_f32=dummy(), ldo=N + 16)) == (1, bm, bn, 1)
    assert plan(conv_desc(CONV_GENERAL)) == (0, 128, 128, 1)
    assert plan(conv_desc(CONV_GENERAL, WM4)) == (0, 128, 128, 1)                # the general loader has one height
    for t0 in PHASE_TAP_BASE:
        assert plan(conv_desc(CONV_PHASE, tap_base=t0)) == (0, 128, 128, 1)


def _epilogue_fp32(acc, x, alpha, full):
    v = acc * torch.tensor(alpha, dtype=torch.float32)
    if full:
        M = acc.shape[0]
        v = v + x["bias"]
        v = v + x["rowbias"].float()[torch.arange(M) // x["rps"]]
        v = v + x["resid"].float()
    return v


@pytest.mark.parametrize("M,N,K", TILE_CASES + [s for s, _ in SPLIT_CASES] + [BIG_SHAPE])
def test_torch_fp32_stays_inside_the_bound(M, N, K):
    """The bound is a property of fp32 accumulation, not of the kernels: torch's fp32 product and a 64-wide chunked sum, with the epilogue
    in fp32 and one rounding, stay inside it - with u = 2^-24 (half of what the GPU tests allow).  Worst error / bound ratios at
    u = 2^-24, fp16 output, over both orders and both epilogues: 0.86 - 0.99 for K <= 200 (0.86 is the 8-element case), 0.86 at K = 520,
    0.70 at K = 1032 / 1024, 0.48 at K = 2048, 0.11 at K = 8192 - which is why the per-element cases keep K <= about 1032: there a
    4-ulp error of one element cannot hide under the accumulation term."""
    x = gemm_inputs(M, N, K)
    top = 0.0
    for full, alpha in ((False, 1.0), (True, 0.5)):
        ref, S = ref64(x["a"], x["w"], alpha, *((x["bias"], x["rowbias"], x["rps"], x["resid"]) if full else ()))
        half_u16 = 0.5 * fp16_ulp(ref) + 0.5 * acc_term(S, K)
        half_u32 = 0.5 * acc_term(S, K) + 2.0 ** -24 * ref.abs()
        for acc in (x["a"].float() @ x["w"].float().t(), chunked_fp32(x["a"], x["w"])):
            v = _epilogue_fp32(acc, x, alpha, full)
            r16_, _ = worst(v.half(), ref, half_u16)
            r32_, _ = worst(v, ref, half_u32)
            assert r16_ <= 1.0 and r32_ <= 1.0, (full, r16_, r32_)
            assert worst(v.half(), ref, bound_f16(ref, S, K))[0] <= 1.0 and worst(v, ref, bound_f32(ref, S, K))[0] <= 1.0
            assert rel_l2(v.half(), ref) < TOL
            top = max(top, r16_)
    print(f"[gemm-edges cpu {M}x{N}x{K}] torch fp32 worst error / bound (u = 2^-24, fp16 output) {top:.3f}")


def test_a_four_ulp_error_in_one_element_leaves_the_bound_but_not_the_norm():
    """What the per-element bound buys over rel-L2: four fp16 ulps on one element of 385 x 392 x 1032 move rel-L2 by 2e-4 (inside TOL)
    and are 3 to 4 times the bound; at K = 8192 the same error hides under the accumulation term."""
    for (M, N, K), caught in (((385, 392, 1032), True), ((127, 128, 8192), False)):
        x = gemm_inputs(M, N, K)
        ref, S = ref64(x["a"], x["w"])
        got = (x["a"].float() @ x["w"].float().t()).half()
        i = int(ref.abs().flatten().argmax())
        bad = got.clone()
        bad.view(-1)[i] = (got.view(-1)[i].double() + 4 * fp16_ulp(ref.flatten()[i])).half()
        assert rel_l2(bad, ref) < TOL
        assert (worst(bad, ref, bound_f16(ref, S, K))[0] > 1.0) == caught


def test_carry_constant_is_what_the_encoding_guarantees():
    """carry_encode is the host statement of carry_of8: the rounding error r = v - fp16(v) is below half an fp16 ulp H of v (or equal to
    it, and then exact), so it lies in the e5m2 binade under H, whose spacing is H / 4: what is left is at most H / 8 = 2^-3 |r| at the
    bottom of that binade, i.e. 2^-4 * H (plus 2^-31 where the scaled carry is an e5m2 subnormal).  The bound of the GPU tests says
    2^-3 * 0.5 * fp16_ulp(ref): the factor of two is for a result that lands in the binade above its reference's."""
    from invertible_cd_amd import ops
    v = torch.cat([torch.randn(20000, generator=torch.Generator().manual_seed(7)) * s for s in (1e-4, 1e-2, 1.0, 30.0)])
    hi, c = ops.carry_encode(v)
    err = (ops.carry_decode(hi, c).double() - v.double()).abs()
    assert bool((err <= 2.0 ** -4 * 0.5 * fp16_ulp(v.double()) + 2.0 ** -31).all())
    assert float((err / (0.5 * fp16_ulp(v.double()))).max()) > 2.0 ** -5          # and it is reached


def test_geglu_bound_holds_for_the_fp32_reference():
    from invertible_cd_amd import ops
    for M, _, K in TILE_EXTRA:
        for N in GEGLU_N:
            x = gemm_inputs(M, N, K, seed=520)
            ref, bound = geglu_ref_bound(x["a"], x["w"], 0.5, x["bias"], K)
            full = (x["a"].float() @ x["w"].float().t()) * 0.5 + x["bias"]
            h, g = full.chunk(2, -1)
            got = (h * F.gelu(g)).half()
            assert worst(got, ref, bound)[0] <= 1.0
            assert sorted(ops.geglu_perm(N // 2).tolist()) == list(range(N))


def test_attention_apply_refuses_head_dims_that_are_no_multiple_of_8():
    """attention_apply rounds N up to 8 columns while heads are d columns apart (o_bs1 = d): for d % 8 != 0 head h would write its pad
    columns into head h + 1's range from another block, and the last head past the row.  No model reaches it (every head dim in use is a
    multiple of 8); the front end refuses it before it builds a descriptor."""
    from invertible_cd_amd import ops
    p, vt = torch.zeros(2, 4, 8, dtype=torch.float16), torch.zeros(1, 24, 8, dtype=torch.float16)
    with pytest.raises(AssertionError, match="multiple of 8"):
        ops.attention_apply(p, vt, 1, 2, 4, 12)


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
TRANS, GEGLU, F32, RF32, LNC = _lib.ICD_GEMM_OUT_TRANS, _lib.ICD_GEMM_GEGLU, _lib.ICD_GEMM_OUT_F32, _lib.ICD_GEMM_RESID_F32, _lib.ICD_GEMM_LN_COMPUTE


def _dense(**kw):
    return dense_desc(128, 128, 64, kw.pop("flags", 0), **kw)


def _xattn(**kw):
    base = dict(rows_per_sample=256, xattn_k=dummy(), xattn_vt=dummy(), xattn_nk=77, xattn_ldk=128, xattn_ldvt=80, xattn_vt_bs=128 * 80,
                xattn_scale=0.125)
    base.update(kw)
    return dense_desc(base.pop("M", 256), base.pop("N", 128), 64, 0, **base)


_TINY = dict(B=1, H=4, W=4, C0=8, C1=0, Co=8)


def _conv(**kw):
    return conv_desc(_TINY, **kw)


def _phase(**kw):
    return conv_desc(_TINY, tap_base=kw.pop("tap_base", 0), **kw)


REFUSALS = [
    ("K % 8", lambda: dense_desc(128, 128, 60), "K and ldw must be multiples of 8"),
    ("N % 8", lambda: dense_desc(128, 100, 64), "N must be a multiple of 8"),
    ("ldw % 8", lambda: _dense(ldw=68), "K and ldw must be multiples of 8"),
    ("lda % 8", lambda: _dense(lda=68), "lda must be a multiple of 8"),
    ("mode 2", lambda: _dense(mode=2), "mode must be 0 (dense) or 1 (conv)"),
    ("trans + bias", lambda: _dense(flags=TRANS, rows_per_sample=64, bias=dummy()), "transposed output supports alpha"),
    ("trans + resid", lambda: _dense(flags=TRANS, rows_per_sample=64, resid=dummy(), ldr=128), "transposed output supports alpha"),
    ("trans + GEGLU", lambda: _dense(flags=TRANS | GEGLU, rows_per_sample=64), "transposed output supports alpha"),
    ("trans + fp32 output", lambda: _dense(flags=TRANS | F32, rows_per_sample=64), "transposed output supports alpha"),
    ("GEGLU N % 64", lambda: dense_desc(128, 136, 64, GEGLU), "GEGLU needs N % 64 == 0"),
    ("GEGLU + resid", lambda: _dense(flags=GEGLU, resid=dummy(), ldr=128), "GEGLU needs N % 64 == 0"),
    ("GEGLU + rowbias", lambda: _dense(flags=GEGLU, rowbias=dummy(), ld_rowbias=128, rows_per_sample=64), "GEGLU needs N % 64 == 0"),
    ("rowbias without rows_per_sample", lambda: _dense(rowbias=dummy(), ld_rowbias=128), "rows_per_sample required"),
    ("trans without rows_per_sample", lambda: _dense(flags=TRANS), "rows_per_sample required"),
    ("out_f32 + GEGLU", lambda: _dense(flags=GEGLU, out_f32=dummy()), "out_f32 (second fp32 output) goes with a plain fp16 output only"),
    ("out_f32 + trans", lambda: _dense(flags=TRANS, rows_per_sample=64, out_f32=dummy()), "out_f32 (second fp32 output)"),
    ("out_f32 + fp32 output", lambda: _dense(flags=F32, out_f32=dummy()), "out_f32 (second fp32 output)"),
    ("out_f32 batched", lambda: _dense(batch=2, out_f32=dummy()), "out_f32 (second fp32 output)"),
    ("out_carry + GEGLU", lambda: _dense(flags=GEGLU, out_carry=dummy()), "out_carry (error carry of the output) goes with a plain fp16 output only"),
    ("out_carry + trans", lambda: _dense(flags=TRANS, rows_per_sample=64, out_carry=dummy()), "out_carry (error carry of the output)"),
    ("out_carry + fp32 output", lambda: _dense(flags=F32, out_carry=dummy()), "out_carry (error carry of the output)"),
    ("out_carry batched", lambda: _dense(batch=2, out_carry=dummy()), "out_carry (error carry of the output)"),
    ("resid_carry without resid", lambda: _dense(resid_carry=dummy()), "resid_carry needs an fp16 resid"),
    ("resid_carry + fp32 resid", lambda: _dense(flags=RF32, resid=dummy(), ldr=128, resid_carry=dummy()), "resid_carry needs an fp16 resid"),
    ("resid_carry ldr % 8", lambda: _dense(resid=dummy(), ldr=132, resid_carry=dummy()), "carried tensors need leading dimensions"),
    ("ln_stats without ln_colsum", lambda: _dense(ln_stats=dummy()), "ln_stats and ln_colsum go together"),
    ("fused LayerNorm on a conv", lambda: _conv(ln_stats=dummy(), ln_colsum=dummy()), "fused LayerNorm applies to dense, unbatched, fp16-output"),
    ("fused LayerNorm batched", lambda: _dense(batch=2, ln_stats=dummy(), ln_colsum=dummy()), "fused LayerNorm applies to dense"),
    ("fused LayerNorm + fp32 output", lambda: _dense(flags=F32, ln_stats=dummy(), ln_colsum=dummy()), "fused LayerNorm applies to dense"),
    ("LN_COMPUTE without a buffer", lambda: _dense(flags=LNC), "ICD_GEMM_LN_COMPUTE needs the ln_stats buffer"),
    ("xattn N % 128", lambda: _xattn(N=192), "N % 128, K % 64 and 16-byte aligned leading dims"),
    ("xattn rows_per_sample % 256", lambda: _xattn(rows_per_sample=128), "rows_per_sample must be a multiple of 256"),
    ("xattn 97 keys", lambda: _xattn(xattn_nk=97, xattn_ldvt=104), "1..96 keys"),
    ("xattn ldvt < keys", lambda: _xattn(xattn_ldvt=72), "ldvt >= keys"),
    ("conv ksize 2", lambda: _conv(ksize=2), "conv ksize must be 1 or 3"),
    ("conv stride 3", lambda: _conv(stride=3), "conv stride must be 1 or 2"),
    ("conv upsample 2", lambda: _conv(upsample=2), "upsample must be 0 or 1"),
    ("conv K != taps * Cin", lambda: _conv(K=80), "K != taps*Cin"),
    ("conv a1 without C1", lambda: _conv(a1=dummy()), "a1/C1 mismatch"),
    ("conv C1 without a1", lambda: _conv(C1=8, K=144), "a1/C1 mismatch"),
    ("conv M % (Hout * Wout)", lambda: _conv(M=17), "bad conv geometry"),
    ("conv_tap_base 2", lambda: _phase(tap_base=2), "conv_tap_base must be 3 py + px"),
    ("out_remap_w != Wout", lambda: _phase(out_remap_w=5), "out_remap_w must equal Wout"),
]


def test_the_unmutated_descriptors_of_the_refusal_table_are_accepted():
    for d in (_dense(), _xattn(), _conv(), _phase(), _dense(flags=TRANS, rows_per_sample=64), _dense(flags=GEGLU)):
        plan(d)


@pytest.mark.parametrize("name,make,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_gemm_refuses(name, make, fragment):
    """Every refusal is made by the shared validation of icd_gemm and icd_gemm_plan before any HIP call; the plan entry is used so that a
    descriptor that slipped through could not launch on dummy pointers."""
    lib = _lib.load()
    info = _lib.GemmPlanInfo()
    d = make()
    assert lib.icd_gemm_plan(C.byref(d), C.byref(info)) == -1, name
    assert fragment.encode() in lib.icd_last_error(), (name, lib.icd_last_error())
