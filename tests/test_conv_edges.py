"""CPU companion of test_conv_edges_gpu.py: the case tables of the spatial kernels that do not go through icd_gemm (csrc/elementwise.hip:
icd_conv_in, icd_conv_out_n, icd_x0_step, icd_sinusoid / icd_sinusoid_f32; csrc/inception.hip: icd_conv2d, icd_pool3x3,
icd_global_avgpool), their fp64 references, the conditions on the inputs that make the comparisons mean what they say, and the argument
refusals of those entries, which all happen before any HIP call.

Two kinds of input for every convolution case.
  exact   activations are integers in [-3, 3] (sample 0 times 3), weights from {-1, -0.5, 0, 0.5, 1}, bias values multiples of 0.25.  Every
          product and every partial sum is then a multiple of 0.25 below 2^24 quarters, so fp32 accumulation in ANY order, with or without
          FMA, on the MFMA or on v_dot2, gives the fp64 value: an fp32 output must equal the reference cast to fp32, an fp16 output the
          reference rounded once to fp16.  The condition (sum |x| |w| + |bias| < 2^22, fp16 references below 65504) is asserted here for
          every case of the tables; it is what keeps the tests sharp at K = 9 * Cin up to 8352, where a per-element bound has lost its power.
  random  Gaussian activations (sample 0 times 50: a halo read into the neighbouring sample shows), weights of variance 2 / K, under the
          GEMM suite's bounds bound_f16 / bound_f32 (test_gemm_edges.py) with S = |x| * |w| + |bias|, K = kh * kw * Cin and u = 2^-23,
          at the same geometries restricted to K <= 1032.
The poolings, the global average and the boundary step are compared for equality with references that make the kernels' own roundings
(stated at each reference); the sinusoids against fp64 under a bound measured here on the fp32 expression itself.

test_wrong_outputs_are_rejected_and_the_first_passes_the_old_bar records why these files exist: a border element with one tap missing
passes a whole-tensor rel-L2 < 3e-4 and fails both comparers.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from test_norm_edges import fp16_ulp
from test_gemm_edges import bound_f16, bound_f32, worst

from invertible_cd_amd import _lib

FAKE = 0x1000                                        # a 16-byte aligned non-null address that a refused call never dereferences
K_RANDOM_MAX = 1032                                  # beyond it (K + 8) * u * S swamps the output rounding (test_gemm_edges.py)
F16_MAX = 65504.0
EXACT_LIMIT = 2.0 ** 22
OLD_BAR = 3e-4                                       # test_fid_gpu.py's rel-L2 bar for icd_conv2d
OLD_GEOM = (2, 16, 24)                               # (B, H, W) of the earlier conv_out tests; on the CPU only, no GPU case is this large

# ============================================================================================================ 1. case tables
# ---- icd_conv_out_n.  The dispatch (elementwise.hip, icd_conv_out_n), with nch = Cin / 8:
#   "if (Cin % 32 == 0 && Cin >= 256 && (size_t)Cin * 72 + 16 <= 64 * 1024)"  -> conv_out_mfma_kernel<TOut, 2, 5>   form "mfma"
#   "if (nch <= 8)"        -> conv_out_kernel<TOut, 8>      form "lpp8"     Cin   8 ..  64
#   "else if (nch <= 16)"  -> conv_out_kernel<TOut, 16>     form "lpp16"    Cin  72 .. 128
#   "else if (nch <= 32)"  -> conv_out_kernel<TOut, 32>     form "lpp32"    Cin 136 .. 248 (256 takes the matrix cores)
#   "else"                 -> conv_out_kernel<TOut, 64>     form "lpp64"    Cin 264 .. that are no multiple of 32, and everything past 896
# each with TOut = half_t and float ("if (out_is_f32)" on the same lines): every case below runs both.
CO_CIN = {8: "lpp8",          # one 8-channel chunk: 7 of the 8 lanes of a pixel idle
          64: "lpp8",         # the form's upper end: every lane one chunk
          72: "lpp16",        # lower end: 9 chunks on 16 lanes
          128: "lpp16",       # upper end (the VAE decoder's width)
          136: "lpp32",       # lower end
          248: "lpp32",       # upper end: 31 chunks, one lane idle
          256: "mfma",        # the matrix-core form at its lower bound; ncc = 8: the UN = 5 unroll ends on a ragged group of 3
          264: "lpp64",       # no multiple of 32: a full wave per pixel, 33 chunks
          288: "mfma",        # ncc = 9: groups of 5 and 4
          320: "mfma",        # ncc = 10: two even groups (the UNet's width)
          896: "mfma",        # the LDS ceiling: 896 * 72 + 16 = 64528 <= 65536
          928: "lpp64"}       # just past it (66832 bytes): back on the VALU form, 116 chunks on 64 lanes
CO_FORM_CIN = {"lpp8": 64, "lpp16": 72, "lpp32": 136, "lpp64": 264, "mfma": 256}       # the width every geometry is run at, per form
CO_GEOMS = [(1, 1, 1),        # one pixel: every tap but the centre is outside
            (1, 1, 5),        # height 1
            (1, 5, 1),        # width 1
            (3, 3, 5),        # 45 pixels: 16-pixel tiles that straddle two samples (15 | 30)
            (2, 4, 4),        # 32 pixels: two full tiles, one per sample
            (1, 1, 17),       # one pixel past a tile
            (3, 7, 9),        # 189 pixels: a second 128-pixel block, tiles that straddle samples at 63 and 126
            (1, 8, 16),       # 128 pixels: exactly one block
            (1, 3, 43)]       # 129 pixels: one past
CO_EVERY_CIN_GEOMS = [(3, 3, 5), (3, 7, 9)]           # the two geometries every Cin is run at


def conv_out_cases():
    """(Cin, (B, H, W)) without repetition: every Cin at two geometries, every geometry at one Cin per form."""
    cases = [(cin, g) for cin in CO_CIN for g in CO_EVERY_CIN_GEOMS]
    cases += [(cin, g) for cin in CO_FORM_CIN.values() for g in CO_GEOMS if (cin, g) not in cases]
    return cases


CO_VARIANTS = [(cout, f32, bias) for cout in (1, 2, 3, 4) for f32 in (False, True) for bias in (True, False)]

# ---- icd_conv_in: one thread per (pixel, 8 output channels); total threads = B * H * W * Cout / 8 against blocks of 256:
#   Cout 8: 1 / 12 / 12 / 105; Cout 24: 3 / 36 / 36 / 315 (one past 256); Cout 320: 40 / 480 / 480 (short of 512) / 4200 (past 4096)
CI_COUT = (8, 24, 320)
CI_GEOMS = [(1, 1, 1), (2, 1, 6), (2, 6, 1), (3, 5, 7)]
CI_VARIANTS = [(f32, bias) for f32 in (False, True) for bias in (True, False)]

# ---- icd_conv2d: (kh, kw, stride, ph, pw), (B, H, W), Cin, N.  M = B * Ho * Wo against the 128-row tile, N against the 64-column tile,
# K = kh * kw * Cin against the 32-wide K step.  Every case runs ldx = Cin and ldx = Cin + 24 and the four combinations of bias and ReLU.
C2D_CASES = [((1, 1, 1, 0, 0), (1, 1, 1), 8, 8),          # M = 1, one chunk of K (a quarter of a K step)
             ((1, 1, 1, 0, 0), (1, 1, 127), 24, 56),      # M = 127; K = 24: a ragged K step
             ((1, 1, 1, 0, 0), (2, 8, 8), 40, 64),        # M = 128 exactly, N = 64 exactly
             ((1, 1, 1, 0, 0), (3, 1, 43), 64, 72),       # M = 129: a second row tile of one pixel; N = 72: a second column tile of 8
             ((1, 1, 1, 0, 0), (1, 257, 1), 8, 136),      # M = 257: a third row tile of one pixel; three column tiles
             ((1, 1, 2, 0, 0), (3, 5, 6), 24, 8),         # stride 2 without padding, odd and even size
             ((1, 1, 2, 0, 0), (2, 16, 15), 40, 136),     # M = 128 from a strided walk
             ((3, 3, 2, 1, 1), (2, 8, 6), 24, 56),        # stride 2 with padding, even H and W; Cin = 24: a K step crosses a tap mid-chunk
             ((3, 3, 2, 1, 1), (3, 7, 9), 40, 72),        # ... odd H and W
             ((3, 3, 2, 1, 1), (2, 16, 16), 64, 64),      # M = 128
             ((3, 3, 1, 2, 0), (3, 3, 5), 24, 136),       # asymmetric padding at kernel - 1: rows of output that see one image row
             ((3, 3, 1, 2, 0), (3, 41, 3), 8, 8),         # M = 129 = 3 * 43 * 1
             ((3, 3, 1, 0, 2), (3, 5, 3), 40, 56),
             ((3, 3, 1, 0, 2), (1, 3, 125), 24, 64),      # M = 127
             ((3, 3, 1, 0, 2), (1, 3, 255), 8, 72),       # M = 257
             ((7, 7, 1, 3, 3), (3, 3, 4), 8, 136),        # a kernel larger than the unpadded image
             ((7, 7, 1, 3, 3), (2, 3, 4), 64, 8),         # K = 3136 (exact inputs only)
             ((15, 1, 1, 7, 0), (2, 9, 2), 64, 56),       # the tallest kernel on a 9 x 2 image
             ((1, 15, 1, 0, 7), (2, 2, 9), 24, 72),       # the widest on 2 x 9: a swapped kh / kw reads outside every row
             ((5, 5, 2, 2, 2), (3, 7, 10), 40, 64),       # K = 1000
             ((5, 5, 2, 2, 2), (2, 8, 7), 64, 136)]       # K = 1600 (exact inputs only)
C2D_LDX_PAD = (0, 24)
C2D_VARIANTS = [(bias, relu) for bias in (True, False) for relu in (True, False)]

# ---- icd_pool3x3: mode -> (B, H, W); C; ldx - C
POOL_GEOMS = {0: [(2, 3, 3), (2, 4, 4), (3, 7, 8)],                                  # ICD_POOL_MAX_S2: one window; one window, a row and column unused
              1: [(2, 1, 1), (2, 1, 5), (2, 5, 1), (2, 2, 2), (3, 7, 8)],            # ICD_POOL_MAX_S1P1: windows of 1, 2, 3, 4, 6 and 9 taps
              2: [(2, 1, 1), (2, 1, 5), (2, 5, 1), (2, 2, 2), (3, 7, 8)]}            # ICD_POOL_AVG_S1P1: counts 1, 2, 3, 4, 6, 9
POOL_C = (8, 24, 264)
POOL_LDX_PAD = (0, 16)

# ---- icd_global_avgpool
GAP_HW, GAP_C, GAP_B = (1, 7, 64, 1000), (8, 40, 2048), (1, 3)

# ---- icd_x0_step: dtype_flags bit 0: x fp32, bit 1: eps fp32, bit 2: out fp32.  B * per_sample against blocks of 256: 3 / 420 / 768 / 771
X0_FLAGS = tuple(range(8))
X0_PER_SAMPLE = (1, 140, 256, 257)
X0_COEF = [[0.6, 0.8, 0.9, 0.4358899],               # (alpha_t, sigma_t, alpha_s, sigma_s): an ordinary step
           [0.3117, 0.9502, 1.0, 0.0],               # the boundary step: s == 0
           [0.03, 0.99955, 0.5, 0.8660254]]          # alpha_t near 0.03: the division amplifies 33 times

# ---- icd_sinusoid / icd_sinusoid_f32: kind -> dims; n; values.  n * half against blocks of 256, e.g. dim 320: 160 / 480 / 800
SIN_DIMS = {0: (2, 6, 320), 1: (4, 7, 257, 512)}
SIN_N = (1, 3, 5)
SIN_VALS = {0: {1: [999.0], 3: [0.0, 19.0, 1024.0], 5: [0.0, 19.0, 779.0, 999.0, 1024.0]},
            1: {1: [19.0], 3: [0.0, 7.0, 19.0], 5: [0.0, 7.0, 19.0, 7.0, 0.0]}}
SIN_MARGIN = 4.0                                     # the device's expf / sinf / cosf are accurate to a few ulp, not correctly rounded


# ============================================================================================================ 2. inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def conv_inputs(kind, x_shape, w_shape, n_bias, K, seed):
    """(x, w, bias) in fp64 holding values the device types represent exactly (x fp16 - or fp32 for random conv_in input -, w fp16, bias
    fp32).  x_shape has the sample first; sample 0 is scaled by 3 (exact) or 50 (random)."""
    g = _gen(seed)
    if kind == "exact":
        x = torch.randint(-3, 4, x_shape, generator=g).double()
        x[0] *= 3.0
        w = torch.randint(-2, 3, w_shape, generator=g).double() / 2
        bias = torch.randint(-16, 17, (n_bias,), generator=g).double() / 4
    else:
        x = torch.randn(x_shape, generator=g)
        x[0] *= 50.0
        x = x.half().double()
        w = (torch.randn(w_shape, generator=g) * (2.0 / K) ** 0.5).half().double()
        bias = torch.randn(n_bias, generator=g).double()
    return x, w, bias


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- conv_out: x [B, H, W, Cin], w [4, 3, 3, Cin] (the kernel's layout), bias [4]
def conv_out_problem(kind, cin, geom):
    """x, w, bias and the fp64 (pre, S) of all four output channels WITHOUT bias, NCHW; variants slice and add the bias."""
    def make():
        B, H, W = geom
        x, w, bias = conv_inputs(kind, (B, H, W, cin), (4, 3, 3, cin), 4, 9 * cin, 1000 + cin * 7 + B * 100 + H * 10 + W)
        pre = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1)
        S = F.conv2d(x.abs().permute(0, 3, 1, 2), w.abs().permute(0, 3, 1, 2), padding=1)
        return dict(x=x, w=w, bias=bias, pre=pre, S=S, K=9 * cin)
    return _cached(("co", kind, cin, geom), make)


def conv_out_ref(p, cout, with_bias):
    ref, S = p["pre"][:, :cout], p["S"][:, :cout]
    if with_bias:
        b = p["bias"][:cout].reshape(1, cout, 1, 1)
        ref, S = ref + b, S + b.abs()
    return ref.contiguous(), S.contiguous()


# ---- conv_in: x [B, 4, H, W], w [Cout, 3, 3, 4], bias [Cout] -> token-major [B * H * W, Cout]
def conv_in_problem(kind, cout, geom, x_f32):
    def make():
        B, H, W = geom
        g = _gen(2000 + cout * 3 + B * 100 + H * 10 + W + int(x_f32))
        x, w, bias = conv_inputs(kind, (B, 4, H, W), (cout, 3, 3, 4), cout, 36, 2000 + cout * 3 + B * 100 + H * 10 + W)
        if kind == "random" and x_f32:               # an fp32 input that is no fp16 number
            x = torch.randn((B, 4, H, W), generator=g)
            x[0] *= 50.0
            x = x.double()
        pre = F.conv2d(x, w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(B * H * W, cout)
        S = F.conv2d(x.abs(), w.abs().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(B * H * W, cout)
        return dict(x=x, w=w, bias=bias, pre=pre, S=S, K=36)
    return _cached(("ci", kind, cout, geom, x_f32), make)


# ---- conv2d: x [B, H, W, Cin], w [N, kh, kw, Cin] (packed tap-major, channel-minor), bias [N] -> [M, N]
def conv2d_out_size(H, W, kh, kw, s, ph, pw):
    return (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1


def conv2d_problem(kind, i):
    def make():
        (kh, kw, s, ph, pw), (B, H, W), cin, n = C2D_CASES[i]
        K = kh * kw * cin
        x, w, bias = conv_inputs(kind, (B, H, W, cin), (n, kh, kw, cin), n, K, 3000 + i)
        pre = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=s, padding=(ph, pw))
        S = F.conv2d(x.abs().permute(0, 3, 1, 2), w.abs().permute(0, 3, 1, 2), stride=s, padding=(ph, pw))
        Ho, Wo = conv2d_out_size(H, W, kh, kw, s, ph, pw)
        assert tuple(pre.shape) == (B, n, Ho, Wo)
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(B * Ho * Wo, n).contiguous()        # noqa: E731
        return dict(x=x, w=w, bias=bias, pre=flat(pre), S=flat(S), K=K, M=B * Ho * Wo, Ho=Ho, Wo=Wo)
    return _cached(("c2d", kind, i), make)


def epilogue_ref(p, with_bias, relu=False):
    """(ref, S) of a token-major problem: + bias, max(0, .)."""
    ref, S = p["pre"], p["S"]
    if with_bias:
        ref, S = ref + p["bias"], S + p["bias"].abs()
    return (ref.clamp_min(0) if relu else ref), S


def conv_taps(x, w, s, ph, pw, Ho, Wo, decode=None, drop=None):
    """The convolution written out tap by tap in fp64 - x [B, H, W, Cin], w [N, kh, kw, Cin] -> [B, Ho, Wo, N] - so that it can be made
    wrong on purpose.  decode(t) -> (ky, kx) replaces the tap walk; drop = (b, yo, xo, n, t) leaves tap t out of one output element."""
    B, H, W, cin = x.shape
    n, kh, kw, _ = w.shape
    decode = decode or (lambda t: (t // kw, t % kw))
    out = torch.zeros(B, Ho, Wo, n, dtype=torch.float64)
    for t in range(kh * kw):
        ky, kx = decode(t)
        for yo in range(Ho):
            yi = yo * s - ph + ky
            if yi < 0 or yi >= H:
                continue
            for xo in range(Wo):
                xi = xo * s - pw + kx
                if xi < 0 or xi >= W:
                    continue
                c = x[:, yi, xi] @ w[:, t // kw, t % kw].t()
                if drop is not None and drop[1:3] == (yo, xo) and drop[4] == t:
                    c[drop[0], drop[3]] = 0.0
                out[:, yo, xo] += c
    return out


def exchange_halos(x, ph):
    """x [2, H, W, Cin] -> [2, H + 2 ph, W, Cin]: each sample between the rows of the OTHER sample that lie next to it in memory."""
    return torch.stack([torch.cat([x[1 - b][x.shape[1] - ph:], x[b], x[1 - b][:ph]]) for b in range(2)])


# ---- pooling
def pool_input(mode, geom, c):
    """fp16 values as fp64 [B, H, W, C]: all negative for the maxima (a zero-padded maximum would win), signed integers for the average
    (the window sum of at most 9 integers below 2^7 is exact in fp32 in any order)."""
    B, H, W = geom
    g = _gen(4000 + mode * 1000 + B * 100 + H * 10 + W + c)
    if mode == 2:
        x = torch.randint(-100, 101, (B, H, W, c), generator=g).double()
    else:
        x = (-torch.rand((B, H, W, c), generator=g) * 4 - 0.125).half().double()
        x[0] *= 64.0                                 # (a power of two: still fp16 numbers)
    return x


def pool_ref(mode, x):
    """-> fp16 [B * Ho * Wo, C].  Maxima: exact.  Average: the kernel's two roundings - the exact window sum divided by the count of taps
    inside the image in fp32 (a correctly rounded division), then rounded once to fp16."""
    nchw = x.permute(0, 3, 1, 2)
    if mode == 0:
        r = F.max_pool2d(nchw, 3, stride=2).half()
    elif mode == 1:
        r = F.max_pool2d(nchw, 3, stride=1, padding=1).half()
    else:
        total = F.avg_pool2d(nchw, 3, stride=1, padding=1, divisor_override=1)
        count = F.avg_pool2d(torch.ones_like(nchw), 3, stride=1, padding=1, divisor_override=1)
        assert torch.equal(total, total.round()) and float(total.abs().max()) < 2 ** 24
        r = (total.float() / count.float()).half()
    return r.permute(0, 2, 3, 1).reshape(-1, x.shape[-1]).contiguous()


def pool_cases():
    return [(mode, g, c) for mode, geoms in POOL_GEOMS.items() for g in geoms for c in POOL_C]


# ---- global average
def gap_input(B, HW, c):
    return (torch.randn((B, HW, c), generator=_gen(5000 + B + HW + c)) * 3).half()


def gap_ref(x):
    """The kernel's own two roundings: the fp64 sum - exact in any order: at most 1000 fp16 numbers, multiples of 2^-24 below 2^16, need
    50 bits - divided by HW in fp64, then cast to fp32."""
    return (x.double().sum(1) / float(x.shape[1])).float()


# ---- boundary step
def x0_inputs(flags, per_sample):
    B = len(X0_COEF)
    g = _gen(6000 + per_sample)
    x, eps = torch.randn((B, per_sample), generator=g) * 1.7, torch.randn((B, per_sample), generator=g)
    x = x if flags & 1 else x.half()
    eps = eps if flags & 2 else eps.half()
    return x, eps, torch.tensor(X0_COEF, dtype=torch.float32)


def x0_ref(x, eps, coef, flags):
    """The five fp32 torch operations, one at a time, on the inputs as the kernel sees them; one cast to the output type."""
    xv, ev = x.float(), eps.float()
    a_t, s_t, a_s, s_s = (coef[:, j:j + 1] for j in range(4))
    prod = s_t * ev
    diff = xv - prod
    x0 = diff / a_t
    p1 = a_s * x0
    p2 = s_s * ev
    out = p1 + p2
    return out if flags & 4 else out.half()


# ---- sinusoids
LN1E4 = math.log(10000.0)


def sinus_ref64(vals, dim, kind):
    """(out, angle) fp64 [n, dim]: the expression of elementwise.hip's header comment.  kind 0: [cos(t f_i) || sin(t f_i)],
    f_i = exp(-ln(1e4) i / half); kind 1: [sin(1000 w f_i) || cos(..)], f_i = exp(-ln(1e4) i / (half - 1)), an odd dim ends on a 0."""
    v = torch.tensor(vals, dtype=torch.float64)[:, None]
    half = dim // 2
    i = torch.arange(half, dtype=torch.float64)
    if kind == 0:
        a = v * torch.exp(-LN1E4 * i / half)
        out, ang = torch.cat([a.cos(), a.sin()], 1), torch.cat([a, a], 1)
    else:
        a = 1000.0 * v * torch.exp(-LN1E4 * i / (half - 1))
        out, ang = torch.cat([a.sin(), a.cos()], 1), torch.cat([a, a], 1)
        if dim & 1:
            z = torch.zeros(len(vals), 1, dtype=torch.float64)
            out, ang = torch.cat([out, z], 1), torch.cat([ang, z], 1)
    return out, ang


def sinus_fp32(vals, dim, kind, f32_entry):
    """sinusoid_kernel's expression, operation by operation, in torch fp32 (the fp32 entry takes exp in double and rounds it once)."""
    v = torch.tensor(vals, dtype=torch.float32)[:, None]
    half = dim // 2
    i = torch.arange(half, dtype=torch.float32)
    lg = torch.tensor(9.210340371976184, dtype=torch.float32)
    if kind == 0:
        arg = (-lg * i) / torch.tensor(float(half), dtype=torch.float32)
        f = torch.exp(arg.double()).float() if f32_entry else torch.exp(arg)
        a = v * f
        return torch.cat([a.cos(), a.sin()], 1)
    step = lg / torch.tensor(float(half - 1), dtype=torch.float32)
    f = torch.exp(i * -step)
    a = (v * torch.tensor(1000.0)) * f
    out = torch.cat([a.sin(), a.cos()], 1)
    return torch.cat([out, torch.zeros(len(vals), 1)], 1) if dim & 1 else out


def sinus_unit(angle):
    return angle.abs() * 2.0 ** -23 + 2.0 ** -24


def sinus_cases():
    return [(kind, dim, n) for kind, dims in SIN_DIMS.items() for dim in dims for n in SIN_N]


def sinus_cpu_figure(kind, f32_entry):
    """Worst |fp32 expression - fp64| in units of |angle| * 2^-23 + 2^-24 over the cases of `kind`."""
    def make():
        r = 0.0
        for k, dim, n in sinus_cases():
            if k == kind:
                ref, ang = sinus_ref64(SIN_VALS[k][n], dim, k)
                r = max(r, float(((sinus_fp32(SIN_VALS[k][n], dim, k, f32_entry).double() - ref).abs() / sinus_unit(ang)).max()))
        return r
    return _cached(("sin", kind, f32_entry), make)


def sinus_bound(ref, ang, kind, f32_entry):
    b = SIN_MARGIN * sinus_cpu_figure(kind, f32_entry) * sinus_unit(ang)
    return b if f32_entry else b + 0.5 * fp16_ulp(ref)


# ============================================================================================================ 3. comparers
def assert_exact(got, ref, what):
    """got (fp16 or fp32, on the CPU) equals the fp64 reference rounded once to got's type."""
    want = ref.to(got.dtype)
    if not torch.equal(got, want):
        bad = (got != want).flatten().nonzero().flatten()
        j = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, the first at flat index {j} "
                             f"{tuple(int(v) for v in torch.unravel_index(torch.tensor(j), got.shape))}: got {float(got.flatten()[j])}, "
                             f"want {float(want.flatten()[j])}")


def bound_of(f32, ref, S, K):
    return bound_f32(ref, S, K) if f32 else bound_f16(ref, S, K)


# ============================================================================================================ 4. the tests
def test_the_tables_hold_what_the_issue_names():
    cases = conv_out_cases()
    assert len(cases) == len(set(cases)) == 24 + 45 - 10          # (the five form widths at the two geometries of every width count once)
    for cin, form in CO_CIN.items():
        nch = cin // 8
        mfma = cin % 32 == 0 and cin >= 256 and cin * 72 + 16 <= 64 * 1024
        assert form == ("mfma" if mfma else "lpp8" if nch <= 8 else "lpp16" if nch <= 16 else "lpp32" if nch <= 32 else "lpp64"), cin
        assert sum(c == cin for c, _ in cases) >= 2
    assert {CO_CIN[c] for c in CO_FORM_CIN.values()} == set(CO_FORM_CIN) == set(CO_CIN.values())
    for g in CO_GEOMS:
        assert {CO_CIN[c] for c, gg in cases if gg == g} == set(CO_FORM_CIN), g
    assert sorted(B * H * W for B, H, W in CO_GEOMS) == [1, 5, 5, 17, 32, 45, 128, 129, 189]
    # every form meets a random case where K <= 1032 admits one: the 8- and 16-lane forms
    assert {CO_CIN[c] for c, _ in cases if 9 * c <= K_RANDOM_MAX} == {"lpp8", "lpp16"}
    ms = set()
    for i, ((kh, kw, s, ph, pw), (B, H, W), cin, n) in enumerate(C2D_CASES):
        Ho, Wo = conv2d_out_size(H, W, kh, kw, s, ph, pw)
        ms.add(B * Ho * Wo)
        assert ph < kh and pw < kw and H + 2 * ph >= kh and W + 2 * pw >= kw and B * Ho * Wo <= 257, i
    assert {1, 127, 128, 129, 257} <= ms
    assert {c[2] for c in C2D_CASES} == {8, 24, 40, 64} and {c[3] for c in C2D_CASES} == {8, 56, 64, 72, 136}
    assert {c[0] for c in C2D_CASES} == {(1, 1, 1, 0, 0), (1, 1, 2, 0, 0), (3, 3, 2, 1, 1), (3, 3, 1, 2, 0), (3, 3, 1, 0, 2), (7, 7, 1, 3, 3),
                                         (15, 1, 1, 7, 0), (1, 15, 1, 0, 7), (5, 5, 2, 2, 2)}
    assert any(c[0][0] > c[1][1] and c[0][1] > c[1][2] for c in C2D_CASES)              # a kernel larger than the unpadded image
    assert any(c[0][:3] == (3, 3, 2) and c[1][1] % 2 == 0 and c[1][2] % 2 == 0 for c in C2D_CASES)
    assert any(c[0][:3] == (3, 3, 2) and c[1][1] % 2 == 1 and c[1][2] % 2 == 1 for c in C2D_CASES)
    totals = sorted(B * H * W * (c // 8) for c in CI_COUT for B, H, W in CI_GEOMS)
    assert any(t < 256 for t in totals) and any(256 < t < 512 for t in totals) and any(4096 < t < 4352 for t in totals)


def test_exact_inputs_stay_exact_in_fp32_and_inside_fp16():
    """The condition on the inputs, for every case of the tables: sum |x| |w| + |bias| < 2^22 (all partial sums are multiples of 0.25:
    below 2^24 quarters, exact in fp32 in any order) and every reference below the largest fp16 number."""
    margins = {}

    def note(entry, S, ref):
        assert float(S.max()) < EXACT_LIMIT and float(ref.abs().max()) < F16_MAX, entry
        assert torch.equal(ref * 4, (ref * 4).round()), entry
        m = margins.setdefault(entry, [0.0, 0.0])
        m[0], m[1] = max(m[0], float(S.max())), max(m[1], float(ref.abs().max()))

    for cin, g in conv_out_cases():
        note("icd_conv_out_n", *conv_out_ref(conv_out_problem("exact", cin, g), 4, True)[::-1])
    for cout in CI_COUT:
        for g in CI_GEOMS:
            note("icd_conv_in", *epilogue_ref(conv_in_problem("exact", cout, g, False), True)[::-1])
    for i in range(len(C2D_CASES)):
        note("icd_conv2d", *epilogue_ref(conv2d_problem("exact", i), True)[::-1])
    for entry, (s, r) in margins.items():
        print(f"[conv-edges cpu] {entry}: largest sum |x||w| + |bias| = {s:.0f} = 2^22 / {EXACT_LIMIT / s:.0f}, largest |reference| = {r:.2f} "
              f"= 65504 / {F16_MAX / r:.0f}")


@pytest.mark.parametrize("i", range(len(C2D_CASES)))
def test_relu_cases_have_sums_the_clamp_changes(i):
    for kind in ("exact", "random"):
        if kind == "random" and conv2d_problem("exact", i)["K"] > K_RANDOM_MAX:
            continue
        p = conv2d_problem(kind, i)
        for with_bias in (True, False):
            ref, _ = epilogue_ref(p, with_bias)
            assert float((ref < 0).float().mean()) > 0.2, (i, kind, with_bias)
        if kind == "exact":                          # the tap-by-tap builder of the wrong outputs is the convolution when nothing is wrong
            (kh, kw, s, ph, pw), _, _, n = C2D_CASES[i]
            if p["M"] <= 64:
                assert torch.equal(conv_taps(p["x"], p["w"], s, ph, pw, p["Ho"], p["Wo"]).reshape(p["M"], n), p["pre"])


def test_torch_fp32_stays_inside_the_bounds_on_the_random_inputs():
    """The bound is a property of fp32 arithmetic: torch's own fp32 convolution, rounded once, stays inside it at every random case."""
    w_all = 0.0
    for i in range(len(C2D_CASES)):
        p = conv2d_problem("random", i)
        if p["K"] > K_RANDOM_MAX:
            continue
        (kh, kw, s, ph, pw), (B, H, W), cin, n = C2D_CASES[i]
        got = F.conv2d(p["x"].float().permute(0, 3, 1, 2), p["w"].float().permute(0, 3, 1, 2), p["bias"].float(), stride=s, padding=(ph, pw))
        got = got.permute(0, 2, 3, 1).reshape(p["M"], n).half()
        ref, S = epilogue_ref(p, True)
        r, _ = worst(got, ref, bound_f16(ref, S, p["K"]))
        w_all = max(w_all, r)
        assert r <= 1.0, i
    print(f"[conv-edges cpu] torch fp32 conv2d on the random inputs: worst error / bound {w_all:.3f}")


def test_wrong_outputs_are_rejected_and_the_first_passes_the_old_bar():
    """Three faults of the kind these kernels can have, built in plain torch: (1) one border element with one tap missing, (2) the two
    samples' halos exchanged (each sample's padding rows read from the neighbouring sample), (3) kh / kw swapped in the tap walk of a
    non-square kernel.  Equality on the exact inputs and worst > 1 on the random ones reject every one of them; the first one passes
    the whole-tensor rel-L2 < 3e-4 of the earlier tests, which is why they could not have seen it."""
    # ---- conv_out, Cin = 72: element (sample 1, channel 0, y 0, x 0) without its tap (ky, kx) = (1, 2), the pixel to the right - at the
    # table's (3, 7, 9) and, random inputs, at the 2 x 4 x 16 x 24 output of the earlier conv_out tests (test_ops_gpu.py), whose bar it passes
    # there (at the 756 elements of (3, 7, 9) one element in 252 of sample 1 weighs more: 6.7e-4, still under the suite's usual 1e-3)
    cin = 72
    for kind, geom in (("exact", (3, 7, 9)), ("random", (3, 7, 9)), ("random", OLD_GEOM)):
        p = conv_out_problem(kind, cin, geom)
        ref, S = conv_out_ref(p, 4, True)
        wrong = ref.clone()
        tap = float(p["x"][1, 0, 1] @ p["w"][0, 1, 2])
        assert tap != 0.0
        wrong[1, 0, 0, 0] -= tap
        e = rel_l2(wrong, ref)
        print(f"[conv-edges cpu] wrong output 1 (conv_out {kind} {geom}: a border element without one tap, {tap:+.4f}): rel-L2 {e:.2e}")
        if kind == "exact":
            for dt in (torch.float16, torch.float32):
                with pytest.raises(AssertionError, match="elements differ"):
                    assert_exact(wrong.to(dt), ref, "wrong 1")
        else:
            assert e < (OLD_BAR if geom == OLD_GEOM else 1e-3)          # the old bar lets it through
            for f32 in (False, True):
                got = wrong.float() if f32 else wrong.half()
                r, j = worst(got, ref, bound_of(f32, ref, S, p["K"]))
                assert r > 1.0 and j == ref[0].numel()           # (sample 1, channel 0, pixel 0)
                print(f"[conv-edges cpu]   rejected: error / bound {r:.1f} ({'fp32' if f32 else 'fp16'} output)")
    # ---- conv_out (2, 4, 4): the halos exchanged
    for kind, cin in (("exact", 256), ("random", 72)):
        p = conv_out_problem(kind, cin, (2, 4, 4))
        ref, S = conv_out_ref(p, 4, True)
        xh = exchange_halos(p["x"], 1)
        wrong = F.conv2d(xh.permute(0, 3, 1, 2), p["w"].permute(0, 3, 1, 2), p["bias"], padding=(0, 1))
        assert wrong.shape == ref.shape
        _report_rejected("2 (conv_out: halos exchanged)", kind, wrong, ref, S, p["K"])
    # ---- conv2d: halos exchanged at (3, 3, 2, 1, 1) on 2 x 8 x 6, kh / kw swapped at (1, 15, 1, 0, 7) on 2 x 2 x 9
    i_halo, i_swap = 7, 18
    assert C2D_CASES[i_halo][:2] == ((3, 3, 2, 1, 1), (2, 8, 6)) and C2D_CASES[i_swap][:2] == ((1, 15, 1, 0, 7), (2, 2, 9))
    for kind in ("exact", "random"):
        p = conv2d_problem(kind, i_halo)
        ref, S = epilogue_ref(p, True)
        (kh, kw, s, ph, pw), _, cin, n = C2D_CASES[i_halo]
        # (the top halo row only: with H even and stride 2 the bottom padding row is never read)
        wrong = F.conv2d(exchange_halos(p["x"], ph).permute(0, 3, 1, 2), p["w"].permute(0, 3, 1, 2), p["bias"], stride=s, padding=(0, pw))
        wrong = wrong[:, :, :p["Ho"]].permute(0, 2, 3, 1).reshape(p["M"], n)
        _report_rejected("2 (conv2d: halos exchanged)", kind, wrong, ref, S, p["K"])
        p = conv2d_problem(kind, i_swap)
        ref, S = epilogue_ref(p, True)
        (kh, kw, s, ph, pw), _, cin, n = C2D_CASES[i_swap]
        wrong = conv_taps(p["x"], p["w"], s, ph, pw, p["Ho"], p["Wo"], decode=lambda t: (t // kh, t % kh)).reshape(p["M"], n) + p["bias"]
        _report_rejected("3 (conv2d: kh / kw swapped)", kind, wrong, ref, S, p["K"])


def _report_rejected(name, kind, wrong, ref, S, K):
    if kind == "exact":
        with pytest.raises(AssertionError, match="elements differ"):
            assert_exact(wrong.half(), ref, name)
        print(f"[conv-edges cpu] wrong output {name}: rejected by equality on the exact inputs, {int((wrong.half() != ref.half()).sum())} "
              f"of {ref.numel()} elements differ")
    else:
        r, _ = worst(wrong.half(), ref, bound_f16(ref, S, K))
        print(f"[conv-edges cpu] wrong output {name}: rejected on the random inputs, error / bound {r:.1f}, rel-L2 {rel_l2(wrong, ref):.2e}")
        assert r > 1.0


def test_pool_and_average_references_meet_their_conditions():
    for mode, g, c in pool_cases():
        x = pool_input(mode, g, c)
        assert torch.equal(x.half().double(), x)
        if mode != 2:
            assert float(x.max()) < 0 and float(pool_ref(mode, x).max()) < 0
        else:
            assert torch.isfinite(pool_ref(mode, x)).all()
    x = gap_input(3, 1000, 40)
    assert torch.equal(gap_ref(x), (x.double().flip(1).sum(1) / 1000.0).float())         # the sum does not depend on the order


def test_boundary_step_reference_covers_the_boundary_and_the_steep_division():
    coef = torch.tensor(X0_COEF)
    assert float(coef[1, 2]) == 1.0 and float(coef[1, 3]) == 0.0 and 0.025 < float(coef[2, 0]) < 0.035
    assert len({tuple(r.tolist()) for r in coef}) == 3
    x, eps, coef = x0_inputs(0, 257)
    out = x0_ref(x, eps, coef, 4)
    ref64 = coef[:, 2:3].double() * ((x.double() - coef[:, 1:2].double() * eps.double()) / coef[:, 0:1].double()) + coef[:, 3:4].double() * eps.double()
    assert rel_l2(out, ref64) < 1e-6
    # rows exchanged: a wrong sample index in coef[b * 4 + ..] cannot pass
    assert not torch.equal(x0_ref(x, eps, coef[[1, 2, 0]], 4), out)


def test_sinusoid_fp32_expression_against_fp64():
    """The figure the GPU bound is built from: the kernel's expression in torch fp32 against fp64, in units of |angle| * 2^-23 + 2^-24.
    Measured: kind 0 3.283 for both entries (the correctly rounded exp of the fp32 entry does not help: the rounding of the exponent's
    fp32 ARGUMENT, up to 9.2, moves the frequency by several ulp), kind 1 4.208.  The GPU tests allow SIN_MARGIN = 4 times these."""
    for kind in (0, 1):
        for f32_entry in (False, True):
            r = sinus_cpu_figure(kind, f32_entry)
            print(f"[conv-edges cpu] sinusoid kind {kind}, {'fp32' if f32_entry else 'fp16'} entry: torch fp32 against fp64, worst "
                  f"{r:.3f} x (|angle| 2^-23 + 2^-24)")
            assert 0.25 < r < 16.0                   # an expression off by a term would show here, not only on the device
    for dim in (7, 257):
        ref, _ = sinus_ref64(SIN_VALS[1][3], dim, 1)
        assert torch.equal(ref[:, -1], torch.zeros(3, dtype=torch.float64))
        assert torch.equal(sinus_fp32(SIN_VALS[1][3], dim, 1, False)[:, -1], torch.zeros(3))
    ref, _ = sinus_ref64([0.0], 6, 0)
    assert torch.equal(ref, torch.tensor([[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]], dtype=torch.float64))


# ============================================================================================================ 5. refusals
def conv2d_c(x=FAKE, ldx=8, B=1, H=4, W=4, Cin=8, w=FAKE, N=8, kh=3, kw=3, stride=1, ph=1, pw=1, relu=0, out=FAKE, ldo=8, col_off=0):
    return _lib.load().icd_conv2d(C.c_void_p(x), ldx, B, H, W, Cin, C.c_void_p(w), None, N, kh, kw, stride, ph, pw, relu, C.c_void_p(out), ldo,
                                  col_off, None)


@pytest.mark.parametrize("kw,fragment", [
    (dict(ph=3), "padding must be in 0 .. kernel size - 1"),
    (dict(kw=3, pw=3), "padding must be in 0 .. kernel size - 1"),
    (dict(kh=7, ph=0, H=3), "does not fit the padded"),
    (dict(stride=3), "stride must be 1 or 2"),
    (dict(Cin=16, ldx=8), "ldx must be a multiple of 8, >= Cin"),
    (dict(x=FAKE + 8), "pointers must be 16-byte aligned"),
    (dict(out=FAKE + 2), "pointers must be 16-byte aligned"),
    (dict(N=16, ldo=16, col_off=8), "col_off + N <= ldo")])
def test_conv2d_refuses_before_any_launch(kw, fragment):
    lib = _lib.load()
    assert conv2d_c(**kw) == -1, kw
    assert fragment.encode() in lib.icd_last_error(), (kw, lib.icd_last_error())


def test_pool_conv_out_boundary_step_and_sinusoid_refuse_before_any_launch():
    lib = _lib.load()
    p = C.c_void_p

    def refused(status, fragment):
        assert status == -1 and fragment.encode() in lib.icd_last_error(), (fragment, lib.icd_last_error())

    refused(lib.icd_pool3x3(p(FAKE), 8, 1, 4, 4, 8, 1, p(FAKE), 8, 0, None), "in-place pooling is not supported")
    refused(lib.icd_pool3x3(p(FAKE), 8, 1, 2, 2, 8, 0, p(FAKE + 64), 8, 0, None), "is too small for this mode")
    for cout in (0, 5):
        refused(lib.icd_conv_out_n(p(FAKE), 1, 4, 4, 64, p(FAKE), None, cout, p(FAKE), 0, None), f"Cout must be 1..4 (got {cout})")
    refused(lib.icd_conv_out_n(p(FAKE), 1, 4, 4, 60, p(FAKE), None, 4, p(FAKE), 0, None), "icd_conv_out: bad shape")
    refused(lib.icd_x0_step(p(FAKE), p(FAKE), p(FAKE), 3, 16, 8, p(FAKE), None), "icd_x0_step: bad dtype flags")
    for entry, name in ((lib.icd_sinusoid, "icd_sinusoid"), (lib.icd_sinusoid_f32, "icd_sinusoid_f32")):
        refused(entry(p(FAKE), 3, 7, 0, p(FAKE), None), f"{name}: Timesteps dim must be even")
        # kind 1 at dim 2 and 3: half - 1 == 0, the frequency step would be ln(1e4) / 0 and every output NaN
        for dim in (2, 3):
            refused(entry(p(FAKE), 3, dim, 1, p(FAKE), None), f"{name}: the guidance embedding needs dim >= 4")
