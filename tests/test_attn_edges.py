"""CPU companion of test_attn_edges_gpu.py: the case tables of the attention entries' edge tests (icd_attention_fused_ex,
icd_attention_probs*, csrc/attention.hip), the instantiation each case is meant to take (a pure-Python copy of the host dispatch - written
when the dispatch was an `if` ladder and then pinned against its source text, unchanged since - held against what icd_attention_plan
answers), the per-element error bounds the GPU tests assert - established here on the reference alone - and the argument refusals of the
entries, which all happen before any HIP call.

The bounds.  u = 2^-23 (a whole fp32 ulp: neither the MFMA's internal rounding nor v_exp_f32's accuracy has been measured on this chip),
c = scale * log2(e) (1 for a prescaled q), A = max_j c * sum_i |q_i| |k_ji| over the keys the row may see (the size of a base-2 exponent's
operands), P = the fp64 softmax, ref = sum_j P_j v_j.

Fused output.  The kernels compute out = sum_j p~_j v_j / sum_j p~_j with p~_j = P_j (1 + delta_j) * (a common factor that cancels), so
    out - ref = sum_j P_j delta_j (v_j - ref) / (1 + sum_j P_j delta_j),        |delta_j| <= eps = 2^-11 + 2 ln2 (d + 4) u A + 4 u:
P rounded to fp16 (the SAME rounded value in numerator and denominator); the fp32 dot product of length d behind the exponent, whose
absolute error (d + 4) u A is a relative error ln2 (d + 4) u A of 2^x - twice, because the MODE 1 / 2 kernels carry the running offset M
(|M| <= A) through the same fp32 accumulation; the scale FMA and exp2 (4 u).  1 / (1 - eps) <= 1.01.  The two fp32 accumulations over Nk
keys (any order) and the final multiply by 1 / l add (Nk + 8) u relative to sum_j P_j |v_j| + |ref|, the output is rounded once:
    |got - ref| <= 0.5 fp16_ulp(ref) + 1.01 eps sum_j P_j |v_j - ref| + (Nk + 8) u (sum_j P_j |v_j| + |ref|) + Nk 2^-24 max_j |v_j - ref|.
The last term: lazy rescaling keeps the row maximum of the un-normalised P in [2^-1, 2^8] (the offset lags the maximum by at most 2^8; M
rounded to fp16 in MODE 1 can exceed it by less than 2^-1 ... in exponent units that is a factor below 2), so the row sum is >= 1/2,
and a P below fp16's normal range (2^-14) is rounded with an absolute error <= 2^-25, i.e. <= 2^-24 after normalisation, per key.

Probabilities.  got = fp16(2^(s - m) / l): the exponent's error as above (once: no offset in the accumulation, but the constant is kept),
the fp32 row sum of Nk terms and the multiply ((Nk + 8) u), scale and exp2 (4 u), one rounding, which below 2^-14 is absolute (2^-25):
    |got - P| <= 0.5 fp16_ulp(P) + (2 ln2 (d + 4) u A + (Nk + 8) u + 4 u) P + 2^-25.
Split operands (icd_attention_probs_split): q = qh + 2^-14 ql, k likewise; the reference is the fp64 softmax of the decoded operands
(ops.carry_decode), A is taken on them, and the exponent gains the dropped ql.kl term: + ln2 * c * 2^-28 max_j sum_i |ql_i| |kl_ji| in
the relative factor.

What is asserted here: a torch emulation of the kernels' arithmetic (fp32 scores, 64-key tiles, running maximum with the 2^8 lazy
rescale, P rounded to fp16, fp32 accumulation, one rounding of the output; exact two-sweep softmax for the probabilities) stays inside
the bounds for every row of every table with u = 2^-24 even - the ratios printed below - and four deliberately broken emulations leave
them.  The emulation runs a row's arithmetic, which does not depend on the batch: rows with thousands of heads are emulated on their
first two samples' first three heads.  The GPU tests assert the kernels against the same bounds with u = 2^-23.
"""
import ctypes as C
import math

import pytest
import torch

from conftest import rel_l2
from test_norm_edges import fp16_ulp

from invertible_cd_amd import _lib, ops

TOL = 2e-3                                         # the rel-L2 limit the attention tests of test_ops_gpu.py use
U = 2.0 ** -23
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
INF = float("inf")
CAUSAL, PRESC, MODE0 = 1, 2, 4                     # ICD_ATTN_CAUSAL, ICD_ATTN_Q_PRESCALED, ICD_ATTN_TUNE_MODE0


def cdiv(a, b):
    return (a + b - 1) // b


# ===================================================================================================== 2. the dispatch, in Python
def fused_dispatch(B, H, Nq, Nk, d, flags=0):
    """icd_attention_fused_ex's choice: (kernel, KS, DT, QT, MODE, DR, causal); kernel "tiled" (attn_fused_kernel) or "cross"
    (attn_cross_kernel, whose tiles per wave and STL cross_plan gives)."""
    causal, presc = bool(flags & CAUSAL), bool(flags & PRESC)
    fast = presc and not (flags & MODE0) and (not causal or d == 64)
    wide = cdiv(Nq, 256) * B * H >= 512 and Nk >= 256 and not causal
    if Nk > 64 and Nk <= 96 and d <= 64 and not causal and cdiv(Nq, 128) * B * H >= 2048:
        ks, dt = (2, 1) if d <= 32 else (3, 2) if d <= 48 else (4, 2)
        return ("cross", ks, dt, 1, 0, 0, False)
    if d <= 16:
        t = (1, 1, 1, 0, 0)
    elif d <= 32:
        t = (2, 1, 1, 0, 0)
    elif fast and d == 40 and wide:
        t = (3, 2, 2, 1, 3)
    elif fast and d == 40:
        t = (3, 2, 1, 1, 0)
    elif fast and d == 64:
        t = (4, 2, 1, 2, 0)
    elif fast and d == 80:
        t = (5, 3, 1, 2, 0)
    elif d <= 48:
        t = (3, 2, 2, 0, 0) if wide else (3, 2, 1, 0, 0)
    elif d <= 64:
        t = (4, 2, 1, 0, 0)
    elif d <= 80:
        t = (5, 3, 1, 0, 0)
    elif d <= 96:
        t = (6, 3, 1, 0, 0)
    elif d <= 128:
        t = (8, 4, 1, 0, 0)
    else:
        t = (10, 5, 1, 0, 0)
    return ("tiled",) + t + (causal,)


def cross_plan(B, H, Nq, Nk):
    """launch_attn_cross: (query tiles per wave, STL)."""
    tpw = 8
    while tpw > 1 and cdiv(Nq, 128 * tpw) * B * H < 1024:
        tpw >>= 1
    return tpw, (5 if Nk <= 80 else 6)


def probs_dispatch(d, ldp, split=False, epi=0):
    """attention_probs_run's choice: (KS, SPLIT, EPI, FEW); epi 0 none, 1 acc / self replacement, 2 the cross edit (few keys only)."""
    ks = 3 if d <= 48 else 5 if d <= 80 else 8 if d <= 128 else 10
    return (ks, split, epi, True if epi == 2 else ldp <= 96)


def masked_dispatch(Nk, d):
    """icd_attention_masked's choice: (NT, DT), 32-key tiles and 32-row tiles of the head dim."""
    tiles = lambda n: 1 if n <= 32 else 2 if n <= 64 else 3 if n <= 96 else 4
    return tiles(Nk), tiles(d)


def plan(entry, B, H, Nq, Nk, d, ldp=0, flags=0, split=False, epi=0):
    """icd_attention_plan (entry 0 fused, 1 probs, 2 masked): (status, icd_attention_info)"""
    query, info = _lib.AttentionQuery(entry, B, H, Nq, Nk, d, ldp, flags, int(split), epi), _lib.AttentionInfo()
    return _lib.load().icd_attention_plan(C.byref(query), C.byref(info)), info


def plan_fused(B, H, Nq, Nk, d, flags=0):
    """The library's answer in the mirror's terms: (what fused_dispatch returns, what cross_plan returns or None, info); the fields the
    mirror leaves out (OCC, NST, grid, LDS ring) are asserted here."""
    rc, i = plan(0, B, H, Nq, Nk, d, flags=flags)
    assert rc == 0 and i.variants == (22, 6)[i.family] and (i.grid_y, i.grid_z) == (1, 1)
    if i.family == 1:
        assert i.grid_x == cdiv(Nq, 128 * i.tiles_per_wave) * B * H and i.lds_bytes == 0
        return ("cross", i.KS, i.DT, 1, 0, 0, False), (i.tiles_per_wave, i.STL), i
    assert (i.OCC, i.NST) == (1 if i.KS == 10 else 2, 2) and i.grid_x == cdiv(Nq, 128 * i.QT) * B * H
    assert i.lds_bytes == i.NST * (64 * 32 * i.KS + (16 * i.DR if i.DR else 32 * i.DT) * 128)
    return ("tiled", i.KS, i.DT, i.QT, i.MODE, i.DR, bool(i.causal)), None, i


def plan_probs(r):
    rc, i = plan(1, r["B"], r["H"], r["Nq"], r["Nk"], r["d"], r["ldp"], split=r["split"], epi=r["epi"])
    assert rc == 0 and (i.family, i.variants) == (2, 40) and (i.grid_x, i.grid_y, i.grid_z, i.lds_bytes) == (cdiv(r["Nq"], 128), r["B"] * r["H"], 1, 0)
    return (i.KS, bool(i.SPLIT), i.EPI, bool(i.FEW)), i


def plan_masked(B, H, Nq, Nk, d):
    rc, i = plan(2, B, H, Nq, Nk, d)
    assert rc == 0 and (i.family, i.variants) == (3, 16) and (i.grid_x, i.grid_y, i.grid_z, i.lds_bytes) == (cdiv(Nq, 32), H, B, 0)
    return (i.NT, i.DT), i


# ============================================================================================================ 1. case tables
# (KS, DT) every head dim must take on the tiled kernel, written out (not computed): the boundary dims 16, 32, 48, 64, 80, 96, 128, 160
# and the dims strictly inside a branch, where only the `dd < d` guards keep head h off head h + 1's columns
KSDT = {8: (1, 1), 16: (1, 1), 24: (2, 1), 32: (2, 1), 40: (3, 2), 48: (3, 2), 56: (4, 2), 64: (4, 2), 72: (5, 3), 80: (5, 3),
        88: (6, 3), 96: (6, 3), 104: (8, 4), 120: (8, 4), 128: (8, 4), 136: (10, 5), 152: (10, 5), 160: (10, 5)}
FASTMODE = {40: 1, 64: 2, 80: 2}                   # head dims with a MODE 1 / MODE 2 kernel for a prescaled q


def _row(sec, B, H, Nq, Nk, d, flags, want, **kw):
    return dict(sec=sec, B=B, H=H, Nq=Nq, Nk=Nk, d=d, flags=flags, want=want, **kw)


def _tiled(d, mode=0, causal=False, qt=1, dr=0):
    return ("tiled",) + KSDT[d] + (qt, mode, dr, causal)


# A. head-dim sweep on the tiled kernel: Nq = 100 (a ragged query tile: wave 3 has 4 rows), Nk = 77 (one ragged key tile), H = 3;
#    plain (MODE 0), prescaled (MODE 1 at 40, MODE 2 at 64 / 80, the VALU form elsewhere), prescaled + ICD_ATTN_TUNE_MODE0
A_ROWS = [_row("A", 2, 3, 100, 77, d, f, _tiled(d, FASTMODE.get(d, 0) if f == PRESC else 0)) for d in KSDT for f in (0, PRESC, PRESC | MODE0)]

# B. key-count edges: one key; a chunk edge (7, 8); a full tile without a peel (64) and either side of it; odd and even full-tile counts
#    of the 2-stage ring (127, 128, 129: one / two full tiles, two + a one-key peel); leftover full tiles after the unrolled pair (192,
#    193).  Query counts: one row; a second wave of one row (33); a full block (128); a second block of one row (129).  Nk >= 65 runs on
#    `spread` data (key magnitudes growing per tile), so the lazy rescale fires after the first tile.
B_DIMS, B_NK, B_NQ = (40, 64, 96, 128, 160), (1, 7, 8, 63, 64, 65, 127, 128, 129, 192, 193), (1, 33, 128, 129)
B_ROWS = [_row("B", 2, 2, Nq, Nk, d, 0, _tiled(d), spread=Nk >= 65) for d in B_DIMS for Nk in B_NK for Nq in B_NQ]

# C. causal, one head dim per KS, and the MODE 2 causal kernel at 64: one row; exactly one tile (rag false: only CAUSAL masks); a ragged
#    tile; two full tiles; two + a two-key peel; three + a peel (the unrolled pair, a leftover, a peel)
C_DIMS, C_N = (16, 32, 40, 64, 80, 96, 128, 160), (1, 64, 77, 128, 130, 200)
C_ROWS = [_row("C", 2, 2, N, N, d, CAUSAL, _tiled(d, causal=True)) for d in C_DIMS for N in C_N] + \
         [_row("C", 2, 2, N, N, 64, CAUSAL | PRESC, _tiled(64, 2, causal=True)) for N in C_N]

# D. the wide kernels (two query tiles per wave): ceil(300 / 256) * 4 * 64 = 512 blocks, Nk = 256 (no peel) and 333 (peel); Nq = 300:
#    the second 256-row block holds 44 rows (wave 0 full + 12 rows of wave 1's first tile, every other tile query-less)
D_ROWS = [_row("D", 4, 64, 300, Nk, d, f, want) for Nk in (256, 333) for d, f, want in
          ((40, 0, _tiled(40, qt=2)), (48, 0, _tiled(48, qt=2)), (40, PRESC, _tiled(40, 1, qt=2, dr=3)))]

# E. attn_cross_kernel at small shapes (B * H = 2048): every (d, Nk) - all three <KS, DT> pairs with inside-branch dims, both STL (5 up to
#    80 keys, 6 above), 65 = one live key in the masked tile, 96 = no masked slot - with Nq cycling, and every (Nq, Nk) at d = 40.
#    want = (KS, DT), cross = (tiles per wave, STL): Nq <= 128 is one block per head (2048 blocks: 8 -> 4 -> 2 tiles per wave ... the loop
#    stops at 1024 blocks, so 8 stay), almost all tiles query-less
E_KSDT = {8: (2, 1), 24: (2, 1), 32: (2, 1), 40: (3, 2), 48: (3, 2), 56: (4, 2), 64: (4, 2)}
E_NQ, E_NK = (1, 100, 128, 129, 300), (65, 77, 80, 81, 96)
E_STL = {65: 5, 77: 5, 80: 5, 81: 6, 96: 6}
_e = [(d, Nk, E_NQ[(i + j) % 5]) for i, d in enumerate(E_KSDT) for j, Nk in enumerate(E_NK)]
_e += [(40, Nk, Nq) for Nk in E_NK for Nq in E_NQ if (40, Nk, Nq) not in _e]
E_ROWS = [_row("E", 32, 64, Nq, Nk, d, 0, ("cross",) + E_KSDT[d] + (1, 0, 0, False), cross=(8, E_STL[Nk])) for d, Nk, Nq in _e]

# F. strides, on one case per kernel family; `variants` of the GPU helper are applied one at a time and all at once
F_ROWS = [_row("F", 2, 3, 100, 77, 72, 0, _tiled(72)),                                   # tiled, QT = 1, inside-branch head dim
          _row("F", 4, 64, 300, 333, 40, PRESC, _tiled(40, 1, qt=2, dr=3)),              # wide (16-row P.V tiles)
          _row("F", 32, 64, 100, 77, 40, 0, ("cross", 3, 2, 1, 0, 0, False), cross=(8, 5)),      # cross
          _row("F", 2, 3, 130, 130, 64, CAUSAL, _tiled(64, causal=True)),                # causal
          _row("F", 2, 1, 100, 100, 160, 0, _tiled(160))]                                # H = 1, d = 160: the VAE's layout
F_VARIANTS = ("ldq", "ldk", "ldo", "ldvt8", "ldvt64", "vtbs")

# G. probabilities.  (Nk, ldp): one key; 3 pad columns; a pad of more than half a k-tile on the FEW side; no pad at the switch; one side
#    and the other of ldp <= 96; a whole k-tile of pad and more (77, 160); full tiles without pad (256, 256).  Every head dim runs one pair
#    on each side of the switch, in four forms: plain, split operands, acc (EPI 1), split + acc.
G_KS = {40: 3, 48: 3, 72: 5, 80: 5, 88: 8, 128: 8, 136: 10, 160: 10}
G_FEW = [(1, 8), (77, 80), (77, 96), (96, 96)]
G_MANY = [(77, 104), (97, 104), (129, 136), (256, 256), (77, 160)]
G_NQ = (1, 33, 127, 129)
G_ROWS = []
for _i, _d in enumerate(G_KS):
    for _few, (_nk, _ld) in ((True, G_FEW[_i % 4]), (False, G_MANY[_i % 5]), (False, G_MANY[(_i + 3) % 5])):
        for _j, (_split, _epi) in enumerate(((False, 0), (True, 0), (False, 1), (True, 1))):
            G_ROWS.append(dict(sec="G", B=3, H=2, Nq=G_NQ[(_i + _j) % 4], Nk=_nk, d=_d, ldp=_ld, split=_split, epi=_epi,
                               want=(G_KS[_d], _split, _epi, _few)))

# H. icd_attention_masked at full key counts under the same bound: one inside-branch head dim per branch of its dispatch
H_ROWS = [dict(sec="H", B=2, H=3, Nq=100, Nk=77, d=d) for d in (24, 56, 88, 120)]

FUSED_TABLES = dict(A=A_ROWS, B=B_ROWS, C=C_ROWS, D=D_ROWS, E=E_ROWS, F=F_ROWS)


# =============================================================================================== shared inputs, references, bounds
def attn_inputs(B, H, Nq, Nk, d, seed=900, spread=False):
    """fp16 q [B, Nq, H d], k, v [B, Nk, H d], different for every sample and head.  spread: q three times as large and the keys of tile t
    (1 + 1.5 t) times as large, so the row maximum of tile t + 1 outgrows the running offset by more than 2^8 in most rows."""
    g = torch.Generator().manual_seed(seed + 7 * d + Nk)
    q, k, v = (torch.randn(B, n, H * d, generator=g) for n in (Nq, Nk, Nk))
    if spread:
        q, k = q * 3.0, k * (1.0 + 1.5 * (torch.arange(Nk) // 64).float())[None, :, None]
    return q.half(), k.half(), v.half()


def prescale(q, d):
    """the query a packer that folds d^-1/2 * log2(e) into the projection hands over (one fp16 rounding)"""
    return (q.float() * (d ** -0.5 * LOG2E)).half()


def heads(t, H, d):
    B, N, _ = t.shape
    return t.reshape(B, N, H, d).permute(0, 2, 1, 3)                       # [B, H, N, d]


def unheads(t):
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * d)


def _dead(Nq, Nk, causal, device):
    last = torch.arange(Nq, device=device).clamp(max=Nk - 1) if causal else torch.full((Nq,), Nk - 1, device=device)
    return torch.arange(Nk, device=device)[None, :] > last[:, None]        # [Nq, Nk]: keys the row may not see


def fused_ref_bound(q, k, v, H, d, c, causal=False, u=U, device="cpu"):
    """(ref, bound) of the fused output, fp64 [B, Nq, H d] on the CPU; c = scale * log2(e) (1 for a prescaled q).  Computed on `device`."""
    qh, kh, vh = (heads(t.to(device).double(), H, d) for t in (q, k, v))
    Nq, Nk = qh.shape[2], kh.shape[2]
    dead = _dead(Nq, Nk, causal, device)
    e = (qh @ kh.transpose(-1, -2)) * (c * LN2)
    A = (c * (qh.abs() @ kh.abs().transpose(-1, -2))).masked_fill(dead, 0.0).amax(-1, keepdim=True)
    P = torch.softmax(e.masked_fill(dead, -INF), -1)
    ref = P @ vh
    eps = 2.0 ** -11 + 2 * LN2 * (d + 4) * u * A + 4 * u
    T1, T3 = torch.empty_like(ref), torch.empty_like(ref)
    cs = max(1, (1 << 25) // (P.numel()))
    for c0 in range(0, d, cs):
        dv = (vh[:, :, None, :, c0:c0 + cs] - ref[:, :, :, None, c0:c0 + cs]).abs()       # [B, H, Nq, Nk, cs]
        T1[..., c0:c0 + cs] = (P[..., None] * dv).sum(-2)
        T3[..., c0:c0 + cs] = dv.masked_fill(dead[:, :, None], 0.0).amax(-2)
    bound = 0.5 * fp16_ulp(ref) + 1.01 * eps * T1 + (Nk + 8) * u * (P @ vh.abs() + ref.abs()) + Nk * 2.0 ** -24 * T3
    return unheads(ref).cpu(), unheads(bound).cpu()


def probs_ref_bound(q, k, H, d, c, qc=None, kc=None, u=U):
    """(P, bound) fp64 [B H, Nq, Nk]; qc / kc: the uint8 carries of split operands (the reference is taken on the decoded values)."""
    q64 = (ops.carry_decode(q, qc) if qc is not None else q).double()
    k64 = (ops.carry_decode(k, kc) if kc is not None else k).double()
    qh, kh = heads(q64, H, d), heads(k64, H, d)
    A = (c * (qh.abs() @ kh.abs().transpose(-1, -2))).amax(-1, keepdim=True)
    P = torch.softmax((qh @ kh.transpose(-1, -2)) * (c * LN2), -1)
    rel = 2 * LN2 * (d + 4) * u * A + (k.shape[1] + 8) * u + 4 * u
    if qc is not None or kc is not None:
        ql, kl = heads(q64 - q.double(), H, d).abs(), heads(k64 - k.double(), H, d).abs()       # 2^-14 ql, 2^-14 kl
        rel = rel + LN2 * c * (ql @ kl.transpose(-1, -2)).amax(-1, keepdim=True)
    bound = 0.5 * fp16_ulp(P) + rel * P + 2.0 ** -25
    return P.flatten(0, 1), bound.flatten(0, 1)


def worst(got, ref, bound):
    """(largest error / bound, its flat index)"""
    ratio = (got.double() - ref).abs() / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, INF), ratio)
    i = int(ratio.flatten().argmax())
    return float(ratio.flatten()[i]), i


# ===================================================================================================== 4. the kernels' arithmetic
def emulate_fused(q, k, v, H, d, c, causal=False, m_fp16=False, brk=None):
    """The tiled kernel's arithmetic in torch: fp32 scores, 64-key tiles, running offset moved when a row maximum outgrows it by more than
    2^8 (per row; the kernel moves a whole wave's rows together, which is one of the admissible schedules), p = exp2(fma(s, c, -m c))
    rounded to fp16 for numerator AND denominator, fp32 accumulation, one rounding of O / l.  m_fp16: the offset kept fp16-exact (MODE 1).
    brk: None, or one of the bugs the bound is there to see - "ragged" (the last key of the ragged tile dropped), "causal" (one key too
    many), "head" (head h also multiplies the first 8 columns of head h + 1), "rescale" (a rescale shrinks O but not l)."""
    qh, kh, vh = heads(q.float(), H, d), heads(k.float(), H, d), heads(v.float(), H, d)
    B, _, Nq, _ = qh.shape
    Nk = kh.shape[2]
    s_all = qh @ kh.transpose(-1, -2)
    if brk == "head":
        s_all = s_all + qh.roll(-1, 1)[..., :8] @ kh.roll(-1, 1)[..., :8].transpose(-1, -2)
    last = torch.arange(Nq).clamp(max=Nk - 1) if causal else torch.full((Nq,), Nk - 1)
    if brk == "causal":
        last = (last + 1).clamp(max=Nk - 1)
    if brk == "ragged":
        last = last.clamp(max=Nk - 2)
    s_all = s_all.masked_fill(torch.arange(Nk)[None, :] > last[:, None], -INF)
    c32 = torch.tensor(c, dtype=torch.float32)
    m = torch.full((B, H, Nq), -INF)
    l = torch.zeros(B, H, Nq)
    O = torch.zeros(B, H, Nq, d)
    for t0 in range(0, Nk, 64):
        s = s_all[..., t0:t0 + 64]
        mx = s.amax(-1)
        need = (mx - m) * c32 > 8.0                                        # (nan and -inf compare false: a tile of masked keys moves nothing)
        m_new = torch.where(need, torch.maximum(m, mx), m)
        if m_fp16:
            m_new = m_new.half().float()
        alpha = torch.where(need & torch.isfinite(m), torch.exp2((m - m_new) * c32), torch.ones_like(m))
        O = O * alpha[..., None]
        if brk != "rescale":
            l = l * alpha
        m = m_new
        p = torch.exp2((s.double() * c + (-m * c32).double()[..., None]).float()).half().float()     # one rounding: the FMA
        l = l + p.sum(-1)
        O = O + p @ vh[:, :, t0:t0 + 64]
    return unheads((O * (1.0 / l)[..., None]).half())


def emulate_probs(q, k, H, d, c, qc=None, kc=None):
    """attn_probs_kernel's arithmetic: fp32 scores (split: + 2^-14 (kl.qh + kh.ql) through an fp32 FMA), times c, exp2(s - max),
    fp32 row sum, times its reciprocal, one rounding."""
    qh, kh = heads(q.float(), H, d), heads(k.float(), H, d)
    s = qh @ kh.transpose(-1, -2)
    if qc is not None or kc is not None:
        lo = lambda t, cr: heads(cr.view(torch.float8_e5m2).float(), H, d) if cr is not None else torch.zeros_like(t)
        t = heads(k.float(), H, d)
        s = s + (qh @ lo(t, kc).transpose(-1, -2) + lo(qh, qc) @ kh.transpose(-1, -2)) * (1.0 / 16384.0)
    s = s * torch.tensor(c, dtype=torch.float32)
    e = torch.exp2(s - s.amax(-1, keepdim=True))
    return (e * (1.0 / e.sum(-1, keepdim=True))).half().flatten(0, 1)


def split_inputs(q, k, seed):
    """(qh, qc, kh, kc): fp16 + carry of values that are NOT fp16 numbers (the fp16 inputs plus a perturbation below their ulp)"""
    g = torch.Generator().manual_seed(seed)
    qf = q.float() * (1.0 + 2.0 ** -12 * torch.randn(q.shape, generator=g))
    kf = k.float() * (1.0 + 2.0 ** -12 * torch.randn(k.shape, generator=g))
    (qh, qc), (kh, kc) = ops.carry_encode(qf), ops.carry_encode(kf)
    return qh, qc, kh, kc


def row_case(r, shrink=False):
    """(q, k, v, c, B, H) of a fused row: inputs (prescaled if the row says so) and the exponent scale.  shrink: at most 2 samples, 3 heads."""
    B, H = (min(r["B"], 2), min(r["H"], 3)) if shrink else (r["B"], r["H"])
    q, k, v = attn_inputs(B, H, r["Nq"], r["Nk"], r["d"], spread=r.get("spread", False))
    if r["flags"] & PRESC:
        return prescale(q, r["d"]), k, v, 1.0, B, H
    return q, k, v, r["d"] ** -0.5 * LOG2E, B, H


def scale_of(r):
    return r["d"] ** -0.5


# ===================================================================================================================== the tests
def test_every_row_takes_the_instantiation_it_is_there_for():
    for rows in FUSED_TABLES.values():
        for r in rows:
            got, got_cross, _ = plan_fused(r["B"], r["H"], r["Nq"], r["Nk"], r["d"], r["flags"])
            assert fused_dispatch(r["B"], r["H"], r["Nq"], r["Nk"], r["d"], r["flags"]) == r["want"] == got, r
            if r["want"][0] == "cross":
                assert cross_plan(r["B"], r["H"], r["Nq"], r["Nk"]) == r["cross"] == got_cross, r
    for r in G_ROWS:
        assert probs_dispatch(r["d"], r["ldp"], r["split"], r["epi"]) == r["want"] == plan_probs(r)[0], r
        assert r["ldp"] % 8 == 0 and r["ldp"] >= r["Nk"]
    for r in H_ROWS:
        assert masked_dispatch(r["Nk"], r["d"]) == plan_masked(r["B"], r["H"], r["Nq"], r["Nk"], r["d"])[0], r
    # the wide rows are the smallest that reach the wide kernels, the cross rows sit on the threshold
    assert all(cdiv(r["Nq"], 256) * r["B"] * r["H"] == 512 for r in D_ROWS) and all(r["B"] * r["H"] == 2048 for r in E_ROWS)


# Shapes (B, H, Nq, Nk) of the fused sweep: one per regime (plain, causal-capable, wide, cross with both STL), then both sides of every
# threshold of the dispatch.  wide: ceil(Nq / 256) B H = 511 | 512, and Nk = 255 | 256 at 512 blocks (Nq == Nk there: a causal call must
# stay narrow).  cross: ceil(Nq / 128) B H = 2047 | 2048 at the key counts either side of 64 | 65, 80 | 81 (STL), 96 | 97, crossed with
# every head dim (32 | 40, 48 | 56, 64 | 72 among them); 2048 blocks with Nq == Nk (a causal call must stay on the tiled kernel).
# Tiles per wave: ceil(Nq / (128 tpw)) B H = 1023 | 1024 for tpw = 8, 4, 2, 1 - below 1024 blocks at tpw = 2 the cross rule itself
# (2048 blocks of 128 rows) cannot hold, so one tile per wave is out of reach and the last three shapes run tiled.
SWEEP_SHAPES = [(2, 2, 100, 77), (2, 2, 100, 100), (4, 64, 300, 256), (32, 64, 100, 77), (32, 64, 100, 96),
                (1, 511, 256, 256), (1, 512, 256, 256), (1, 512, 256, 255), (1, 2048, 77, 77)] + \
               [(1, bh, 128, Nk) for bh in (2047, 2048) for Nk in (64, 65, 80, 81, 96, 97)] + \
               [(1, 1023, 1024, 77), (1, 1024, 1024, 77), (1, 341, 1536, 77), (1, 512, 1024, 77), (1, 341, 768, 77), (1, 256, 1024, 77),
                (1, 1023, 128, 77), (1, 128, 1024, 77)]


def test_the_mirror_agrees_with_the_library_and_the_tables_reach_everything():
    seen = {0: set(), 1: set(), 2: {}, 3: set()}                           # family -> variants the sweep reached (probs: variant -> EPI)
    tpws = set()
    for d in range(8, 161, 8):
        for flags in (0, PRESC, PRESC | MODE0, CAUSAL, CAUSAL | PRESC, CAUSAL | PRESC | MODE0):
            for B, H, Nq, Nk in SWEEP_SHAPES:
                if (flags & CAUSAL) and Nq != Nk:
                    continue
                got, got_cross, i = plan_fused(B, H, Nq, Nk, d, flags)
                assert got == fused_dispatch(B, H, Nq, Nk, d, flags), (B, H, Nq, Nk, d, flags)
                assert got_cross is None or got_cross == cross_plan(B, H, Nq, Nk), (B, H, Nq, Nk, d)
                seen[i.family].add(i.variant)
                tpws.add(i.tiles_per_wave)
        for ldp in (88, 96, 104):
            for sp in (False, True):
                for ep in (0, 1, 2):
                    r = dict(B=3, H=2, Nq=100, Nk=77, d=d, ldp=ldp, split=sp, epi=ep)
                    if ep == 2 and ldp > 96:                               # the cross edit exists for <= 96 columns only
                        assert plan(1, 3, 2, 100, 77, d, ldp, split=sp, epi=2)[0] == -1
                        continue
                    got, i = plan_probs(r)
                    assert got == probs_dispatch(d, ldp, sp, ep), r
                    seen[2][i.variant] = i.EPI
        for Nk in (1, 32, 33, 64, 65, 96, 97, 128) if d <= 128 else ():
            got, i = plan_masked(2, 3, 100, Nk, d)
            assert got == masked_dispatch(Nk, d), (Nk, d)
            seen[3].add(i.variant)
    assert tpws == {0, 8, 4, 2}                                            # (0: the tiled kernel)
    assert [sorted(seen[f]) for f in range(4)] == [list(range(n)) for n in (22, 6, 40, 16)]
    # ... and the tables hit all of it (the cross-edit instantiations, EPI = 2, keep their bit-for-bit tests in test_ops_gpu.py / test_p2p_gpu.py)
    rows = [plan_fused(r["B"], r["H"], r["Nq"], r["Nk"], r["d"], r["flags"])[2] for t in FUSED_TABLES.values() for r in t]
    assert [{i.variant for i in rows if i.family == f} for f in (0, 1)] == [seen[0], seen[1]]
    assert {plan_probs(r)[1].variant for r in G_ROWS} == {v for v, epi in seen[2].items() if epi != 2}


@pytest.mark.parametrize("sec", list(FUSED_TABLES))
def test_the_emulation_stays_inside_the_fused_bound(sec):
    top = 0.0
    for r in FUSED_TABLES[sec]:
        q, k, v, c, B, H = row_case(r, shrink=True)
        causal = bool(r["flags"] & CAUSAL)
        got = emulate_fused(q, k, v, H, r["d"], c, causal, m_fp16=r["want"][4] == 1)
        ref, bound = fused_ref_bound(q, k, v, H, r["d"], c, causal, u=2.0 ** -24)
        ratio, _ = worst(got, ref, bound)
        assert ratio <= 1.0, (r, ratio)
        assert rel_l2(got, ref) < TOL
        top = max(top, ratio)
    print(f"[attn-edges cpu {sec}] emulation worst error / bound (u = 2^-24) {top:.3f} over {len(FUSED_TABLES[sec])} rows")


def test_the_emulation_stays_inside_the_probs_bound():
    top = top_s = 0.0
    for r in G_ROWS:
        q, k, _ = attn_inputs(r["B"], r["H"], r["Nq"], r["Nk"], r["d"])
        qc = kc = None
        if r["split"]:
            q, qc, k, kc = split_inputs(q, k, 7)
        c = scale_of(r) * LOG2E
        got = emulate_probs(q, k, r["H"], r["d"], c, qc, kc)
        P, bound = probs_ref_bound(q, k, r["H"], r["d"], c, qc, kc, u=2.0 ** -24)
        ratio, _ = worst(got, P, bound)
        assert ratio <= 1.0, (r, ratio)
        assert float((got.double().sum(-1) - 1.0).abs().max()) <= r["Nk"] * 2.0 ** -11
        top, top_s = (top, max(top_s, ratio)) if r["split"] else (max(top, ratio), top_s)
    print(f"[attn-edges cpu G] emulation worst error / bound (u = 2^-24) {top:.3f}, split operands {top_s:.3f}, over {len(G_ROWS)} rows")


BREAKS = [("ragged", _row("A", 2, 3, 100, 77, 72, 0, None)),                # key 76 of the peeled tile dropped
          ("causal", _row("C", 2, 2, 130, 130, 64, CAUSAL, None)),          # row n sees key n + 1
          ("head", _row("A", 2, 3, 100, 77, 24, 0, None)),                  # d = 24 in the KS = 2 kernel without the `dd < d` guard
          ("rescale", _row("B", 2, 2, 129, 193, 96, 0, None, spread=True))]


@pytest.mark.parametrize("brk,r", BREAKS, ids=[b for b, _ in BREAKS])
def test_a_broken_emulation_leaves_the_bound(brk, r):
    """The bound (at the u the GPU tests use) sees the bugs it is for - on the very rows of the tables where they would show."""
    q, k, v, c, B, H = row_case(r)
    causal = bool(r["flags"] & CAUSAL)
    ref, bound = fused_ref_bound(q, k, v, H, r["d"], c, causal)
    assert worst(emulate_fused(q, k, v, H, r["d"], c, causal), ref, bound)[0] <= 1.0
    bad = emulate_fused(q, k, v, H, r["d"], c, causal, brk=brk)
    ratio, i = worst(bad, ref, bound)
    n_bad = int(((bad.double() - ref).abs() > bound).sum())
    print(f"[attn-edges cpu break {brk}] worst error / bound {ratio:.1f}, {n_bad} of {ref.numel()} elements outside, rel-L2 {rel_l2(bad, ref):.1e}")
    assert ratio > 1.0 and n_bad >= 1


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
_BUF = (C.c_char * 4096)()                         # host memory, never dereferenced: every call below is refused before any HIP call
P0 = (C.addressof(_BUF) + 15) // 16 * 16


def _fused(**kw):
    a = dict(q=P0, k=P0, vt=P0, out=P0, B=2, H=2, Nq=35, Nk=35, d=64, ldq=128, ldk=128, ldvt=40, ldo=128, vt_bs=0, scale=0.125, flags=0)
    a.update(kw)
    return _lib.load().icd_attention_fused_ex(a["q"], a["k"], a["vt"], a["out"], a["B"], a["H"], a["Nq"], a["Nk"], a["d"], a["ldq"], a["ldk"],
                                              a["ldvt"], a["ldo"], a["vt_bs"], a["scale"], a["flags"], None)


FUSED_REFUSALS = [
    ("unknown flags", dict(flags=8), "unknown flags"),
    ("causal Nq != Nk", dict(flags=CAUSAL, Nq=36), "Nq == Nk"),
    ("d = 0", dict(d=0), "head dim"), ("d = 12", dict(d=12), "head dim"), ("d = 168", dict(d=168, ldq=336, ldk=336, ldo=336), "head dim"),
    ("ldvt < Nk", dict(ldvt=32), "ldvt >= Nk"),
    ("ldq % 8", dict(ldq=132), "16-byte aligned"), ("ldk % 8", dict(ldk=132), "16-byte aligned"), ("ldvt % 8", dict(ldvt=44), "16-byte aligned"),
    ("ldo % 4", dict(ldo=130), "16-byte aligned"),
    ("scale 0", dict(scale=0.0), "scale must be positive"), ("scale < 0", dict(scale=-1.0), "scale must be positive"),
    ("q null", dict(q=None), "null pointer"), ("k null", dict(k=None), "null pointer"), ("vt null", dict(vt=None), "null pointer"),
    ("out null", dict(out=None), "null pointer"), ("empty", dict(Nq=0), "empty shape"),
    ("ldq < H d", dict(ldq=120), ">= H * d"), ("ldk < H d", dict(ldk=64), ">= H * d"), ("ldo < H d", dict(ldo=124), ">= H * d"),
    ("vt_batch_stride short", dict(vt_bs=2 * 64 * 40 - 8), "vt_batch_stride below"), ("vt_batch_stride < 0", dict(vt_bs=-1), "vt_batch_stride below"),
    ("q misaligned", dict(q=P0 + 8), "16-byte aligned, out 8-byte"), ("k misaligned", dict(k=P0 + 2), "16-byte aligned, out 8-byte"),
    ("vt misaligned", dict(vt=P0 + 8), "16-byte aligned, out 8-byte"), ("out misaligned", dict(out=P0 + 4), "16-byte aligned, out 8-byte"),
]


@pytest.mark.parametrize("name,kw,fragment", FUSED_REFUSALS, ids=[r[0] for r in FUSED_REFUSALS])
def test_attention_fused_refuses(name, kw, fragment):
    lib = _lib.load()
    assert _fused(**kw) == -1, name
    assert fragment.encode() in lib.icd_last_error(), (name, lib.icd_last_error())


def _epi(**kw):
    e = _lib.ProbsEpilogue()
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _probs(entry="plain", epi=None, **kw):
    a = dict(q=P0, qc=P0, k=P0, kc=P0, p=P0, B=3, H=2, Nq=35, Nk=35, d=64, ldq=128, ldk=128, ldp=40, scale=0.125)
    a.update(kw)
    lib = _lib.load()
    tail = (a["B"], a["H"], a["Nq"], a["Nk"], a["d"], a["ldq"], a["ldk"], a["ldp"], a["scale"])
    if entry == "plain":
        return lib.icd_attention_probs(a["q"], a["k"], a["p"], *tail, None)
    if entry == "split":
        return lib.icd_attention_probs_split(a["q"], a["qc"], a["k"], a["kc"], a["p"], *tail, None)
    return lib.icd_attention_probs_ex(a["q"], a["qc"], a["k"], a["kc"], a["p"], *tail, C.byref(epi), None)


PROBS_REFUSALS = [
    ("q null", "plain", None, dict(q=None), "null pointer"), ("probs null", "split", None, dict(p=None), "null pointer"),
    ("empty", "plain", None, dict(Nk=0), "empty shape"),
    ("d = 0", "plain", None, dict(d=0), "head dim"), ("d = 12", "plain", None, dict(d=12), "head dim"),
    ("d = 168", "plain", None, dict(d=168, ldq=336, ldk=336), "head dim"),
    ("ldp < Nk", "plain", None, dict(ldp=32), "ldp >= Nk"), ("ldp % 8", "plain", None, dict(ldp=44), "ldp >= Nk"),
    ("ldq % 8", "plain", None, dict(ldq=132), "16-byte aligned"), ("scale 0", "plain", None, dict(scale=0.0), "scale must be positive"),
    ("grid limit", "plain", None, dict(B=32768), "grid limit"),
    ("ldq < H d", "plain", None, dict(ldq=120), ">= H * d"), ("ldk < H d", "split", None, dict(ldk=64), ">= H * d"),
    ("q misaligned", "plain", None, dict(q=P0 + 8), "16-byte aligned, the carries 8-byte"),
    ("k misaligned", "plain", None, dict(k=P0 + 2), "16-byte aligned, the carries 8-byte"),
    ("probs misaligned", "plain", None, dict(p=P0 + 8), "16-byte aligned, the carries 8-byte"),
    ("q_carry misaligned", "split", None, dict(qc=P0 + 4), "16-byte aligned, the carries 8-byte"),
    ("k_carry misaligned", "split", None, dict(kc=P0 + 1), "16-byte aligned, the carries 8-byte"),
    ("acc misaligned", "ex", dict(acc=P0 + 8), {}, "acc must be 16-byte aligned"),
    ("first_cond_sample", "ex", dict(acc=P0, first_cond_sample=3), {}, "first_cond_sample out of range"),
    ("edit without D", "ex", dict(edit_At=P0, first_cond_sample=1), {}, "the cross-attention edit needs edit_D"),
    ("edit with 81 keys", "ex", dict(edit_At=P0, edit_D=P0, first_cond_sample=1), dict(Nk=81, ldp=88),
     "the cross-attention edit needs edit_D"),
    ("first_cond_row % H", "ex", dict(acc=P0, first_cond_row=3), {}, "first_cond_row must be a multiple of H"),
    ("edit without an edited prompt", "ex", dict(self_from_base=1, first_cond_sample=2), {}, "an edit needs a base prompt"),
    ("group_count without edit_count", "ex", dict(acc=P0, group_count=2), {}, "needs edit_count > 0"),
    ("edit_count mismatch", "ex", dict(acc=P0, edit_count=1), {}, "does not match"),
    ("groups do not divide", "ex", dict(acc=P0, group_count=2, edit_count=1), {}, "groups of"),
]


@pytest.mark.parametrize("name,entry,epi,kw,fragment", PROBS_REFUSALS, ids=[r[0] for r in PROBS_REFUSALS])
def test_attention_probs_refuses(name, entry, epi, kw, fragment):
    lib = _lib.load()
    assert _probs(entry, _epi(**epi) if epi is not None else None, **kw) == -1, name
    assert fragment.encode() in lib.icd_last_error(), (name, lib.icd_last_error())


_Q = dict(B=3, H=2, Nq=35, Nk=35, d=64, ldp=40)
PLAN_REFUSALS = [                                  # what the entries refuse on shape and flags alone, with their status and message
    ("fused d = 12", 0, dict(d=12), -1, "head dim"), ("fused d = 168", 0, dict(d=168), -1, "head dim"),
    ("fused unknown flags", 0, dict(flags=8), -1, "unknown flags"), ("fused causal Nq != Nk", 0, dict(flags=CAUSAL, Nq=36), -1, "Nq == Nk"),
    ("masked Nk = 129", 2, dict(Nk=129), -2, "128 keys"), ("masked d = 136", 2, dict(d=136), -2, "head dim"),
    ("masked d = 36", 2, dict(d=36), -2, "head dim"),
    ("probs d = 12", 1, dict(d=12), -1, "head dim"), ("probs d = 168", 1, dict(d=168), -1, "head dim"),
    ("probs ldp < Nk", 1, dict(ldp=32), -1, "ldp >= Nk"), ("probs ldp % 8", 1, dict(ldp=44), -1, "ldp >= Nk"),
    ("probs edit with 81 keys", 1, dict(epi=2, Nk=81, ldp=88), -1, "the cross-attention edit needs edit_D"),
    ("probs edit with ldp 104", 1, dict(epi=2, ldp=104), -1, "the cross-attention edit needs edit_D"),
    ("probs grid limit", 1, dict(B=32768), -1, "grid limit"),
]


@pytest.mark.parametrize("name,entry,kw,status,fragment", PLAN_REFUSALS, ids=[r[0] for r in PLAN_REFUSALS])
def test_attention_plan_refuses_what_the_entry_refuses(name, entry, kw, status, fragment):
    assert plan(entry, **dict(_Q, **kw))[0] == status, name
    assert fragment.encode() in _lib.load().icd_last_error(), (name, _lib.load().icd_last_error())


def test_attention_plan_accepts_what_only_a_pointer_refuses():
    lib = _lib.load()
    assert _fused(q=None) == -1 and _fused(out=P0 + 4) == -1 and plan(0, 2, 2, 35, 35, 64)[0] == 0
    assert _probs(q=None) == -1 and _probs("split", kc=P0 + 1) == -1 and plan(1, 3, 2, 35, 35, 64, 40, split=True)[0] == 0
    assert _probs("ex", _epi(acc=P0 + 8)) == -1 and plan(1, 3, 2, 35, 35, 64, 40, split=True, epi=1)[0] == 0
    assert lib.icd_attention_masked(P0, P0, P0, P0, None, 2, 2, 35, 35, 64, 128, 128, 40, 128, 0, 0.125, None) == -1
    assert plan(2, 2, 2, 35, 35, 64)[0] == 0
