"""The normalisation kernels (csrc/norm.hip), the fp32-fidelity split-operand entries and the small elementwise entries against plain torch
fp64 on the CPU, at the shapes where their dispatch changes: group counts other than 32, both sides of every small-map / streaming switch,
guard rows behind every output, DC offsets and zero variance, every register width of the row softmax.

Inputs are fp16- or fp32-representable, so both sides see identical values.  Where a kernel's contract is exact (layout, split, gather,
max) the assertion is torch.equal.  The bounds of the DC-offset, zero-variance and activation tests come from the restatement of the
kernels' arithmetic in test_norm_edges.py, which checks them on the CPU alone.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
import test_norm_edges as cpu

pytestmark = pytest.mark.gpu
TOL = 1e-3
SENTINEL = -7.0


def _ops():
    from invertible_cd_amd import ops
    return ops


def _raw():
    from invertible_cd_amd import _lib
    return _lib, _lib.load()


def r16(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def r32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def cu(t):
    return None if t is None else t.cuda()


def cat2(a, b):
    return a if b is None else torch.cat([a, b], -1)


# ================================================================================================ A. fp16 GroupNorm
GN_GROUP_CASES = [(24, 0, 8),        # cpg 3, 8 groups per slab
                  (40, 0, 4),        # cpg 10, 4 groups per slab
                  (16, 8, 2),        # cpg 12, 2 groups per slab; the group straddles the two sources
                  (64, 0, 1),        # one group
                  (1024, 0, 1),      # a 1024-channel slab: the small-map kernel is refused, streaming even at HW = 100
                  (40, 24, 16),      # cpg 4; the concat boundary falls inside a group
                  (320, 0, 5)]       # cpg 64


@pytest.mark.parametrize("HW", [100, 1090])          # small-map kernel / streaming kernels with a ragged last slab and apply block
@pytest.mark.parametrize("C0,C1,groups", GN_GROUP_CASES)
def test_groupnorm_group_counts_other_than_32(C0, C1, groups, HW):
    ops = _ops()
    B, Cc = 2, C0 + C1
    assert cpu.gn_takes_small_path(B, HW, Cc, groups)[0] == (HW == 100 and Cc != 1024)
    x0 = (r16(B * HW, C0, seed=20).float() * 1.5 + 0.3).half()
    x1 = r16(B * HW, C1, seed=21) if C1 else None
    g, b = cpu.affine(Cc)
    for silu in (True, False):
        out = ops.groupnorm(x0.cuda(), B, HW, g.cuda(), b.cuda(), 1e-5, silu, x2=cu(x1), groups=groups)
        e = rel_l2(out, cpu.gn_ref64(cat2(x0, x1), B, HW, groups, g, b, 1e-5, silu))
        assert torch.isfinite(out).all() and e < TOL, (silu, e)
    if not C1:
        return
    # the carry variant on the two-source cases: normalises fp16 + 2^-14 * bf8, aux = [x2 | lo0 | lo1] bit for bit
    v0, v1 = r32(B * HW, C0, seed=30, scale=1.5) + 0.3, r32(B * HW, C1, seed=31)
    (h0, c0), (h1, c1) = ops.carry_encode(v0), ops.carry_encode(v1)
    out, aux = ops.groupnorm_carry(h0.cuda(), B, HW, g.cuda(), b.cuda(), 1e-5, True, carry=c0.cuda(), x2=h1.cuda(), carry2=c1.cuda(),
                                   groups=groups, with_aux=True)
    full = torch.cat([ops.carry_decode(h0, c0), ops.carry_decode(h1, c1)], -1)
    assert rel_l2(out, cpu.gn_ref64(full, B, HW, groups, g, b, 1e-5, True)) < TOL
    lo0 = (c0.view(torch.float8_e5m2).float() / 16384.0).half()
    lo1 = (c1.view(torch.float8_e5m2).float() / 16384.0).half()
    assert torch.equal(aux.cpu(), torch.cat([h1, lo0, lo1], 1))


def test_groupnorm_refuses_group_counts_it_cannot_hold():
    ops = _ops()
    g, b = cpu.affine(128)
    x = r16(2 * 16, 128, seed=20).cuda()
    for groups in (64, 5):                            # more than the 32 the apply kernels keep in LDS; no divisor of C
        with pytest.raises(RuntimeError, match="bad group count"):
            ops.groupnorm(x, 2, 16, g.cuda(), b.cuda(), 1e-5, True, groups=groups)
        with pytest.raises(RuntimeError, match="bad group count"):
            ops.groupnorm_carry(x, 2, 16, g.cuda(), b.cuda(), 1e-5, True, groups=groups)


_SWITCH = {}


def _switch_data(key, B, HW, Cc, groups):
    """One generator per switch: the two sides share their samples, and the fp64 reference of the larger side is computed once."""
    if key not in _SWITCH:
        x = (r16(B * HW, Cc, seed=40).float() * 1.5 + 0.3).half()
        g, b = cpu.affine(Cc)
        _SWITCH[key] = (x, g, b, cpu.gn_ref64(x, B, HW, groups, g, b, 1e-5, True))
    return _SWITCH[key]


@pytest.mark.parametrize("HW", [1024, 1025])
def test_groupnorm_both_sides_of_the_map_size_switch(HW):
    ops = _ops()
    B, Cc = 2, 32
    assert cpu.gn_takes_small_path(B, HW, Cc, 32)[0] == (HW == 1024)
    x = (r16(B * 1025, Cc, seed=41).float() * 1.5 + 0.3).half().reshape(B, 1025, Cc)[:, :HW].reshape(B * HW, Cc).contiguous()
    g, b = cpu.affine(Cc)
    out = ops.groupnorm(x.cuda(), B, HW, g.cuda(), b.cuda(), 1e-5, True)
    assert rel_l2(out, cpu.gn_ref64(x, B, HW, 32, g, b, 1e-5, True)) < TOL


@pytest.mark.parametrize("B", [12, 13])
def test_groupnorm_both_sides_of_the_element_count_switch(B):
    """B * HW * C = 12 * 2^20 exactly is the last size of the small-map kernel; one sample more streams."""
    ops = _ops()
    HW, Cc = 1024, 1024
    assert cpu.gn_takes_small_path(B, HW, Cc, 32)[0] == (B == 12)
    x, g, b, ref = _switch_data("elements", 13, HW, Cc, 32)            # (GroupNorm is per sample: the first 12 are the B = 12 case)
    out = ops.groupnorm(x[:B * HW].cuda(), B, HW, g.cuda(), b.cuda(), 1e-5, True)
    assert rel_l2(out, ref[:B * HW]) < TOL


def test_groupnorm_with_more_samples_than_statistics_blocks():
    """B = 769: 768 / B rounds to zero statistics blocks per sample, gn_pix_per_split clamps it to one.  At HW = 4 the fp16 entry takes the
    small-map kernel whatever B is, so the clamp is reached through the workspace size and the fp32 entry (streaming only)."""
    ops = _ops()
    lib = _raw()[1]
    B, HW, Cc, groups = 769, 4, 8, 4
    x = (r16(B * HW, Cc, seed=42).float() * 1.5 + 0.3).half()
    g, b = cpu.affine(Cc)
    ref = cpu.gn_ref64(x, B, HW, groups, g, b, 1e-5, True)
    assert rel_l2(ops.groupnorm(x.cuda(), B, HW, g.cuda(), b.cuda(), 1e-5, True, groups=groups), ref) < TOL
    assert lib.icd_groupnorm_ws_floats(B, HW, groups) == B * groups * 2
    assert lib.icd_groupnorm_ws_floats(5000, HW, groups) == 5000 * groups * 2          # 4096 / B rounds to zero as well
    out = ops.groupnorm_f32_split(x.float().cuda(), B, HW, g.cuda(), b.cuda(), 1e-5, True, groups=groups).double().cpu()
    assert rel_l2(out[:, :Cc] + out[:, Cc:2 * Cc], ref) < 1e-5


def test_groupnorm_finishes_more_than_16_statistics_blocks():
    """B = 1, HW = 4097: 64 statistics blocks, the last of 2 pixels - four trips of the 16-lane finish loop - in a workspace of exactly
    icd_groupnorm_ws_floats with a guard band behind it."""
    ops = _ops()
    _lib, lib = _raw()
    B, HW, Cc, groups = 1, 4097, 32, 32
    pps = cpu.gn_pix_per_split(B, HW)
    nsplit = (HW + pps - 1) // pps
    assert (nsplit, HW - (nsplit - 1) * pps) == (64, 2)
    n_ws = lib.icd_groupnorm_ws_floats(B, HW, groups)
    assert n_ws >= B * nsplit * groups * 2
    x = (r16(B * HW, Cc, seed=43).float() * 1.5 + 0.3).half()
    g, b = cpu.affine(Cc)
    ws = torch.full((n_ws + 64,), SENTINEL, device="cuda")
    out = torch.empty(B * HW, Cc, device="cuda", dtype=torch.float16)
    xd, gd, bd = x.cuda(), g.cuda(), b.cuda()
    _lib.check(lib.icd_groupnorm(ops._p(xd), Cc, None, 0, B, HW, groups, ops._p(gd), ops._p(bd), 1e-5, 1, ops._p(out), ops._p(ws),
                                 ops._stream()), "icd_groupnorm")
    assert rel_l2(out, cpu.gn_ref64(x, B, HW, groups, g, b, 1e-5, True)) < TOL
    assert torch.all(ws[n_ws:] == SENTINEL)


@pytest.mark.parametrize("B,HW", [(3, 37), (1, 1090)])              # small-map kernel / streaming kernels; B * HW is no multiple of 64
def test_groupnorm_writes_nothing_outside_its_outputs(B, HW):
    """icd_groupnorm_carry through the C ABI: two rows behind `out`, two rows behind `aux` and the 8 pad columns of an aux with
    ld_aux = C0 + 2 C1 + 8 come back as they were."""
    ops = _ops()
    _lib, lib = _raw()
    C0, C1, groups = 16, 8, 2
    Cc, rows, ld_aux = C0 + C1, B * HW, C0 + 2 * C1 + 8
    assert cpu.gn_takes_small_path(B, HW, Cc, groups)[0] == (HW == 37)
    v0, v1 = r32(rows, C0, seed=44, scale=1.5) + 0.3, r32(rows, C1, seed=45)
    (h0, c0), (h1, c1) = ops.carry_encode(v0), ops.carry_encode(v1)
    g, b = cpu.affine(Cc)
    out = torch.full((rows + 2, Cc), SENTINEL, device="cuda", dtype=torch.float16)
    aux = torch.full((rows + 2, ld_aux), SENTINEL, device="cuda", dtype=torch.float16)
    ws = torch.empty(lib.icd_groupnorm_ws_floats(B, HW, groups), device="cuda")
    dev = [t.cuda() for t in (h0, c0, h1, c1, g, b)]
    _lib.check(lib.icd_groupnorm_carry(ops._p(dev[0]), C0, ops._p(dev[1]), ops._p(dev[2]), C1, ops._p(dev[3]), B, HW, groups, ops._p(dev[4]),
                                       ops._p(dev[5]), 1e-5, 1, ops._p(out), ops._p(aux), ld_aux, ops._p(ws), ops._stream()),
               "icd_groupnorm_carry")
    full = torch.cat([ops.carry_decode(h0, c0), ops.carry_decode(h1, c1)], -1)
    assert rel_l2(out[:rows], cpu.gn_ref64(full, B, HW, groups, g, b, 1e-5, True)) < TOL
    lo0 = (c0.view(torch.float8_e5m2).float() / 16384.0).half()
    lo1 = (c1.view(torch.float8_e5m2).float() / 16384.0).half()
    assert torch.equal(aux[:rows, :ld_aux - 8].cpu(), torch.cat([h1, lo0, lo1], 1))
    assert torch.all(out[rows:] == SENTINEL) and torch.all(aux[rows:] == SENTINEL) and torch.all(aux[:rows, ld_aux - 8:] == SENTINEL)


@pytest.mark.parametrize("ratio", cpu.DC_RATIOS_BOUND + cpu.DC_RATIOS_REPORTED)
@pytest.mark.parametrize("B,HW,Cc", cpu.DC_SHAPES)
def test_groupnorm_under_a_dc_offset(B, HW, Cc, ratio):
    """The fp16 GroupNorm forms E[x^2] - mean^2 from raw fp32 sums, which cancels as |mean| / std grows.  Up to a ratio of 32 it holds
    TOL (the restated arithmetic stays under TOL / 2 there, test_norm_edges.py); beyond, the error is reported, not bounded - measured on
    the MI355X (small-map / streaming): 5.0e-4 / 5.4e-4 at 64, 1.7e-3 / 2.1e-3 at 128, 5.5e-3 / 8.3e-3 at 256."""
    ops = _ops()
    x = cpu.dc_offset_input(ratio, B, HW, Cc)
    g, b = cpu.affine(Cc)
    out = ops.groupnorm(x.cuda(), B, HW, g.cuda(), b.cuda(), 1e-5, False)
    e = rel_l2(out, cpu.gn_ref64(x, B, HW, 32, g, b, 1e-5))
    print(f"[GroupNorm DC offset B={B} HW={HW} C={Cc} mean/std={ratio}] rel-L2 {e:.3e}")
    assert torch.isfinite(out).all()
    if ratio in cpu.DC_RATIOS_BOUND:
        assert e < TOL


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("value", [cpu.ZV_EXACT, cpu.ZV_NEGATIVE])
@pytest.mark.parametrize("HW", cpu.ZV_HW)
def test_groupnorm_of_a_constant_group_is_beta(HW, value, eps):
    """A group held at one value beside ordinary groups: finite, and beta to 4 x what the restated arithmetic gives (emulated
    max |y - beta|: 1.2e-4 for 3.0 at both eps, 1.6e-4 / 9.4e-4 for 20.03125 at eps 1e-5 / 1e-6).  The sums of 3.0 are exact; those of
    20.03125 round to a raw variance of about -7e-4, which only the clamp at zero keeps away from rsqrt."""
    ops = _ops()
    s = cpu.ZV_SHAPE
    B, Cc, groups = s["B"], s["C"], s["groups"]
    cpg = Cc // groups
    cols = slice(s["const_group"] * cpg, (s["const_group"] + 1) * cpg)
    x = cpu.zero_variance_input(B, HW, Cc, groups, s["const_group"], value)
    g, b = cpu.affine(Cc)
    out = ops.groupnorm(x.cuda(), B, HW, g.cuda(), b.cuda(), eps, False, groups=groups).cpu()
    assert torch.isfinite(out).all()
    dev = float((out[:, cols].double() - b[cols].double()).abs().max())
    bound = cpu.zero_variance_bound(HW, value, eps)
    print(f"[GroupNorm constant group HW={HW} value={value} eps={eps}] max |y - beta| {dev:.3e} (bound {bound:.3e})")
    assert dev <= bound
    assert rel_l2(out, cpu.gn_ref64(x, B, HW, groups, g, b, eps)) < TOL            # (the ordinary groups beside it)


# ================================================================================================ B. fp32-fidelity path
def _f32_split_input(B, HW, Cc, groups, seed):
    """fp32 [B*HW, C], unit spread, a different mean for every (sample, group): 3 .. 21 sigma."""
    cpg = Cc // groups
    mean = 3.0 + 7.0 * torch.arange(B)[:, None, None] + ((torch.arange(Cc) // cpg) % 5)[None, None, :]
    return (r32(B, HW, Cc, seed=seed) + mean).reshape(B * HW, Cc).contiguous()


@pytest.mark.parametrize("B,HW,Cc,groups,silu", [(3, 100, 32, 32, True),
                                                 (2, 1090, 12, 3, True),        # 3 chunks: 170 row slots, two idle threads
                                                 (1, 4097, 32, 8, False),       # 64 statistics blocks
                                                 (2, 70, 2048, 32, True)])      # widest accepted: one row slot
def test_groupnorm_f32_split(B, HW, Cc, groups, silu):
    """hi + lo of icd_groupnorm_f32_split against fp64 on the same fp32 inputs.  The bound is the one of
    test_fp32_groupnorm_keeps_its_digits_under_a_large_dc_offset_and_the_guard_sees_nan, rel-L2 < 3e-4 and < 4 e_in + 1e-5, with e_in (what
    rounding the input to fp32 costs) zero here: 1e-5.  (torch's own fp32 group_norm sits at about 1e-7 on these shapes - printed.)"""
    ops = _ops()
    _lib, lib = _raw()
    rows = B * HW
    x = _f32_split_input(B, HW, Cc, groups, seed=50)
    g, b = r32(Cc, seed=51), r32(Cc, seed=52)
    ref = cpu.gn_ref64(x, B, HW, groups, g, b, 1e-6, silu)
    r_t = F.group_norm(x.reshape(B, HW, Cc).permute(0, 2, 1), groups, g, b, 1e-6).permute(0, 2, 1).reshape(rows, Cc)
    e_torch = rel_l2(F.silu(r_t) if silu else r_t, ref)
    buf = torch.full((rows + 2, 3 * Cc), SENTINEL, device="cuda", dtype=torch.float16)
    ws = torch.empty(lib.icd_groupnorm_ws_floats(B, HW, groups), device="cuda")
    xd, gd, bd = x.cuda(), g.cuda(), b.cuda()
    _lib.check(lib.icd_groupnorm_f32_split(ops._p(xd), Cc, B, HW, groups, ops._p(gd), ops._p(bd), 1e-6, int(silu), ops._p(buf), ops._p(ws),
                                           ops._stream()), "icd_groupnorm_f32_split")
    assert torch.all(buf[rows:] == SENTINEL)
    out = buf[:rows].cpu()
    assert torch.equal(out, ops.groupnorm_f32_split(xd, B, HW, gd, bd, 1e-6, silu, groups=groups).cpu())
    hi, lo = out[:, :Cc], out[:, Cc:2 * Cc]
    e = rel_l2(hi.double() + lo.double(), ref)
    print(f"[fp32 GroupNorm B={B} HW={HW} C={Cc} groups={groups}] rel-L2 vs fp64 {e:.3e} (torch fp32: {e_torch:.3e})")
    assert e < 3e-4 and e < 1e-5
    assert torch.equal(hi, out[:, 2 * Cc:])
    v32 = hi.float() + lo.float()
    assert torch.equal(lo, (v32 - hi.float()).half())


def test_groupnorm_f32_split_refuses_what_it_cannot_hold():
    ops = _ops()
    for Cc, groups in ((2052, 4), (132, 33)):         # more than 512 four-channel chunks; more than 32 groups
        g, b = r32(Cc, seed=51).cuda(), r32(Cc, seed=52).cuda()
        with pytest.raises(RuntimeError, match="icd_groupnorm_f32_split"):
            ops.groupnorm_f32_split(r32(2 * 16, Cc, seed=53).cuda(), 2, 16, g, b, 1e-6, True, groups=groups)


def _split3_ref(x, scale):
    v = x * torch.tensor(scale, dtype=torch.float32)
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.cat([hi, lo, hi], -1)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -3, 2.0 ** 4])
@pytest.mark.parametrize("rows,Cc", [(1, 4), (37, 12), (300, 132)])              # 300 x 33 chunks: no whole number of 256-thread blocks
def test_split_cast_is_the_torch_split(rows, Cc, scale):
    ops = _ops()
    _lib, lib = _raw()
    x = r32(rows, Cc, seed=60, scale=3.0)
    flat = x.view(-1)
    flat[0::4] = r32(flat[0::4].numel(), seed=61, scale=1e-3) / scale              # lo below 2^-14: subnormal in fp16
    flat[1::7] = (6e4 + 100.0 * r32(flat[1::7].numel(), seed=62)) / scale          # near the end of the fp16 range
    flat[2::9] *= -1.0
    ref = _split3_ref(x, scale)
    lo = ref[:, Cc:2 * Cc].float()
    assert torch.isfinite(ref).all() and bool(((lo != 0) & (lo.abs() < 2.0 ** -14)).any()) and float(ref.abs().max()) > 5.9e4
    buf = torch.full((rows + 1, 3 * Cc), SENTINEL, device="cuda", dtype=torch.float16)
    xd = x.cuda()
    _lib.check(lib.icd_split_cast(ops._p(xd), rows, Cc, scale, ops._p(buf), ops._stream()), "icd_split_cast")
    assert torch.equal(buf[:rows].cpu(), ref) and torch.all(buf[rows:] == SENTINEL)
    assert torch.equal(ops.split_cast(xd, scale).cpu(), ref)


@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 3])                     # the last: more elements than grid threads
def test_absmax_is_exact(n):
    ops = _ops()
    x = r32(n, seed=63, scale=5.0)
    assert ops.absmax(x.cuda()) == float(x.abs().max())
    x[-1] = -1e6                                      # a negative maximum in the last element
    assert ops.absmax(x.cuda()) == 1e6
    z = torch.zeros(n)
    z[n // 2] = -0.0
    got = ops.absmax(z.cuda())
    assert got == 0.0 and math.copysign(1.0, got) == 1.0
    x[n // 3] = float("-inf")
    assert ops.absmax(x.cuda()) == float("inf")


@pytest.mark.parametrize("m", [1.0, 8192.0, 8192.0009765625, 8192.0 * 2 ** 5, 3e38])       # 8192.0009765625: the next float above 8192
def test_split_cast_guarded_picks_the_smallest_power_of_two(m):
    ops = _ops()
    m = float(torch.tensor(m, dtype=torch.float32))
    x = r32(8, 12, seed=64, scale=0.1)
    x[5, 7] = -m
    split, inv = ops.split_cast_guarded(x.cuda())
    assert math.frexp(inv)[0] == 0.5 and inv >= 1.0                              # a power of two, never an upscale
    assert m / inv <= 8192.0
    assert inv == 1.0 if m <= 8192.0 else m / (inv / 2) > 8192.0                # ... and the smallest that fits
    assert torch.equal(split.cpu(), _split3_ref(x, 1.0 / inv))


@pytest.mark.parametrize("M,K,N", [(300, 64, 64), (256, 320, 320)])              # split K = 192 and 960
def test_split_operands_show_the_gemm_the_fp32_value(M, K, N):
    """[hi | lo | hi] x [w_hi | w_hi | w_lo] = (a_hi + a_lo)(w_hi + w_lo) - a_lo w_lo: the unchanged fp16 GEMM sees both fp32 operands to
    about 2^-21 instead of 2^-11.  Against fp64 the split product must be at least 20 x closer than the fp16-operand one (in theory
    2^-9 x; the rest is the fp32 accumulation over K)."""
    ops = _ops()
    a32, w32 = r32(M, K, seed=65), r32(N, K, seed=66, scale=K ** -0.5)
    ref = a32.double() @ w32.double().t()
    a3, w3 = ops.split_cast(a32.cuda()), ops.split_weight(w32).cuda()
    assert a3.shape == (M, 3 * K) and w3.shape == (N, 3 * K)
    e_split = rel_l2(ops.gemm(a3, w3, out_f32=True), ref)
    e_fp16 = rel_l2(ops.gemm(a32.half().cuda(), w32.half().cuda(), out_f32=True), ref)
    print(f"[split operands {M}x{N}x{K}] split {e_split:.3e}, fp16 operands {e_fp16:.3e}")
    assert e_fp16 > 1e-4 and e_split < 0.05 * e_fp16


# ================================================================================================ C. LayerNorm and row softmax
LN_WIDTHS = [320, 640, 1280, 520]                    # the three multi-row kernels (32 / 16 / 8 rows per wave pass) and the generic one


@pytest.mark.parametrize("rows", [1, 5, 33])
@pytest.mark.parametrize("Cc", LN_WIDTHS)
def test_layernorm_writes_exactly_its_rows(Cc, rows):
    ops = _ops()
    _lib, lib = _raw()
    x = (r16(rows, Cc, seed=24).float() * 2 + 0.5).half()
    g, b = cpu.affine(Cc, seed=25)
    buf = torch.full((rows + 2, Cc), SENTINEL, device="cuda", dtype=torch.float16)
    xd, gd, bd = x.cuda(), g.cuda(), b.cuda()
    _lib.check(lib.icd_layernorm(ops._p(xd), rows, Cc, ops._p(gd), ops._p(bd), 1e-5, ops._p(buf), ops._stream()), "icd_layernorm")
    assert rel_l2(buf[:rows], F.layer_norm(x.double(), (Cc,), g.double(), b.double(), 1e-5)) < TOL
    assert torch.all(buf[rows:] == SENTINEL)


@pytest.mark.parametrize("Cc", LN_WIDTHS)
def test_layernorm_of_constant_and_offset_rows(Cc):
    """The two-pass form is immune to what the raw-sum GroupNorm is not: a constant row gives beta, and rows with mean = 200 std keep the
    tolerances of test_layernorm / test_layernorm_stats (against fp64 here)."""
    ops = _ops()
    rows = 7
    g, b = cpu.affine(Cc, seed=25)
    x = (r16(rows, Cc, seed=24).float() * 2 + 0.5).half()
    x[2] = 3.0
    x[5] = -0.1                                       # (fp16: -0.0999755859375; its sums round)
    out = ops.layernorm(x.cuda(), g.cuda(), b.cuda()).cpu()
    assert torch.isfinite(out).all()
    for r in (2, 5):
        assert float((out[r].double() - b.double()).abs().max()) <= 1e-3
    keep = [0, 1, 3, 4, 6]
    assert rel_l2(out[keep], F.layer_norm(x[keep].double(), (Cc,), g.double(), b.double(), 1e-5)) < TOL
    xo = (r32(rows, Cc, seed=27, scale=0.5) + 100.0).half()                       # mean = 200 std
    xd = xo.double()
    out = ops.layernorm(xo.cuda(), g.cuda(), b.cuda())
    assert rel_l2(out, F.layer_norm(xd, (Cc,), g.double(), b.double(), 1e-5)) < TOL
    st = ops.layernorm_stats(xo.cuda()).cpu().double()
    assert torch.allclose(st[:, 0], xd.mean(1), atol=1e-5, rtol=1e-5)
    assert torch.allclose(st[:, 1], (xd.var(1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-4, atol=0)


SOFTMAX_WIDTHS = [(1, 4),              # a single column
                  (253, 256),          # one float4 per lane
                  (257, 260), (1021, 1024),      # four
                  (1025, 1028), (4093, 4096),    # sixteen
                  (4100, 4100)]        # past the widest register kernel: the generic one, although ld % 4 == 0


def _softmax_guarded(s, cols, ld, scale):
    """icd_softmax_rows through the C ABI with one guard row behind p; returns the rows written."""
    ops = _ops()
    _lib, lib = _raw()
    rows = s.shape[0]
    p = torch.full((rows + 1, ld), SENTINEL, device="cuda", dtype=torch.float16)
    sd = s.cuda()
    _lib.check(lib.icd_softmax_rows(ops._p(sd), rows, cols, ld, scale, ops._p(p), ld, ops._stream()), "icd_softmax_rows")
    assert torch.all(p[rows:] == SENTINEL)
    return p[:rows].cpu()


@pytest.mark.parametrize("rows", [5, 6])
@pytest.mark.parametrize("cols,ld", SOFTMAX_WIDTHS)
def test_softmax_rows_at_every_width_switch(cols, ld, rows):
    s = r32(rows, ld, seed=27, scale=3.0)
    p = _softmax_guarded(s, cols, ld, 0.5)
    assert rel_l2(p[:, :cols], torch.softmax(s[:, :cols].double() * 0.5, -1)) < TOL
    if ld > cols:
        assert float(p[:, cols:].abs().max()) == 0.0


@pytest.mark.parametrize("cols,ld", [(253, 256), (1021, 1024), (4093, 4096), (4100, 4100)])
def test_softmax_rows_subtracts_the_row_maximum(cols, ld):
    """Scores spread over +-80 at scale 1, and the same rows moved by +100 and -100 (softmax does not see a common offset; exp of the raw
    scores overflows in the first and underflows to 0 / 0 in the second)."""
    g = torch.Generator().manual_seed(28)
    s = (torch.rand(5, ld, generator=g) * 160.0 - 80.0)
    s[:, :3] = torch.tensor([80.0, 79.5, 78.0])       # a few entries share the top of each row
    ref = torch.softmax(s[:, :cols].double(), -1)
    for shift in (0.0, 100.0, -100.0):
        p = _softmax_guarded(s + shift, cols, ld, 1.0)
        assert torch.isfinite(p).all() and rel_l2(p[:, :cols], torch.softmax((s + shift)[:, :cols].double(), -1)) < TOL, shift
        assert rel_l2(p[:, :cols], ref) < TOL, shift
        if ld > cols:
            assert float(p[:, cols:].abs().max()) == 0.0


@pytest.mark.parametrize("cols,ld", [(253, 256), (1021, 1024), (4093, 4096), (4100, 4100)])
def test_softmax_rows_with_masked_scores(cols, ld):
    """Half of every row at -inf: those probabilities are exactly zero, the others are the softmax of the rest."""
    s = r32(6, ld, seed=29, scale=3.0)
    mask = torch.rand(6, ld, generator=torch.Generator().manual_seed(30)) < 0.5
    mask[:, 1] = False                                # (never a whole row)
    s[mask] = float("-inf")
    p = _softmax_guarded(s, cols, ld, 0.5)
    assert float(p[:, :cols][mask[:, :cols]].abs().max()) == 0.0
    assert rel_l2(p[:, :cols], torch.softmax(s[:, :cols].double() * 0.5, -1)) < TOL
    if ld > cols:
        assert float(p[:, cols:].abs().max()) == 0.0


# ================================================================================================ D. elementwise entries
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_activation_kinds(kind):
    """silu / x sigmoid(1.702 x) / erf-GELU: rel-L2 over [-12, 12], and on [-4, 4] every value within 2 fp16 ulps of the fp64 one (the fp32
    evaluation of the same formulas meets that on the CPU: test_norm_edges.py; gelu_erf_f is the erf form)."""
    ops = _ops()
    x = cpu.act_inputs(12.0)
    assert rel_l2(ops.activation(x.cuda(), kind), cpu.act_ref64(kind, x)) < TOL
    x = cpu.act_inputs(4.0)
    ref = cpu.act_ref64(kind, x)
    worst = float(((ops.activation(x.cuda(), kind).cpu().double() - ref).abs() / cpu.fp16_ulp(ref)).max())
    print(f"[activation kind {kind}] max error {worst:.2f} fp16 ulps on [-4, 4]")
    assert worst <= 2.0
    if kind == 0:
        assert torch.equal(ops.activation(x.cuda(), 0), ops.silu(x.cuda()))
    with pytest.raises(RuntimeError, match="kind must be"):
        ops.activation(x.cuda(), 3)


def test_embed_tokens_gathers_and_adds_bit_for_bit():
    ops = _ops()
    B, T, Cc, vocab = 3, 7, 24, 11
    tok, pos = r16(vocab, Cc, seed=80), r16(T, Cc, seed=81)                       # (random rows: no two positions alike)
    ids = torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(82))
    ids[0, 0], ids[1, 3], ids[2, T - 1] = 0, vocab - 1, vocab - 1
    ids[0, 5] = 0
    out = ops.embed_tokens(ids.cuda(), tok.cuda(), pos.cuda())
    ref = (tok[ids].float() + pos[None, :, :].float()).half().reshape(B * T, Cc)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("Cc,ones", [(4, -1), (4, 4), (3, 5), (8, -1)])
def test_pack_nchw_layout(Cc, ones, f32):
    ops = _ops()
    B, H, W = 2, 37, 1
    x = r32(B, Cc, H, W, seed=83, scale=2.0)
    x = x if f32 else x.half()
    out = ops.pack_nchw(x.cuda(), ones_channel=ones)
    ref = torch.zeros(B, H * W, 8, dtype=torch.float16)
    ref[:, :, :Cc] = x.reshape(B, Cc, H * W).permute(0, 2, 1).half()
    if ones >= 0:
        ref[:, :, ones] = 1.0
    assert torch.equal(out.cpu(), ref.reshape(B * H * W, 8))
    with pytest.raises(RuntimeError, match="ones channel"):
        ops.pack_nchw(x.cuda(), ones_channel=Cc - 1)                               # a data channel cannot be the ones channel


@pytest.mark.parametrize("act", [0, 1])
def test_split2_act(act):
    """[hi | lo] of an fp32 tensor, raw (bit-exact against the torch split) and behind a SiLU (hi + lo against fp64, within 4 x the rel-L2
    error of torch's fp32 SiLU at the same inputs)."""
    ops = _ops()
    _lib, lib = _raw()
    rows, Cc = 3, 20
    x = cpu.split2_inputs(rows, Cc)
    buf = torch.full((rows + 1, 2 * Cc), SENTINEL, device="cuda", dtype=torch.float16)
    xd = x.cuda()
    _lib.check(lib.icd_split2_act(ops._p(xd), rows, Cc, act, ops._p(buf), ops._stream()), "icd_split2_act")
    assert torch.all(buf[rows:] == SENTINEL)
    hi, lo = buf[:rows, :Cc].cpu(), buf[:rows, Cc:].cpu()
    if act == 0:
        assert torch.equal(hi, x.half()) and torch.equal(lo, (x - x.half().float()).half())
        return
    ref = F.silu(x.double())
    e, e_torch = rel_l2(hi.double() + lo.double(), ref), rel_l2(F.silu(x), ref)
    print(f"[split2_act silu] hi + lo rel-L2 {e:.3e}, torch fp32 SiLU {e_torch:.3e}")
    assert e < 4 * e_torch


def test_sinusoid_f32_timestep_embedding():
    """Kind 0 in fp32: [cos(t f_i) | sin(t f_i)] with f_i the correctly rounded fp32 value of exp(-ln(1e4) i / half) (the kernel's comment
    says why), against fp64 on those frequencies; 4 fp32 ulps of the angle + 1e-6."""
    ops = _ops()
    _lib, lib = _raw()
    dim, half = 320, 160
    t = torch.tensor([0.0, 1.0, 999.0])
    out = torch.full((t.numel() + 1, dim), SENTINEL, device="cuda")
    td = t.cuda()
    _lib.check(lib.icd_sinusoid_f32(ops._p(td), t.numel(), dim, 0, ops._p(out), ops._stream()), "icd_sinusoid_f32")
    assert torch.all(out[t.numel():] == SENTINEL)
    arg = torch.tensor(-9.210340371976184, dtype=torch.float32) * torch.arange(half, dtype=torch.float32) / torch.tensor(float(half))
    f = arg.double().exp().float()
    ang = t.double()[:, None] * f.double()[None, :]
    ref = torch.cat([torch.cos(ang), torch.sin(ang)], -1)
    ulp = torch.exp2(torch.floor(torch.log2(ang.clamp_min(2.0 ** -126))) - 23)
    bound = (4 * ulp + 1e-6).repeat(1, 2)
    err = (out[:t.numel()].cpu().double() - ref).abs()
    print(f"[sinusoid fp32] max error {float(err.max()):.3e}, largest error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(out[0].cpu(), torch.cat([torch.ones(half), torch.zeros(half)]))       # t = 0: cos 0 | sin 0
