"""The spatial kernels outside icd_gemm (csrc/elementwise.hip: icd_conv_in, icd_conv_out_n, icd_x0_step, icd_sinusoid / icd_sinusoid_f32;
csrc/inception.hip: icd_conv2d, icd_pool3x3, icd_global_avgpool) against plain torch fp64 on the CPU, judged per element at every dispatch
edge.  The case tables, the references, the conditions on the inputs and the bounds live in test_conv_edges.py.

Every launch goes through the C entry: every input lies between guard rows of NaN (and, where it is a column slice, NaN columns), weight
rows the header calls ignored are NaN, the bias is followed by NaN; every output lies inside a larger buffer of sentinels that must come
back bit for bit.  Convolutions: equality on the exact inputs (fp32 output == fp64 reference cast to fp32, fp16 output == the reference
rounded once), worst error / bound <= 1 under bound_f16 / bound_f32 on the random inputs (K <= 1032).  Poolings, global average, boundary
step: equality.  Sinusoids: 4 x the figure test_conv_edges.py measures on the fp32 expression, + half an fp16 ulp for the fp16 entry.
"""
import pytest
import torch

import test_conv_edges as cpu

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
NAN = float("nan")
G = 64                                               # guard rows (2-D operands) / guard elements (flat ones) on either side

TOTALS = {}                                          # entry -> [launches compared for equality, launches under a bound, worst ratio]


def _lib():
    from invertible_cd_amd import _lib
    return _lib.load()


def _ok(status, what):
    from invertible_cd_amd import _lib
    _lib.check(status, what)


def _tally(entry, exact=0, bounded=0, ratio=0.0):
    t = TOTALS.setdefault(entry, [0, 0, 0.0])
    t[0], t[1], t[2] = t[0] + exact, t[1] + bounded, max(t[2], ratio)


@pytest.fixture(scope="module", autouse=True)
def _print_totals():
    yield
    for entry, (ne, nb, r) in TOTALS.items():
        print(f"\n[conv-edges] {entry}: {ne} launches compared for equality, {nb} under a bound, worst error / bound {r:.3f}", end="")
    print()


# ------------------------------------------------------------------------------------------------------------------- the guards
def rows_in_nan(t, dtype, pad=0):
    """t [R, Wd] (CPU) -> (device buffer [R + 2 G, Wd + pad] of NaN, its view [R, Wd] at row G holding t)."""
    buf = torch.full((t.shape[0] + 2 * G, t.shape[1] + pad), NAN, dtype=dtype)
    buf[G:G + t.shape[0], :t.shape[1]] = t.to(dtype)
    buf = buf.cuda()
    return buf, buf[G:G + t.shape[0], :t.shape[1]]


def flat_in_nan(t, dtype):
    buf = torch.full((t.numel() + 2 * G,), NAN, dtype=dtype)
    buf[G:G + t.numel()] = t.flatten().to(dtype)
    buf = buf.cuda()
    return buf, buf[G:G + t.numel()]


def out_flat(n, dtype):
    buf = torch.full((n + 2 * G,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[G:G + n]


def out_rows(R, n, ldo, col_off, dtype=torch.float16):
    """(buffer [R + 2 G, ldo] of sentinels, the [R, ldo] rows the entry is given, the [R, n] slice it may write)."""
    buf = torch.full((R + 2 * G, ldo), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[G:G + R], buf[G:G + R, col_off:col_off + n]


def sentinels_intact(buf, view):
    """Everything of `buf` outside `view` (a slice of it) still holds the sentinel."""
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    o = view.storage_offset() - buf.storage_offset()
    if buf.dim() == 1:
        keep[o:o + view.numel()] = False
    else:
        r0, c0 = divmod(o, buf.stride(0))
        keep[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    return bool((buf[keep] == SENTINEL).all())


def judge(entry, name, kind, got, ref, S, K, f32):
    """One launch: finite, then equality (exact inputs) or the bound (random inputs).  Returns the ratio (0 for equality)."""
    got = got.detach().cpu()
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output (a read outside the operand, or of an ignored weight row)"
    if kind == "exact":
        cpu.assert_exact(got, ref, name)
        _tally(entry, exact=1)
        return 0.0
    bound = cpu.bound_of(f32, ref, S, K)
    r, i = cpu.worst(got, ref, bound)
    assert r <= 1.0, (f"{name}: |got - ref| = {abs(float(got.flatten()[i]) - float(ref.flatten()[i])):.3e} > bound {float(bound.flatten()[i]):.3e} at "
                      f"flat index {i} {tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))}")
    _tally(entry, bounded=1, ratio=r)
    return r


def kinds_for(K):
    return ("exact", "random") if K <= cpu.K_RANDOM_MAX else ("exact",)


# ----------------------------------------------------------------------------------------------------------------- icd_conv_out_n
@pytest.mark.parametrize("cin,geom", cpu.conv_out_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_conv_out_every_form_per_element(cin, geom):
    """Cout 1..4 x fp16 / fp32 output x bias / NULL at one (Cin, geometry): 16 launches per kind of input.  Weight rows >= Cout are NaN.
    Measured on the MI355X: every exact launch equal; random inputs (the 8- and 16-lane forms) worst error / bound 0.949."""
    lib, (B, H, W) = _lib(), geom
    for kind in kinds_for(9 * cin):
        p = cpu.conv_out_problem(kind, cin, geom)
        xbuf, xv = rows_in_nan(p["x"].reshape(B * H * W, cin), torch.float16)
        worst = 0.0
        for cout, f32, with_bias in cpu.CO_VARIANTS:
            w4 = torch.full((4, 9 * cin), NAN, dtype=torch.float16)
            w4[:cout] = p["w"][:cout].reshape(cout, 9 * cin).half()
            wdev = w4.cuda()
            bdev = torch.cat([p["bias"][:cout].float(), torch.full((8,), NAN)]).cuda() if with_bias else None
            obuf, ov = out_flat(B * cout * H * W, torch.float32 if f32 else torch.float16)
            _ok(lib.icd_conv_out_n(xv.data_ptr(), B, H, W, cin, wdev.data_ptr(), bdev.data_ptr() if with_bias else None, cout, ov.data_ptr(),
                                   int(f32), None), "icd_conv_out_n")
            ref, S = cpu.conv_out_ref(p, cout, with_bias)
            name = f"conv_out {kind} Cin {cin} ({cpu.CO_CIN[cin]}) {geom} Cout {cout} {'fp32' if f32 else 'fp16'} bias {with_bias}"
            worst = max(worst, judge("icd_conv_out_n", name, kind, ov.reshape(B, cout, H, W), ref, S, p["K"], f32))
            assert sentinels_intact(obuf, ov), f"{name}: wrote outside the output"
        print(f"[conv-edges conv_out_n] Cin {cin} ({cpu.CO_CIN[cin]}) {geom} {kind}: {len(cpu.CO_VARIANTS)} launches, "
              + ("all equal" if kind == "exact" else f"worst error / bound {worst:.3f}"))


# -------------------------------------------------------------------------------------------------------------------- icd_conv_in
@pytest.mark.parametrize("geom", cpu.CI_GEOMS, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("cout", cpu.CI_COUT)
def test_conv_in_per_element(cout, geom):
    """fp16 / fp32 NCHW input x bias / NULL.  Measured on the MI355X: every exact launch equal; random worst error / bound 0.987."""
    lib, (B, H, W) = _lib(), geom
    for kind in ("exact", "random"):
        worst = 0.0
        for x_f32, with_bias in cpu.CI_VARIANTS:
            p = cpu.conv_in_problem(kind, cout, geom, x_f32)
            xbuf, xv = flat_in_nan(p["x"], torch.float32 if x_f32 else torch.float16)
            wbuf, wv = rows_in_nan(p["w"].reshape(cout, 36), torch.float16)
            bdev = torch.cat([p["bias"].float(), torch.full((8,), NAN)]).cuda() if with_bias else None
            obuf, orows, ov = out_rows(B * H * W, cout, cout, 0)
            _ok(lib.icd_conv_in(xv.data_ptr(), int(x_f32), B, H, W, wv.data_ptr(), bdev.data_ptr() if with_bias else None, cout, ov.data_ptr(),
                                None), "icd_conv_in")
            ref, S = cpu.epilogue_ref(p, with_bias)
            name = f"conv_in {kind} Cout {cout} {geom} x {'fp32' if x_f32 else 'fp16'} bias {with_bias}"
            worst = max(worst, judge("icd_conv_in", name, kind, ov, ref, S, 36, False))
            assert sentinels_intact(obuf, ov), f"{name}: wrote outside the output"
        print(f"[conv-edges conv_in] Cout {cout} {geom} {kind}: " + ("all equal" if kind == "exact" else f"worst error / bound {worst:.3f}"))


# --------------------------------------------------------------------------------------------------------------------- icd_conv2d
@pytest.mark.parametrize("i", range(len(cpu.C2D_CASES)), ids=lambda i: str(cpu.C2D_CASES[i]).replace(" ", ""))
def test_conv2d_per_element(i):
    """ldx = Cin and Cin + 24 (NaN in the columns that are not read) x bias / NULL x ReLU on / off, into a column slice under sentinels.
    Measured on the MI355X: every exact launch equal; random worst error / bound 0.995."""
    lib = _lib()
    (kh, kw, s, ph, pw), (B, H, W), cin, n = cpu.C2D_CASES[i]
    for kind in kinds_for(kh * kw * cin):
        p = cpu.conv2d_problem(kind, i)
        M, worst = p["M"], 0.0
        wbuf, wv = rows_in_nan(p["w"].reshape(n, p["K"]), torch.float16)
        bdev = torch.cat([p["bias"].float(), torch.full((8,), NAN)]).cuda()
        for pad in cpu.C2D_LDX_PAD:
            xbuf, xv = rows_in_nan(p["x"].reshape(B * H * W, cin), torch.float16, pad)
            col_off, ldo = (16, n + 24) if pad else (0, n)
            for with_bias, relu in cpu.C2D_VARIANTS:
                obuf, orows, ov = out_rows(M, n, ldo, col_off)
                _ok(lib.icd_conv2d(xv.data_ptr(), xbuf.stride(0), B, H, W, cin, wv.data_ptr(), bdev.data_ptr() if with_bias else None, n, kh, kw,
                                   s, ph, pw, int(relu), orows.data_ptr(), ldo, col_off, None), "icd_conv2d")
                ref, S = cpu.epilogue_ref(p, with_bias, relu)
                name = f"conv2d {kind} {cpu.C2D_CASES[i]} ldx {cin + pad} bias {with_bias} relu {relu}"
                worst = max(worst, judge("icd_conv2d", name, kind, ov, ref, S, p["K"], False))
                assert sentinels_intact(obuf, ov), f"{name}: wrote outside the column slice"
        print(f"[conv-edges conv2d] {cpu.C2D_CASES[i]} M {M} K {p['K']} {kind}: 8 launches, "
              + ("all equal" if kind == "exact" else f"worst error / bound {worst:.3f}"))


# -------------------------------------------------------------------------------------------------------------------- icd_pool3x3
@pytest.mark.parametrize("mode,geom,c", cpu.pool_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_pool3x3_equals_the_reference(mode, geom, c):
    """All three modes bit for bit - the average too: its window sum of integers is exact, and the reference makes the kernel's two
    roundings (fp32 division, then fp16).  Measured on the MI355X: equal in every case."""
    lib, (B, H, W) = _lib(), geom
    x = cpu.pool_input(mode, geom, c)
    want = cpu.pool_ref(mode, x)
    for pad in cpu.POOL_LDX_PAD:
        xbuf, xv = rows_in_nan(x.reshape(B * H * W, c), torch.float16, pad)
        col_off, ldo = (8, c + 24) if pad else (0, c)
        obuf, orows, ov = out_rows(want.shape[0], c, ldo, col_off)
        _ok(lib.icd_pool3x3(xv.data_ptr(), xbuf.stride(0), B, H, W, c, mode, orows.data_ptr(), ldo, col_off, None), "icd_pool3x3")
        got = ov.cpu()
        assert torch.isfinite(got.float()).all(), "non-finite output: a read outside the operand"
        cpu.assert_exact(got, want.double(), f"pool3x3 mode {mode} {geom} C {c} ldx {c + pad}")
        assert sentinels_intact(obuf, ov)
        _tally("icd_pool3x3", exact=1)


# ------------------------------------------------------------------------------------------------------------- icd_global_avgpool
@pytest.mark.parametrize("hw", cpu.GAP_HW)
@pytest.mark.parametrize("c", cpu.GAP_C)
def test_global_avgpool_equals_the_two_rounding_reference(c, hw):
    """Measured on the MI355X: equal in every case."""
    lib = _lib()
    for B in cpu.GAP_B:
        x = cpu.gap_input(B, hw, c)
        xbuf, xv = rows_in_nan(x.reshape(B * hw, c), torch.float16)
        obuf, ov = out_flat(B * c, torch.float32)
        _ok(lib.icd_global_avgpool(xv.data_ptr(), B, hw, c, ov.data_ptr(), None), "icd_global_avgpool")
        cpu.assert_exact(ov.cpu().reshape(B, c), cpu.gap_ref(x).double(), f"global_avgpool B {B} HW {hw} C {c}")
        assert sentinels_intact(obuf, ov)
        _tally("icd_global_avgpool", exact=1)


# -------------------------------------------------------------------------------------------------------------------- icd_x0_step
@pytest.mark.parametrize("per_sample", cpu.X0_PER_SAMPLE)
@pytest.mark.parametrize("flags", cpu.X0_FLAGS)
def test_x0_step_equals_the_fp32_torch_order(flags, per_sample):
    """Three samples with three coefficient rows, every dtype combination.  Measured on the MI355X: equal in every case."""
    lib = _lib()
    x, eps, coef = cpu.x0_inputs(flags, per_sample)
    B = x.shape[0]
    xbuf, xv = flat_in_nan(x, x.dtype)
    ebuf, ev = flat_in_nan(eps, eps.dtype)
    cdev = torch.cat([coef.flatten(), torch.full((8,), NAN)]).cuda()
    obuf, ov = out_flat(B * per_sample, torch.float32 if flags & 4 else torch.float16)
    _ok(lib.icd_x0_step(xv.data_ptr(), ev.data_ptr(), cdev.data_ptr(), B, per_sample, flags, ov.data_ptr(), None), "icd_x0_step")
    got = ov.cpu().reshape(B, per_sample)
    assert torch.isfinite(got.float()).all()
    cpu.assert_exact(got, cpu.x0_ref(x, eps, coef, flags).double(), f"x0_step flags {flags} per_sample {per_sample}")
    assert sentinels_intact(obuf, ov)
    _tally("icd_x0_step", exact=1)


# ------------------------------------------------------------------------------------------------------------------- icd_sinusoid
@pytest.mark.parametrize("kind,dim,n", cpu.sinus_cases())
def test_sinusoids_against_fp64(kind, dim, n):
    """Both entries.  The bound: SIN_MARGIN = 4 times the error of the same expression in torch fp32 (test_conv_edges.py: 3.283 units of
    |angle| 2^-23 + 2^-24 for kind 0, 4.208 for kind 1), + half an fp16 ulp for the fp16 entry.  Measured on the MI355X, worst error /
    bound: icd_sinusoid 0.994 (the half ulp of the fp16 rounding), icd_sinusoid_f32 0.255.  At an odd dim the last column is exactly 0."""
    lib = _lib()
    vals = cpu.SIN_VALS[kind][n]
    ref, ang = cpu.sinus_ref64(vals, dim, kind)
    vdev = torch.cat([torch.tensor(vals, dtype=torch.float32), torch.full((8,), NAN)]).cuda()
    for f32_entry in (False, True):
        entry = "icd_sinusoid_f32" if f32_entry else "icd_sinusoid"
        obuf, ov = out_flat(n * dim, torch.float32 if f32_entry else torch.float16)
        _ok(getattr(lib, entry)(vdev.data_ptr(), n, dim, kind, ov.data_ptr(), None), entry)
        got = ov.cpu().reshape(n, dim)
        assert torch.isfinite(got.float()).all()
        bound = cpu.sinus_bound(ref, ang, kind, f32_entry)
        r, i = cpu.worst(got, ref, bound)
        print(f"[conv-edges sinusoid] {entry} kind {kind} dim {dim} n {n}: worst error / bound {r:.3f} at {divmod(i, dim)}")
        assert r <= 1.0, (entry, kind, dim, n, divmod(i, dim), float(got.flatten()[i]), float(ref.flatten()[i]))
        if dim & 1:
            assert torch.equal(got[:, -1], torch.zeros(n, dtype=got.dtype))
        assert sentinels_intact(obuf, ov)
        _tally(entry, bounded=1, ratio=r)
