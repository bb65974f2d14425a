"""icd_ffn_geglu (csrc/ffn_fused.hip): the GEGLU feed-forward of a transformer block in one launch, per element against fp64 and against
the two launches it replaces (icd_gemm with ICD_GEMM_GEGLU, then the output projection) on the same seeded fp16 inputs.

The bar: both paths round the hidden tensor to fp16 and differ only in fp32 summation order, so the fused result's relative L2 error and
its maximum error in fp16 ulps of the fp64 value may exceed the two-launch path's by at most 1.5 x.  Every output element is compared
(no mask: an output that is exactly zero counts; the padding columns of a wide leading dimension must come back untouched).

The carried output (value = fp16 + 2^-14 * bf8 carry) is held to the bound of the GEMM entry's carry tests (test_gemm_edges.bound_carry),
unwidened, around the fp64 output projection of the fp16 hidden tensor the two-launch path stored.
"""
import ctypes as C
import functools

import pytest
import torch

from conftest import rel_l2
from test_gemm_edges import bound_carry, gelu64
from test_norm_edges import fp16_ulp

from invertible_cd_amd import _lib

pytestmark = pytest.mark.gpu

CH, HID = 320, 1280
M_SET = (32, 96, 128, 160, 4096 + 32)          # one wave, a partial block, one block, a ragged second block, many blocks + a ragged tail
BAR = 1.5


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(7100)
    rn = lambda *s: torch.randn(*s, generator=g)
    w1 = (rn(2 * HID, CH) * CH ** -0.5).half().cuda()          # rows in the interleaved order of ICD_GEMM_GEGLU: 32 value, 32 gate, ...
    w2 = (rn(CH, HID) * HID ** -0.5).half().cuda()
    b1, b2 = (rn(2 * HID) * 0.2).cuda(), (rn(CH) * 0.2).cuda()
    colsum = w1.double().sum(1).float()
    return w1, b1, colsum, w2, b2


@functools.lru_cache(maxsize=None)
def _acts(M):
    g = torch.Generator().manual_seed(7200 + M)
    x = (torch.randn(M, CH, generator=g) * 1.5 + 0.25).half().cuda()
    resid = torch.randn(M, CH, generator=g).half().cuda()
    rc = torch.randint(0, 256, (M, CH), generator=g, dtype=torch.uint8)
    rc[(rc & 0x7C) == 0x7C] = 0                                  # no inf / NaN bytes among the bf8 carries
    return x, resid, rc.cuda()


def carry_decode(c):
    """bf8 e5m2 byte -> its value times 2^-14 (fp64)."""
    return (c.to(torch.int16) << 8).view(torch.float16).double() * 2.0 ** -14


@functools.lru_cache(maxsize=None)
def _reference(M, ln, mode):
    """fp64 on the device: (out, hidden) of the feed-forward from the fp16 inputs; LayerNorm statistics in fp64 (eps 1e-5)."""
    w1, b1, colsum, w2, b2 = _weights()
    x, resid, rc = _acts(M)
    xd = x.double()
    if ln:
        mean = xd.mean(1, keepdim=True)
        xd = (xd - mean) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-5)
    pre = (xd @ w1.double().t() + b1.double()).view(M, HID // 32, 2, 32)
    hidden = (pre[:, :, 0] * gelu64(pre[:, :, 1])).reshape(M, HID)
    r = resid.double() + (carry_decode(rc) if mode == "carry" else 0.0)
    if mode == "twin":
        r = _twin_resid(M).double()
    return hidden @ w2.double().t() + b2.double() + r, hidden


@functools.lru_cache(maxsize=None)
def _twin_resid(M):
    return (_acts(M)[1].float() * 1.0009765625 + 3e-5).contiguous()          # an fp32 residual that is no fp16 number


def _bufs(M, mode, ldo, inplace):
    x, resid, rc = _acts(M)
    out = torch.full((M, ldo), 7.0, dtype=torch.float16, device="cuda")
    oc = torch.full((M, ldo), 0x55, dtype=torch.uint8, device="cuda") if mode == "carry" else None
    o32 = torch.full((M, ldo), 7.0, dtype=torch.float32, device="cuda") if mode == "twin" else None
    ldr = CH
    if mode == "twin":
        r, r_c = _twin_resid(M).clone(), None
        if inplace:
            o32[:, :CH] = r
            r, ldr = o32, ldo
    else:
        r, r_c = resid.clone(), (rc.clone() if mode == "carry" else None)
        if inplace:
            out[:, :CH] = r
            r, ldr = out, ldo
            if mode == "carry":
                oc[:, :CH] = r_c
                r_c = oc
    return out, oc, o32, r, r_c, ldr


def _padded(w, ld):
    """The rows of w at a leading dimension of ld elements; the padding columns are NaN (a kernel that reads one shows it)."""
    wide = torch.full((w.shape[0], ld), float("nan"), dtype=w.dtype, device=w.device)
    wide[:, :w.shape[1]] = w
    return wide


def run_fused(M, ln, mode, ldx=CH, ldo=CH, inplace=False, stats=None, ldw1=CH, ldw2=HID):
    w1, b1, colsum, w2, b2 = _weights()
    if ldw1 != CH:
        w1 = _padded(w1, ldw1)
    if ldw2 != HID:
        w2 = _padded(w2, ldw2)
    x = _acts(M)[0]
    if ldx != CH:
        xw = torch.full((M, ldx), 9.0, dtype=torch.float16, device="cuda")
        xw[:, :CH] = x
        x = xw
    out, oc, o32, r, r_c, ldr = _bufs(M, mode, ldo, inplace)
    st = stats if stats is not None else torch.zeros(M, 2, device="cuda")
    d = _lib.FfnDesc()
    d.x, d.w1, d.b1, d.w2, d.b2, d.resid, d.out = x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), r.data_ptr(), out.data_ptr()
    d.M, d.C, d.hidden, d.ldx, d.ldw1, d.ldw2, d.ldo, d.ldr = M, CH, HID, ldx, ldw1, ldw2, ldo, ldr
    if ln:
        d.ln_stats, d.ln_colsum = st.data_ptr(), colsum.data_ptr()
        d.flags = 0 if stats is not None else _lib.ICD_GEMM_LN_COMPUTE
    if mode == "twin":
        d.flags |= _lib.ICD_GEMM_RESID_F32
        d.out_f32 = o32.data_ptr()
    if mode == "carry":
        d.resid_carry, d.out_carry = r_c.data_ptr(), oc.data_ptr()
    _lib.check(_lib.load().icd_ffn_geglu(C.byref(d), _stream()), "icd_ffn_geglu")
    torch.cuda.synchronize()
    return out, oc, o32, st


def run_pair(M, ln, mode):
    """The two launches the executor issues today, on the same buffers' contents; returns (out, out_carry, out_f32, hidden fp16)."""
    w1, b1, colsum, w2, b2 = _weights()
    x = _acts(M)[0]
    out, oc, o32, r, r_c, ldr = _bufs(M, mode, CH, False)
    hid = torch.empty(M, HID, dtype=torch.float16, device="cuda")
    st = torch.zeros(M, 2, device="cuda")
    lib = _lib.load()
    d = _lib.GemmDesc()
    d.a0, d.w, d.bias, d.out = x.data_ptr(), w1.data_ptr(), b1.data_ptr(), hid.data_ptr()
    d.M, d.N, d.K, d.Nw, d.lda, d.ldw, d.ldo = M, 2 * HID, CH, 2 * HID, CH, CH, HID
    d.mode, d.batch, d.zdiv, d.alpha = 0, 1, 1, 1.0
    d.flags = _lib.ICD_GEMM_GEGLU | (_lib.ICD_GEMM_LN_COMPUTE if ln else 0)
    if ln:
        d.ln_stats, d.ln_colsum = st.data_ptr(), colsum.data_ptr()
    _lib.check(lib.icd_gemm(C.byref(d), _stream()), "icd_gemm(geglu)")
    e = _lib.GemmDesc()
    e.a0, e.w, e.bias, e.resid, e.out = hid.data_ptr(), w2.data_ptr(), b2.data_ptr(), r.data_ptr(), out.data_ptr()
    e.M, e.N, e.K, e.Nw, e.lda, e.ldw, e.ldo, e.ldr = M, CH, HID, CH, HID, HID, CH, ldr
    e.mode, e.batch, e.zdiv, e.alpha = 0, 1, 1, 1.0
    if mode == "twin":
        e.flags = _lib.ICD_GEMM_RESID_F32
        e.out_f32 = o32.data_ptr()
    if mode == "carry":
        e.resid_carry, e.out_carry = r_c.data_ptr(), oc.data_ptr()
    _lib.check(lib.icd_gemm(C.byref(e), _stream()), "icd_gemm(out)")
    torch.cuda.synchronize()
    return out, oc, o32, hid


def _value(out, oc, o32, mode):
    """What the mode hands to the next consumer of the stream, as fp64 [M, CH]."""
    if mode == "twin":
        return o32[:, :CH].double()
    v = out[:, :CH].double()
    return v + carry_decode(oc[:, :CH]) if mode == "carry" else v


def _errors(got, ref):
    return rel_l2(got, ref), float(((got - ref).abs() / fp16_ulp(ref)).max())


def _check_against_pair(tag, M, ln, mode, fused):
    ref, _ = _reference(M, ln, mode)
    pair = run_pair(M, ln, mode)
    for what, sel in (("stream value", lambda t: _value(t[0], t[1], t[2], mode)), ("fp16 out", lambda t: t[0][:, :CH].double())):
        (l2_f, ulp_f), (l2_p, ulp_p) = _errors(sel(fused), ref), _errors(sel(pair), ref)
        print(f"[ffn {tag} M={M} ln={ln} {mode}] {what}: fused rel-L2 {l2_f:.3e} max {ulp_f:.2f} ulp | two launches rel-L2 {l2_p:.3e} max {ulp_p:.2f} ulp "
              f"| ratios {l2_f / l2_p:.3f} {ulp_f / ulp_p:.3f}")
        assert l2_f <= BAR * l2_p and ulp_f <= BAR * ulp_p
    return pair


@pytest.mark.parametrize("mode", ["plain", "carry", "twin"])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("M", M_SET)
def test_fused_ffn_matches_the_two_launches_against_fp64(M, ln, mode):
    fused = run_fused(M, ln, mode)
    pair = _check_against_pair("contiguous", M, ln, mode, fused)
    if ln:                                           # ICD_GEMM_LN_COMPUTE: the statistics are an output, as they are of the GEGLU launch
        x = _acts(M)[0].double()
        want = torch.stack([x.mean(1), 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)], 1)
        assert float((fused[3].double() - want).abs().max() / want.abs().max()) < 1e-5
    if mode == "carry":
        # the bound of the GEMM entry's carry tests, around the output projection of the fp16 hidden tensor (module docstring)
        w2, b2 = _weights()[3], _weights()[4]
        _, resid, rc = _acts(M)
        hid = pair[3].double()
        r = resid.double() + carry_decode(rc)
        ref2 = hid @ w2.double().t() + b2.double() + r
        S = hid.abs() @ w2.double().abs().t() + b2.double().abs() + r.abs()
        bound = bound_carry(ref2, S, HID)
        worst = float(((_value(*fused[:3], "carry") - ref2).abs() / bound).max())
        worst_pair = float(((_value(*pair[:3], "carry") - ref2).abs() / bound).max())
        differ = int((fused[0] != pair[0]).sum()) + int((fused[1] != pair[1]).sum())
        print(f"[ffn carry M={M} ln={ln}] worst |out + carry - ref| / bound = {worst:.3f} (two launches {worst_pair:.3f}; "
              f"{differ} fp16 / carry elements differ between the paths)")
        assert worst <= 1.0


@pytest.mark.parametrize("mode", ["plain", "carry", "twin"])
def test_in_place_wide_leading_dimensions_and_given_statistics(mode):
    """The executor's call: the residual IS the output buffer (h <- h + ff(h)), here also with rows 8 / 24 elements wider than C and the
    LayerNorm statistics handed in instead of computed; the padding columns of every output come back untouched."""
    M = 160
    x = _acts(M)[0].double()
    stats = torch.stack([x.mean(1), 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)], 1).float().contiguous()
    fused = run_fused(M, True, mode, ldx=CH + 8, ldo=CH + 24, inplace=True, stats=stats)
    _check_against_pair("in place, ldx 328, ldo 344", M, True, mode, fused)
    assert bool((fused[0][:, CH:] == 7.0).all())
    if mode == "carry":
        assert bool((fused[1][:, CH:] == 0x55).all())
    if mode == "twin":
        assert bool((fused[2][:, CH:] == 7.0).all())


@pytest.mark.parametrize("mode", ["plain", "carry"])
def test_padded_weight_leading_dimensions(mode):
    """W1 at ldw1 = C + 8 and W2 at ldw2 = hidden + 8, the padding NaN: the same bits as with contiguous weights (the arithmetic is the
    same; only the addresses of the weight chunks move), over two blocks with a ragged tail, and inside the bar against the two launches."""
    M = 160
    fused = run_fused(M, True, mode, ldw1=CH + 8, ldw2=HID + 8)
    plain = run_fused(M, True, mode)
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[3], plain[3]) and bool(torch.isfinite(fused[0]).all())
    if mode == "carry":
        assert torch.equal(fused[1], plain[1])
    _check_against_pair("ldw1 328, ldw2 1288", M, True, mode, fused)


def test_unsupported_arguments_are_refused_before_any_launch():
    w1, b1, colsum, w2, b2 = _weights()
    x = _acts(32)[0]
    out = torch.full((32, CH), 7.0, dtype=torch.float16, device="cuda")
    lib = _lib.load()

    def desc(**kw):
        d = _lib.FfnDesc()
        d.x, d.w1, d.b1, d.w2, d.b2, d.out = x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.data_ptr()
        d.M, d.C, d.hidden, d.ldx, d.ldw1, d.ldw2, d.ldo, d.ldr = 32, CH, HID, CH, CH, HID, CH, CH
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw, word in ((dict(C=640, hidden=2560), b"C = 320"), (dict(C=1280, hidden=5120), b"C = 320"), (dict(M=0), b"positive"),
                     (dict(x=x.data_ptr() + 2), b"aligned"), (dict(out=out.data_ptr() + 8), b"aligned"), (dict(ldo=CH + 4), b"multiples of 8"),
                     (dict(flags=_lib.ICD_GEMM_LN_COMPUTE), b"ln_stats"), (dict(flags=_lib.ICD_GEMM_GEGLU), b"flags"),
                     (dict(ln_colsum=colsum.data_ptr()), b"ln_colsum without")):
        assert lib.icd_ffn_geglu(C.byref(desc(**kw)), _stream()) == -1, kw
        assert word in lib.icd_last_error(), (kw, lib.icd_last_error())
    assert lib.icd_ffn_geglu(None, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                  # nothing ran


def test_full_width_sd15_forward_with_and_without_the_fused_feed_forward():
    """Full-width SD1.5, B = 2 at 64 x 64 latents: option ffn_fusion 0 (two launches) against 1 (icd_ffn_geglu on the five C = 320 blocks).
    The two evaluations differ by fp32 summation order only: the distance the fused cross-attention A/B of test_sdxl_full_gpu.py allows between
    two launch plans of one evaluation (rel-L2 < 2e-3), and not zero - the switch must switch something.  The planner records show the
    ten dense launches of the five feed-forwards becoming five."""
    from invertible_cd_amd import synthetic, unet, unet_config as uc
    cfg = uc.SD15
    m = unet.UNet2DConditionModel(cfg, synthetic.synthetic_state_dict(cfg, seed=2, device="cuda", dtype=torch.float16)).set_precision("fast")
    inp = synthetic.synthetic_inputs(cfg, 2, 64, 64, seed=2, device="cuda")
    kw = dict(encoder_hidden_states=inp["context"].half(), timestep_cond=torch.randn(2, 512, device="cuda").half())
    x = inp["latents"].half()

    def run(mode):
        m.set_option("ffn_fusion", mode)
        _lib.profile_enable(True)
        try:
            eps = m(x, 519, **kw).sample.clone()
            torch.cuda.synchronize()
            return eps, [r for r in _lib.profile_dump() if r[0] == "gemm_dense"]
        finally:
            _lib.profile_enable(False)

    run(0)                                           # (fills the context-projection cache)
    e0, d0 = run(0)
    e1, d1 = run(1)
    e2, d2 = run(2)
    dist = rel_l2(e1, e0)
    print(f"[ffn_fusion 0 -> 1, SD1.5 B=2 64x64] {len(d0)} -> {len(d1)} dense launches; eps distance {dist:.3e}")
    assert torch.isfinite(e1).all() and 0 < dist < 2e-3
    assert len(d0) - len(d1) == 5 and sum(1 for r in d1 if (r[1], r[2], r[3]) == (2 * 4096, CH, HID)) == 5
    assert torch.equal(e2, e0) and len(d2) == len(d0)          # the default keeps the two launches below 65536 tokens
