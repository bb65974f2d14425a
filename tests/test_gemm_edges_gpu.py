"""The GEMM entry (icd_gemm: csrc/gemm.hip, the big tiles, splitk_reduce_kernel) against plain torch fp64 on the CPU at every tile,
stride and epilogue edge, judged per element.

Every launch goes through one helper: the output lies inside a larger buffer pre-filled with a sentinel (3 extra rows, and 8 columns on
either side where the leading dimension allows) that must come back bit for bit; every strided input is a column slice of a wider tensor
whose other columns and trailing rows are NaN, so a read outside the operand shows as a non-finite result.  The assertion is the
per-element bound that test_gemm_edges.py derives and establishes on the reference alone, plus rel-L2 < TOL; a failure names the worst
(m, n) and its tile.  The case tables, and the plan each case must take, live in test_gemm_edges.py.
"""
import ctypes as C

import pytest
import torch

from conftest import rel_l2
import test_gemm_edges as cpu

pytestmark = pytest.mark.gpu
TOL = 1e-3
SENTINEL = -7.0
NAN = float("nan")


def _ops():
    from invertible_cd_amd import ops
    return ops


def _lib():
    from invertible_cd_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------------- the helper
def slab(t, pad, fill, off=8, rows=3):
    """t [M, W] -> (buffer [M + rows, W + pad] filled with `fill`, its view [M, W] at column `off` holding t), on the device."""
    buf = torch.full((t.shape[0] + rows, t.shape[1] + pad), fill, dtype=t.dtype)
    o = off if pad else 0
    buf[:t.shape[0], o:o + t.shape[1]] = t
    buf = buf.cuda()
    return buf, buf[:t.shape[0], o:o + t.shape[1]]


def out_slab(M, N, pad, dtype):
    buf = torch.full((M + 3, N + pad), SENTINEL, dtype=dtype, device="cuda")
    o = 8 if pad else 0
    return buf, buf[:M, o:o + N]


def guard_intact(buf, view):
    """Everything of `buf` outside `view` still holds the sentinel (uint8 buffers: the sentinel's byte)."""
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    o = view.storage_offset() - buf.storage_offset()
    r0, c0 = o // buf.stride(0), o % buf.stride(0)
    keep[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    return bool((buf[keep] == buf.new_tensor(SENTINEL if buf.dtype.is_floating_point else 0xA5)).all())


def check(section, name, got, ref, bound, tile=(128, 128)):
    got = got.detach().cpu()
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output (a read outside the operand?)"
    ratio, i = cpu.worst(got, ref, bound)
    m, n = divmod(i, ref.shape[-1])
    e = rel_l2(got, ref)
    print(f"[gemm-edges {section}] {name}: worst error / bound {ratio:.3f} at ({m}, {n}), rel-L2 {e:.2e}")
    assert ratio <= 1.0, (f"{name}: |got - ref| = {abs(float(got.flatten()[i]) - float(ref.flatten()[i])):.3e} > bound {float(bound.flatten()[i]):.3e} at "
                          f"(m, n) = ({m}, {n}), tile ({m // tile[0]}, {n // tile[1]}), row {m % tile[0]} / column {n % tile[1]} of it")
    assert e < TOL, (name, e)


def run_dense(section, name, x, flags, tile, *, epi=False, alpha=1.0, pads=None, out_f32=False, resid32=False, out32=False, carry=False,
              geglu=False, ws=1.0):
    """One dense launch of a [M, K] x [N, K]^T problem from cpu.gemm_inputs under guards, checked against fp64.  epi: alpha + bias + fp16
    residual + rowbias; pads: leading dimension minus width per operand (cpu.STRIDE_PAD); carry: resid_carry in and out_carry out;
    ws: fraction of the split-K bytes icd_gemm_workspace_bytes asks for."""
    L, ops = _lib(), _ops()
    pads = pads or {}
    a, w = x["a"], x["w"]
    M, K = a.shape
    N = w.shape[0]
    n_out = N // 2 if geglu else N
    bias = rowbias = resid = rcarry = None
    if epi or geglu:
        bias = x["bias"]
    if epi:
        rowbias = x["rowbias"]
        resid = x["resid"].float() + 0.01 * x["resid"].float() ** 2 if (resid32 or carry) else x["resid"]     # (not an fp16 number)
        if carry:
            resid, rcarry = ops.carry_encode(resid)
    keep = []
    abuf, av = slab(a, pads.get("lda", 0), NAN)
    wsrc = w[ops.geglu_perm(N // 2)].contiguous() if geglu else w
    wbuf, wv = slab(wsrc, pads.get("ldw", 0), NAN)
    obuf, ov = out_slab(M, n_out, pads.get("ldo", 0), torch.float32 if out_f32 else torch.float16)
    d = cpu.dense_desc(M, N, K, flags | (L.ICD_GEMM_OUT_F32 if out_f32 else 0) | (L.ICD_GEMM_GEGLU if geglu else 0),
                       a0=av.data_ptr(), w=wv.data_ptr(), out=ov.data_ptr(), lda=abuf.stride(0), ldw=wbuf.stride(0), ldo=obuf.stride(0), alpha=alpha)
    if bias is not None:
        bsrc = bias[ops.geglu_perm(N // 2)].contiguous() if geglu else bias
        bdev = torch.cat([bsrc, torch.full((8,), NAN)]).cuda()
        d.bias = bdev.data_ptr()
        keep.append(bdev)
    if rowbias is not None:
        rbbuf, rbv = slab(rowbias, pads.get("ld_rowbias", 0), NAN)
        d.rowbias, d.ld_rowbias, d.rows_per_sample = rbv.data_ptr(), rbbuf.stride(0), x["rps"]
    if resid is not None:
        rbuf, rv = slab(resid, pads.get("ldr", 0), NAN)
        d.resid, d.ldr = rv.data_ptr(), rbuf.stride(0)
        if resid.dtype == torch.float32:
            d.flags |= L.ICD_GEMM_RESID_F32
        if rcarry is not None:
            rcbuf, rcv = slab(rcarry, pads.get("ldr", 0), 0x7f)            # (0x7f is an e5m2 NaN: a carry read outside the operand shows)
            d.resid_carry = rcv.data_ptr()
    if out32:
        o32buf, o32v = out_slab(M, n_out, pads.get("ldo", 0), torch.float32)
        d.out_f32 = o32v.data_ptr()
    if carry:
        ocbuf = torch.full(obuf.shape, 0xA5, dtype=torch.uint8, device="cuda")
        ocv = ocbuf[:M, (8 if pads.get("ldo", 0) else 0):][:, :n_out]
        d.out_carry = ocv.data_ptr()
    nbytes = int(cpu.ws_bytes(M, N, K) * ws)
    if nbytes:
        wsbuf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        d.splitk_ws, d.splitk_ws_bytes = wsbuf.data_ptr(), nbytes
    got_plan = cpu.plan(d)
    _launch(d)
    # ---- reference and bound (computed once per problem and epilogue, shared by the launches that differ in path only)
    key = (M, N, K, alpha, epi, geglu, resid32, carry)
    if key not in _REFS:
        if geglu:
            _REFS[key] = cpu.geglu_ref_bound(a, w, alpha, bias, K)
        else:
            rfull = ops.carry_decode(resid, rcarry) if rcarry is not None else resid
            _REFS[key] = cpu.ref64(a, w, alpha, bias, rowbias, x["rps"], rfull)
    if geglu:
        ref, bound = _REFS[key]
    else:
        ref, S = _REFS[key]
        bound = cpu.bound_f32(ref, S, K) if out_f32 else cpu.bound_f16(ref, S, K)
    check(section, name, ov, ref, bound, tile)
    assert guard_intact(obuf, ov), f"{name}: the output guard was written"
    if out32:
        check(section, name + " out_f32", o32v, ref, cpu.bound_f32(ref, S, K), tile)
        assert guard_intact(o32buf, o32v), f"{name}: the guard of out_f32 was written"
        assert torch.equal(ov, o32v.half()), f"{name}: out is not the fp16 rounding of out_f32"
    if carry:
        check(section, name + " carried", ops.carry_decode(ov, ocv), ref, cpu.bound_carry(ref, S, K), tile)
        assert guard_intact(ocbuf, ocv), f"{name}: the guard of out_carry was written"
    return got_plan


def _launch(d, what="icd_gemm"):
    L = _lib()
    L.check(L.load().icd_gemm(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), what)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                           # a device error poisons the context: launch nothing more in this session
        pytest.exit(f"{what}: device error after the launch, stopping the session: {e}", returncode=3)


_INPUTS, _REFS = {}, {}


def inputs(M, N, K):
    if (M, N, K) not in _INPUTS:
        _INPUTS[(M, N, K)] = cpu.gemm_inputs(M, N, K)
    return _INPUTS[(M, N, K)]


# ============================================================================== A. tile edges of the 128-wide dense kernels
@pytest.mark.parametrize("flags,tm", cpu.HEIGHTS, ids=["128x128", "256x128"])
@pytest.mark.parametrize("M,N,K", cpu.TILE_CASES)
def test_tile_edges_plain_and_full_epilogue(M, N, K, flags, tm):
    x = inputs(M, N, K)
    assert run_dense("A", f"{M}x{N}x{K} plain", x, flags, (tm, 128)) == (0, tm, 128, 1)
    assert run_dense("A", f"{M}x{N}x{K} alpha + bias + residual + rowbias", x, flags, (tm, 128), epi=True, alpha=0.5) == (0, tm, 128, 1)


@pytest.mark.parametrize("flags,tm", cpu.HEIGHTS, ids=["128x128", "256x128"])
@pytest.mark.parametrize("M,N,K", cpu.TILE_EXTRA)
def test_tile_edges_every_output_form(M, N, K, flags, tm):
    x = inputs(M, N, K)
    t = (tm, 128)
    run_dense("A", f"{M}x{N}x{K} fp32 output", x, flags, t, epi=True, alpha=0.5, out_f32=True)
    run_dense("A", f"{M}x{N}x{K} fp32 residual", x, flags, t, epi=True, alpha=0.5, resid32=True)
    run_dense("A", f"{M}x{N}x{K} second output", x, flags, t, epi=True, alpha=0.5, resid32=True, out32=True)
    run_dense("A", f"{M}x{N}x{K} carries", x, flags, t, epi=True, alpha=0.5, carry=True)
    for n in cpu.GEGLU_N:
        run_dense("A", f"{M}x{n}x{K} GEGLU", cpu.gemm_inputs(M, n, K, seed=520), flags, t, geglu=True, alpha=0.5)


# ================================================================================================================== B. strides
@pytest.mark.parametrize("flags,tm", cpu.HEIGHTS, ids=["128x128", "256x128"])
@pytest.mark.parametrize("M,N,K", cpu.TILE_EXTRA)
def test_every_leading_dimension_wider_than_its_operand(M, N, K, flags, tm):
    x = inputs(M, N, K)
    t, p = (tm, 128), cpu.STRIDE_PAD
    run_dense("B", f"{M}x{N}x{K} strided", x, flags, t, epi=True, alpha=0.5, pads=p)
    run_dense("B", f"{M}x{N}x{K} strided, fp32 residual + second output", x, flags, t, epi=True, alpha=0.5, pads=p, resid32=True, out32=True)
    run_dense("B", f"{M}x{N}x{K} strided, carries", x, flags, t, epi=True, alpha=0.5, pads=p, carry=True)
    run_dense("B", f"{M}x{N}x{K} strided, fp32 output", x, flags, t, epi=True, alpha=0.5, pads=p, out_f32=True)


# ================================================================================================================== C. split-K
@pytest.mark.parametrize("shape,want", cpu.SPLIT_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s, _ in cpu.SPLIT_CASES])
def test_split_k_with_a_k_tail_and_the_full_epilogue(shape, want):
    M, N, K = shape
    x = inputs(M, N, K)
    t = want[1:3]
    assert run_dense("C", f"{M}x{N}x{K} split plain", x, 0, t) == want
    assert run_dense("C", f"{M}x{N}x{K} split, full epilogue", x, 0, t, epi=True, alpha=0.5) == want


def test_split_k_reduce_kernel_every_output_form_and_a_short_workspace():
    M, N, K = cpu.SPLIT_EXTRA
    x = inputs(M, N, K)
    t = (128, 128)
    for kw, name in ((dict(resid32=True, out32=True), "fp32 residual + second output"), (dict(carry=True), "carries"), (dict(out_f32=True), "fp32 output"),
                     (dict(pads=dict(ldo=16)), "ldo > N"), (dict(pads=cpu.STRIDE_PAD, carry=True), "every stride, carries")):
        assert run_dense("C", f"{M}x{N}x{K} split, {name}", x, 0, t, epi=True, alpha=0.5, **kw)[3] == 2
    # half the workspace, and none: the planner lowers the split, the values still meet the bound (another summation order, not equality)
    for (shape, frac, ksplit) in cpu.SPLIT_WS_PINS:
        if shape == cpu.SPLIT_EXTRA and frac < 1.0:
            assert run_dense("C", f"{M}x{N}x{K} workspace x {frac}", x, 0, t, epi=True, alpha=0.5, ws=frac)[3] == ksplit
    M, N, K = 127, 128, 8192
    assert run_dense("C", f"{M}x{N}x{K} workspace x 0.5", inputs(M, N, K), 0, t, epi=True, alpha=0.5, ws=0.5)[3] == 4


# ================================================================================ D. transposed output on the 128-wide kernels
def run_trans(name, B, rps, ldo, N, K, flags, tile, alpha=1.0, ln=False):
    L = _lib()
    M = B * rps
    x = inputs(M, N, K)
    a, w = x["a"], x["w"]
    abuf, av = slab(a, 24, NAN)
    wbuf, wv = slab(w, 8, NAN)
    obuf = torch.full((B * N + 3, ldo), SENTINEL, dtype=torch.float16, device="cuda")
    d = cpu.dense_desc(M, N, K, flags | L.ICD_GEMM_OUT_TRANS, a0=av.data_ptr(), w=wv.data_ptr(), out=obuf.data_ptr(), lda=abuf.stride(0),
                       ldw=wbuf.stride(0), ldo=ldo, rows_per_sample=rps, alpha=alpha)
    ref, S = cpu.ref64(a, w, alpha)
    if ln:
        mean = a.double().mean(1)
        rstd = (a.double().var(1, unbiased=False) + 1e-5).rsqrt()
        stats = torch.stack([mean, rstd], 1).float().contiguous()
        colsum = w.double().sum(1).float()
        sdev, cdev = stats.cuda(), colsum.cuda()
        d.ln_stats, d.ln_colsum = sdev.data_ptr(), cdev.data_ptr()
        ref = stats[:, 1:2].double() * (ref - stats[:, 0:1].double() * colsum.double()[None, :])
    got_plan = cpu.plan(d)
    _launch(d, "icd_gemm(transposed)")
    out = obuf[:B * N].reshape(B, N, ldo)
    got = out[:, :, :rps].permute(0, 2, 1).reshape(M, N)                # back to [m, n]
    if ln:
        assert torch.isfinite(got).all() and rel_l2(got, ref) < TOL, name
    else:
        check("D", name, got, ref, cpu.bound_f16(ref, S, K), tile)
    assert bool((out[:, :, rps:] == 0).all()), f"{name}: columns [rps, ldo) are not zero"
    assert bool((obuf[B * N:] == SENTINEL).all()), f"{name}: the output guard was written"
    return got_plan


@pytest.mark.parametrize("flags,tm", cpu.HEIGHTS, ids=["128x128", "256x128"])
@pytest.mark.parametrize("B,rps,ldo", cpu.TRANS_CASES)
def test_transposed_output_vector_and_scalar_paths(B, rps, ldo, flags, tm):
    for N in cpu.TRANS_N:
        assert run_trans(f"V^T B={B} rps={rps} ldo={ldo} N={N}", B, rps, ldo, N, cpu.TRANS_K, flags, (tm, 128)) == (0, tm, 128, 1)
    if (B, rps, ldo) == (2, 100, 104):
        run_trans(f"V^T B={B} rps={rps} ldo={ldo} alpha 0.25", B, rps, ldo, 136, cpu.TRANS_K, flags, (tm, 128), alpha=0.25)
        run_trans(f"V^T B={B} rps={rps} ldo={ldo} fused LayerNorm", B, rps, ldo, 136, cpu.TRANS_K, flags, (tm, 128), ln=True)


@pytest.mark.parametrize("c,kernel", cpu.TRANS_BIG, ids=["big tile", "pad columns", "ragged samples"])
def test_transposed_output_big_tile_and_its_fallbacks(c, kernel):
    B = -(-c["M"] // c["rps"])
    if c["M"] % c["rps"]:                              # (1024 rows of 77-row samples: the last sample is partial; its row block still exists)
        L = _lib()
        x = inputs(c["M"], c["N"], c["K"])
        abuf, av = slab(x["a"], 0, NAN)
        obuf = torch.full((B * c["N"] + 3, c["ldo"]), SENTINEL, dtype=torch.float16, device="cuda")
        wdev = slab(x["w"], 0, NAN)[0]
        d = cpu.dense_desc(c["M"], c["N"], c["K"], cpu.FORCE_BIG | L.ICD_GEMM_OUT_TRANS, a0=av.data_ptr(), w=wdev.data_ptr(), out=obuf.data_ptr(),
                           ldo=c["ldo"], rows_per_sample=c["rps"])
        assert cpu.plan(d)[0] == kernel
        _launch(d)
        ref, S = cpu.ref64(x["a"], x["w"])
        bound = cpu.bound_f16(ref, S, c["K"])
        out = obuf[:B * c["N"]].reshape(B, c["N"], c["ldo"]).cpu()
        for b in range(B):
            rows = min(c["rps"], c["M"] - b * c["rps"])
            sl = slice(b * c["rps"], b * c["rps"] + rows)
            check("D", f"V^T 1024x1280x320 rps 77, sample {b}", out[b, :, :rows].t(), ref[sl], bound[sl])
            if rows == c["rps"]:
                assert bool((out[b, :, rows:] == 0).all())
        assert bool((obuf[B * c["N"]:] == SENTINEL).all())
        return
    got = run_trans(f"V^T {c['M']}x{c['N']}x{c['K']} rps={c['rps']} ldo={c['ldo']} FORCE_BIG", B, c["rps"], c["ldo"], c["N"], c["K"], cpu.FORCE_BIG,
                    (256, 256) if kernel else (128, 128))
    assert got[0] == kernel


# ============================================================================================================= E. batched mode
def _att_data(Nq, dh):
    B, H, Nk = cpu.ATT_B, cpu.ATT_H, cpu.ATT_NK
    q, k, v = cpu.r16(B * Nq, H * dh, seed=600), cpu.r16(B * Nk, H * dh, seed=601), cpu.r16(B * Nk, H * dh, seed=602)
    return q, k, v


@pytest.mark.parametrize("dh", cpu.ATT_D)
@pytest.mark.parametrize("ld", cpu.ATT_LD)
@pytest.mark.parametrize("Nq", cpu.ATT_NQ)
def test_batched_scores_and_apply(Nq, ld, dh):
    ops, L = _ops(), _lib()
    B, H, Nk = cpu.ATT_B, cpu.ATT_H, cpu.ATT_NK
    q, k, v = _att_data(Nq, dh)
    scale = dh ** -0.5
    # ---- scores: q and k are column slices of wider NaN-padded matrices, three NaN rows behind every sample's keys (row Nk is never read)
    qbuf, qv = slab(q, 24, NAN)
    kpad = torch.full((B, Nk + 3, H * dh + 8), NAN, dtype=torch.float16)
    kpad[:, :Nk, 8:] = k.reshape(B, Nk, H * dh)
    kdev = kpad.cuda()
    sbuf = torch.full((B * H * Nq + 3, ld), SENTINEL, dtype=torch.float32, device="cuda")
    d = cpu.scores_desc(Nq, dh, ld, ldq=qbuf.stride(0), ldk=kdev.stride(1), k_rows=Nk + 3, a0=qv.data_ptr(), w=kdev[0, 0, 8:].data_ptr(),
                        out=sbuf.data_ptr())
    assert cpu.plan(d) == (0, 128, 128, 1)
    _launch(d, "icd_gemm(QK^T)")
    s = sbuf[:B * H * Nq].reshape(B * H, Nq, ld)
    q64 = q.double().reshape(B, Nq, H, dh).permute(0, 2, 1, 3).reshape(B * H, Nq, dh)
    k64 = k.double().reshape(B, Nk, H, dh).permute(0, 2, 1, 3).reshape(B * H, Nk, dh)
    v64 = v.double().reshape(B, Nk, H, dh).permute(0, 2, 1, 3).reshape(B * H, Nk, dh)
    ref = scale * q64 @ k64.transpose(1, 2)
    S = scale * q64.abs() @ k64.abs().transpose(1, 2)
    check("E", f"scores Nq={Nq} ld={ld} d={dh}", s[:, :, :Nk].reshape(-1, Nk), ref.reshape(-1, Nk), cpu.bound_f32(ref, S, dh).reshape(-1, Nk))
    assert bool((s[:, :, Nk:] == 0).all()), "columns [Nk, ld) of the scores are not exactly zero"
    assert bool((sbuf[B * H * Nq:] == SENTINEL).all())
    if (ld, dh) == (80, 40):                           # the front end builds the same launch: bit for bit
        assert torch.equal(ops.attention_scores(q.cuda(), k.cuda(), B, H, Nq, Nk, dh, scale, ld), s)
    # ---- apply: P [B*H, Nq, ld] fp16 with zero pad columns, V^T a column slice of [B, H*d, ld + 16] (pad keys zero, NaN outside)
    p = torch.zeros(B * H, Nq, ld, dtype=torch.float16)
    p[:, :, :Nk] = torch.softmax(ref, -1).half()
    vt = torch.full((B, H * dh + 3, ld + 16), NAN, dtype=torch.float16)
    vt[:, :H * dh, 8:8 + ld] = 0
    vt[:, :H * dh, 8:8 + Nk] = v.reshape(B, Nk, H * dh).permute(0, 2, 1)
    vdev, pdev = vt.cuda(), p.cuda()
    obuf, ov = out_slab(B * Nq, H * dh, 16, torch.float16)
    d = cpu.apply_desc(Nq, dh, ld, ldvt=vdev.stride(1), ldo=obuf.stride(0), a0=pdev.data_ptr(), w=vdev[0, 0, 8:].data_ptr(), out=ov.data_ptr(),
                       w_bs0=vdev.stride(0))
    assert cpu.plan(d) == (0, 128, 128, 1)
    _launch(d, "icd_gemm(PV)")
    ref = (p[:, :, :Nk].double() @ v64).reshape(B, H, Nq, dh).permute(0, 2, 1, 3).reshape(B * Nq, H * dh)
    S = (p[:, :, :Nk].double() @ v64.abs()).reshape(B, H, Nq, dh).permute(0, 2, 1, 3).reshape(B * Nq, H * dh)
    check("E", f"apply Nq={Nq} ld={ld} d={dh}", ov, ref, cpu.bound_f16(ref, S, ld))
    assert guard_intact(obuf, ov)
    if (ld, dh) == (80, 40):
        vplain = vt[:, :H * dh, 8:8 + ld].contiguous().cuda()
        assert torch.equal(ops.attention_apply(pdev, vplain, B, H, Nq, dh), ov)


@pytest.mark.parametrize("zdiv_is_batch", [False, True], ids=["zdiv 1", "zdiv batch"])
def test_raw_batched_descriptor(zdiv_is_batch):
    """Z = 5 independent 129 x 136 x 72 products: with zdiv = 1 the batch index walks the *_bs0 strides, with zdiv = batch the *_bs1 ones
    (the unused set is poisoned with a stride that would leave the buffers)."""
    Z, M, N, K = 5, 129, 136, 72
    a, w = cpu.r16(Z * M, K, seed=610), cpu.r16(Z * N, K, seed=611, scale=K ** -0.5)
    abuf, av = slab(a, 24, NAN)
    wbuf, wv = slab(w, 8, NAN)
    obuf, ov = out_slab(Z * M, N, 16, torch.float16)
    st = dict(a=M * abuf.stride(0), w=N * wbuf.stride(0), o=M * obuf.stride(0))
    big = 1 << 40
    bs = {f"{t}_bs{1 if zdiv_is_batch else 0}": st[t] for t in "awo"}
    bs.update({f"{t}_bs{0 if zdiv_is_batch else 1}": big for t in "awo"})
    d = cpu.dense_desc(M, N, K, 0, a0=av.data_ptr(), w=wv.data_ptr(), out=ov.data_ptr(), lda=abuf.stride(0), ldw=wbuf.stride(0), ldo=obuf.stride(0),
                       batch=Z, zdiv=Z if zdiv_is_batch else 1, alpha=0.5, **bs)
    assert cpu.plan(d) == (0, 128, 128, 1)
    _launch(d)
    a64, w64 = a.double().reshape(Z, M, K), w.double().reshape(Z, N, K)
    ref = (0.5 * a64 @ w64.transpose(1, 2)).reshape(Z * M, N)
    S = (0.5 * a64.abs() @ w64.abs().transpose(1, 2)).reshape(Z * M, N)
    check("E", f"raw batched zdiv={'batch' if zdiv_is_batch else 1}", ov, ref, cpu.bound_f16(ref, S, K))
    assert guard_intact(obuf, ov)


def test_attention_apply_refuses_a_head_dim_off_the_8_column_grid():
    ops = _ops()
    p, vt = torch.zeros(2, 4, 8, dtype=torch.float16, device="cuda"), torch.zeros(1, 24, 8, dtype=torch.float16, device="cuda")
    with pytest.raises(AssertionError, match="multiple of 8"):
        ops.attention_apply(p, vt, 1, 2, 4, 12)


# ============================================================================================ F. every big-tile configuration
@pytest.mark.parametrize("cfg_i", range(len(cpu.BIG_TILES)))
def test_big_tile_configurations_under_strides_and_guards(cfg_i):
    M, N, K = cpu.BIG_SHAPE
    bm, bn, geglu_ok = cpu.BIG_TILES[cfg_i]
    x = inputs(M, N, K)
    flag, t = cpu.big_cfg(cfg_i), (bm, bn)
    assert run_dense("F", f"cfg {cfg_i} ({bm}x{bn}) full epilogue, strided", x, flag, t, epi=True, alpha=0.5, pads=cpu.BIG_PAD) == (1, bm, bn, 1)
    assert run_dense("F", f"cfg {cfg_i} ({bm}x{bn}) plain, strided", x, flag, t, pads=cpu.BIG_PAD) == (1, bm, bn, 1)
    if geglu_ok:
        assert run_dense("F", f"cfg {cfg_i} ({bm}x{bn}) GEGLU", x, flag, (bm, bn // 2), geglu=True, alpha=0.5, pads=cpu.BIG_PAD) == (1, bm, bn, 1)
    if cfg_i in (0, 4):
        assert run_dense("F", f"cfg {cfg_i} carries", x, flag, t, epi=True, alpha=0.5, pads=cpu.BIG_PAD, carry=True) == (1, bm, bn, 1)
        assert run_dense("F", f"cfg {cfg_i} second output", x, flag, t, epi=True, alpha=0.5, pads=cpu.BIG_PAD, resid32=True, out32=True) == (1, bm, bn, 1)


# ================================================================================================================ G. conv mode
def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def run_conv(name, c, flags, want, tap_base=None, obuf=None):
    ops = _ops()
    B, H, W, C0, C1, Co = c["B"], c["H"], c["W"], c["C0"], c["C1"], c["Co"]
    Cin, stride = C0 + C1, c.get("stride", 1)
    x = cpu.r16(B, Cin, H, W, seed=700)
    taps = 9 if tap_base is None else 4
    bias = torch.randn(Co, generator=torch.Generator().manual_seed(702))
    if tap_base is None:
        w4 = cpu.r16(Co, Cin, 3, 3, seed=701, scale=(9 * Cin) ** -0.5)
        wq = ops.pack_conv_weight(w4)
    else:
        wq = cpu.r16(Co, 4 * Cin, seed=701 + tap_base, scale=(4 * Cin) ** -0.5)
        w4 = cpu.phase_weight_3x3(wq, Cin, tap_base)
    ref, S = cpu.conv_ref64(x, w4, stride, bias)
    xs = _nhwc(x)
    x0buf, _ = slab(xs[:, :C0].contiguous(), 0, NAN)                   # (three NaN rows behind each source)
    x1buf = slab(xs[:, C0:].contiguous(), 0, NAN)[0] if C1 else None
    wdev, bdev = slab(wq, 0, NAN)[0], bias.cuda()
    M = ref.shape[0]
    rows_out = M if tap_base is None else 4 * M
    if obuf is None:
        obuf = torch.full((rows_out + 3, Co), SENTINEL, dtype=torch.float16, device="cuda")
    d = cpu.conv_desc(c, flags, tap_base, a0=x0buf.data_ptr(), a1=x1buf.data_ptr() if C1 else None, w=wdev.data_ptr(), out=obuf.data_ptr(),
                      bias=bdev.data_ptr())
    assert d.K == taps * Cin and cpu.plan(d) == want
    before = obuf.clone()
    _launch(d, "icd_gemm(conv)")
    if tap_base is None:
        rows = torch.arange(M)
    else:                                               # GEMM row (b, y, x) -> pixel (2y + py, 2x + px) of the [B, 2H, 2W] output
        py, px = tap_base // 3, tap_base % 3
        b, y, xx = torch.arange(B)[:, None, None], torch.arange(H)[None, :, None], torch.arange(W)[None, None, :]
        rows = (b * 4 * H * W + (2 * y + py) * 2 * W + 2 * xx + px).reshape(-1)
    check("G", name, obuf[rows.cuda()], ref, cpu.bound_f16(ref, S, taps * Cin), want[1:3])
    other = torch.ones(obuf.shape[0], dtype=torch.bool)
    other[rows] = False
    assert torch.equal(obuf[other.cuda()], before[other.cuda()]), f"{name}: rows outside this launch's were written"
    return obuf


@pytest.mark.parametrize("flags,tm", cpu.HEIGHTS, ids=["128x128", "256x128"])
@pytest.mark.parametrize("c", cpu.CONV_FAST, ids=["stride 1", "stride 2"])
def test_conv_fast_loader_under_guards(c, flags, tm):
    run_conv(f"conv fast loader stride {c['stride']}", c, flags, (0, tm, 128, 1))


def test_conv_general_loader_under_guards():
    run_conv("conv general loader, two sources", cpu.CONV_GENERAL, 0, (0, 128, 128, 1))


def test_conv_phase_form_writes_its_own_rows_only():
    obuf = None
    for t0 in cpu.PHASE_TAP_BASE:                       # each launch must leave the three other phases' rows (and the guard) bit for bit
        obuf = run_conv(f"conv phase form, tap base {t0}", cpu.CONV_PHASE, 0, (0, 128, 128, 1), tap_base=t0, obuf=obuf)
    assert bool((obuf[:-3] != SENTINEL).all())          # the four phases cover every pixel
