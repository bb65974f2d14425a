"""The attention entries (icd_attention_fused_ex: attn_fused_kernel, attn_cross_kernel; icd_attention_probs*: attn_probs_kernel;
icd_attention_masked) against fp64 torch at every dispatch edge, judged per element.

Every launch goes through one helper that calls the C entry directly, so that every stride can be set: q and k are column slices of
wider tensors whose other columns and trailing rows are NaN; V^T is built in torch as [B, C_total, ldvt] with this layer's block at a row
offset, the other rows NaN and the pad columns [Nk, ldvt) zero (the contract of icd_attention_fused); the output lies inside a
sentinel-filled slab that must come back bit for bit outside the view.  The assertion is: finite everywhere, worst error / bound <= 1
with the bound test_attn_edges.py derives and establishes on the reference alone, and the rel-L2 limit of the older tests.  A failure
names (sample, head, query row, column), the query tile and wave of the row and the key tile count.  The case tables and the
instantiation each case must take live in test_attn_edges.py.  References are fp64 torch on the CPU, on the device where P has more
than 2^22 elements.
"""
import ctypes as C

import pytest
import torch

from conftest import rel_l2
import test_attn_edges as cpu

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
NAN = float("nan")
ON_DEVICE = 1 << 22


def _L():
    from invertible_cd_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------------ the helper
def rows_slab(t, pad):
    """t [B, N, W] -> the view [B * N, W] at column 8 of a NaN-filled [B * N + 3, W + pad] device buffer (pad = 0: no column margin)."""
    B, N, W = t.shape
    buf = torch.full((B * N + 3, W + pad), NAN, dtype=t.dtype)
    o = 8 if pad else 0
    buf[:B * N, o:o + W] = t.reshape(B * N, W)
    buf = buf.cuda()
    return buf, buf[:B * N, o:o + W]


def out_slab(M, N, pad, dtype=torch.float16):
    """A sentinel-filled [M + 3, N + pad] buffer and its [M, N] view: 8 columns either side for pad >= 16, and for pad = 4 the view at
    column 4 (an 8-byte but not 16-byte aligned output whose rows follow each other with 4 foreign columns between them)."""
    buf = torch.full((M + 3, N + pad), SENTINEL, dtype=dtype, device="cuda")
    o = 8 if pad >= 16 else pad
    return buf, buf[:M, o:o + N]


def guard_intact(buf, view):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    o = view.storage_offset() - buf.storage_offset()
    r0, c0 = o // buf.stride(0), o % buf.stride(0)
    keep[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    return bool((buf[keep] == SENTINEL).all())


def vt_block(v, H, d, ldvt, rows_before=0, rows_after=0, pad_value=0.0):
    """v [B, Nk, H d] -> (buffer [B, rows_before + H d + rows_after, ldvt], its block view): V^T of this layer, the other rows NaN, the pad
    columns [Nk, ldvt) `pad_value`."""
    B, Nk, Cc = v.shape
    buf = torch.full((B, rows_before + Cc + rows_after, ldvt), NAN, dtype=torch.float16)
    buf[:, rows_before:rows_before + Cc, :Nk] = v.transpose(1, 2)
    buf[:, rows_before:rows_before + Cc, Nk:] = pad_value
    buf = buf.cuda()
    return buf, buf[:, rows_before:rows_before + Cc]


def launch_fused(q, k, v, H, d, scale, flags=0, variants=(), pad_value=0.0, masked_counts=None):
    """One icd_attention_fused_ex launch (icd_attention_masked with masked_counts) under guards -> out [B, Nq, H d] on the CPU.
    variants (cpu.F_VARIANTS): ldq / ldk (16 extra columns, view at column 8), ldo (H d + 4), ldvt8 (Nk rounded up to 8, the default) /
    ldvt64 (64 more: over a tile of zero pad), vtbs (the block at row 24 of a taller buffer: vt_batch_stride > H d ldvt)."""
    L = _L()
    B, Nq, Cc = q.shape
    Nk = k.shape[1]
    qbuf, qv = rows_slab(q, 16 if "ldq" in variants else 0)
    kbuf, kv = rows_slab(k, 16 if "ldk" in variants else 0)
    ldvt = (Nk + 7) // 8 * 8 + (64 if "ldvt64" in variants else 0)
    vbuf, vv = vt_block(v, H, d, ldvt, *((24, 8) if "vtbs" in variants else (0, 0)), pad_value=pad_value)
    obuf, ov = out_slab(B * Nq, Cc, 4 if "ldo" in variants else 0)
    vt_bs = vbuf.stride(0) if "vtbs" in variants else 0
    lib = L.load()
    if masked_counts is None:
        st = lib.icd_attention_fused_ex(qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), ov.data_ptr(), B, H, Nq, Nk, d, qbuf.stride(0), kbuf.stride(0),
                                        ldvt, obuf.stride(0), vt_bs, scale, flags, None)
    else:
        st = lib.icd_attention_masked(qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), ov.data_ptr(), masked_counts.data_ptr(), B, H, Nq, Nk, d,
                                      qbuf.stride(0), kbuf.stride(0), ldvt, obuf.stride(0), vt_bs, scale, None)
    L.check(st, "attention launch")
    torch.cuda.synchronize()
    assert guard_intact(obuf, ov), "the kernel wrote outside its output"
    return ov.cpu().reshape(B, Nq, Cc)


def check(sec, name, got, ref, bound, H, d, Nk, qt=1, quiet=False):
    """finite, per-element bound, rel-L2; returns the worst ratio"""
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output (a read outside the operand?)"
    ratio, i = cpu.worst(got, ref, bound)
    B, Nq, Cc = ref.shape
    b, rem = divmod(i, Nq * Cc)
    n, col = divmod(rem, Cc)
    e = rel_l2(got, ref)
    if not quiet:
        print(f"[attn-edges {sec}] {name}: worst error / bound {ratio:.3f} at (b, h, n, c) = ({b}, {col // d}, {n}, {col % d}), rel-L2 {e:.2e}")
    assert ratio <= 1.0, (f"{name}: |got - ref| = {abs(float(got.flatten()[i]) - float(ref.flatten()[i])):.3e} > bound {float(bound.flatten()[i]):.3e} at "
                          f"sample {b}, head {col // d}, query row {n}, column {col % d}: query tile {n // (128 * qt)}, wave {n % (128 * qt) // (32 * qt)}, "
                          f"row {n % (32 * qt)} of it; {(Nk + 63) // 64} key tiles, {Nk % 64} keys in the last")
    assert e < cpu.TOL, (name, e)
    return ratio


def run_row(r, variants=(), pad_value=0.0, quiet=False, name=None, cache=None):
    """A row of the fused tables: launch, reference (cached per row in `cache`), check.  Returns (got, worst ratio)."""
    q, k, v, c, B, H = cpu.row_case(r)
    d, Nq, Nk = r["d"], r["Nq"], r["Nk"]
    got = launch_fused(q, k, v, H, d, cpu.scale_of(r), r["flags"], variants, pad_value)
    key = id(r)
    if cache is None or key not in cache:
        dev = "cuda" if B * H * Nq * Nk > ON_DEVICE else "cpu"
        rb = cpu.fused_ref_bound(q, k, v, H, d, c, bool(r["flags"] & cpu.CAUSAL), device=dev)
        if cache is not None:
            cache[key] = rb
    else:
        rb = cache[key]
    name = name or f"d={d} Nq={Nq} Nk={Nk} flags={r['flags']}" + (f" {'+'.join(variants)}" if variants else "")
    return got, check(r["sec"], name, got, rb[0], rb[1], H, d, Nk, r["want"][3], quiet)


def _summary(sec, what, ratios):
    print(f"[attn-edges {sec}] {what}: worst error / bound {max(ratios):.3f} over {len(ratios)} launches")


# ------------------------------------------------------------------------------------------------------------------- sections
@pytest.mark.parametrize("flags", [0, cpu.PRESC, cpu.PRESC | cpu.MODE0], ids=["plain", "prescaled", "prescaled-mode0"])
def test_A_head_dim_sweep(flags):
    _summary("A", f"flags={flags}, d = 8 .. 160", [run_row(r, quiet=True)[1] for r in cpu.A_ROWS if r["flags"] == flags])


@pytest.mark.parametrize("d", cpu.B_DIMS)
def test_B_key_count_edges(d):
    _summary("B", f"d={d}, Nk in {cpu.B_NK}, Nq in {cpu.B_NQ}", [run_row(r, quiet=True)[1] for r in cpu.B_ROWS if r["d"] == d])


def _causal_cases():
    return sorted({(r["d"], r["flags"]) for r in cpu.C_ROWS})


@pytest.mark.parametrize("d,flags", _causal_cases())
def test_C_causal(d, flags):
    ratios = []
    for r in cpu.C_ROWS:
        if (r["d"], r["flags"]) != (d, flags):
            continue
        q, k, v, c, B, H = cpu.row_case(r)
        N = r["Nq"]
        cache = {}
        got, ratio = run_row(r, quiet=True, cache=cache)
        ratios.append(ratio)
        # row 0 sees key 0 alone: v_0 to one output rounding (P = 1 exactly, 1 / l = 1: no rounding at all on fp16 data)
        assert torch.equal(got[:, 0], v[:, 0]), f"d={d} N={N}: row 0 is not v_0"
        # row n must not move when the keys after it change: keys / values from n0 + 1 on replaced by huge (finite) ones, rows <= n0 bit
        # for bit.  n0 is the last row of a wave's 32-row tile: WHEN a row is rescaled is decided per wave (one ballot), so a row that
        # shares its wave with rows that do see the new keys keeps its value only up to rounding - those rows (up to n1, mid-tile) are
        # held to the per-element bound of the unchanged reference instead.
        if N > 32:
            n0, n1 = (N - 2) // 32 * 32 - 1, min((N - 2) // 32 * 32 + 7, N - 2)
            k2, v2 = k.clone(), v.clone()
            k2[:, n1 + 1:], v2[:, n1 + 1:] = 3.0e4, -3.0e4
            got2 = launch_fused(q, k2, v2, H, d, cpu.scale_of(r), r["flags"])
            assert torch.equal(got2[:, :n0 + 1], got[:, :n0 + 1]), f"d={d} N={N}: rows <= {n0} moved with the keys after them"
            ref, bound = cache[id(r)]
            check("C", f"d={d} N={N} rows <= {n1} under huge later keys", got2[:, :n1 + 1], ref[:, :n1 + 1], bound[:, :n1 + 1], H, d, N, quiet=True)
    _summary("C", f"d={d} flags={flags}, N in {cpu.C_N}", ratios)


@pytest.mark.parametrize("i", range(len(cpu.D_ROWS)))
def test_D_wide_kernels(i):
    run_row(cpu.D_ROWS[i])


@pytest.mark.parametrize("d", list(cpu.E_KSDT))
def test_E_cross_kernel_small_shapes(d):
    rows = [r for r in cpu.E_ROWS if r["d"] == d]
    _summary("E", f"d={d}, B H = 2048, (Nq, Nk) in {[(r['Nq'], r['Nk']) for r in rows]}", [run_row(r, quiet=True)[1] for r in rows])


@pytest.mark.parametrize("i", range(len(cpu.F_ROWS)))
def test_F_strides(i):
    r = cpu.F_ROWS[i]
    cache = {}
    base, ratio = run_row(r, cache=cache, quiet=True)
    ratios = [ratio]
    for variants in [(x,) for x in cpu.F_VARIANTS] + [tuple(x for x in cpu.F_VARIANTS if x != "ldvt8")]:
        got, ratio = run_row(r, variants, cache=cache, quiet=True)
        ratios.append(ratio)
        assert torch.equal(got, base), f"{r['want']}: {variants} changed the result"       # strides move data, not arithmetic
    # the V^T pad contract (include/icd_amd.h): a finite pad gives the bits of the zero pad
    for variants in ((), ("ldvt64",)):
        got, ratio = run_row(r, variants, pad_value=777.0, cache=cache, quiet=True)
        assert torch.equal(got, base), f"{r['want']}: a finite non-zero V^T pad changed the result ({variants})"
    _summary("F", f"{r['want']} d={r['d']} H={r['H']} Nq={r['Nq']} Nk={r['Nk']}: each stride, all at once, pad 777", ratios)


def _launch_probs(r, q, k, qc, kc, acc0):
    """-> (P [B H, Nq, ldp] as written, acc after or None); P and acc inside sentinel slabs with 3 extra rows"""
    L = _L()
    lib = L.load()
    B, H, Nq, Nk, d, ldp = r["B"], r["H"], r["Nq"], r["Nk"], r["d"], r["ldp"]
    qbuf, qv = rows_slab(q, 16)
    kbuf, kv = rows_slab(k, 16)
    cb = []
    for cr in (qc, kc):
        if cr is None:
            cb.append((None, None))
        else:
            buf = torch.full((cr.shape[0] * cr.shape[1] + 3, cr.shape[2] + 16), 0x7F, dtype=torch.uint8)      # (0x7F: an e5m2 NaN)
            buf[:cr.shape[0] * cr.shape[1], 8:8 + cr.shape[2]] = cr.reshape(-1, cr.shape[2])
            buf = buf.cuda()
            cb.append((buf, buf[:cr.shape[0] * cr.shape[1], 8:8 + cr.shape[2]]))
    pbuf = torch.full((B * H * Nq + 3, ldp), SENTINEL, dtype=torch.float16, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else None
    args = (B, H, Nq, Nk, d, qbuf.stride(0), kbuf.stride(0), ldp, cpu.scale_of(r))
    abuf = None
    b0 = 1
    if r["epi"]:
        abuf = torch.full(((B - b0) * H * Nq + 3, ldp), SENTINEL, dtype=torch.float16)
        abuf[:(B - b0) * H * Nq] = acc0.reshape(-1, ldp)
        abuf = abuf.cuda()
        epi = L.ProbsEpilogue()
        epi.acc, epi.first_cond_sample = abuf.data_ptr(), b0
        st = lib.icd_attention_probs_ex(qv.data_ptr(), ptr(cb[0][1]), kv.data_ptr(), ptr(cb[1][1]), pbuf.data_ptr(), *args, C.byref(epi), None)
    elif r["split"]:
        st = lib.icd_attention_probs_split(qv.data_ptr(), ptr(cb[0][1]), kv.data_ptr(), ptr(cb[1][1]), pbuf.data_ptr(), *args, None)
    else:
        st = lib.icd_attention_probs(qv.data_ptr(), kv.data_ptr(), pbuf.data_ptr(), *args, None)
    L.check(st, "icd_attention_probs")
    torch.cuda.synchronize()
    assert bool((pbuf[B * H * Nq:] == SENTINEL).all()), "rows past the last query of P were written"
    acc = None
    if abuf is not None:
        assert bool((abuf[(B - b0) * H * Nq:] == SENTINEL).all()), "rows past the last query of acc were written"
        acc = abuf[:(B - b0) * H * Nq].cpu().reshape((B - b0) * H, Nq, ldp)
    return pbuf[:B * H * Nq].cpu().reshape(B * H, Nq, ldp), acc


@pytest.mark.parametrize("d", list(cpu.G_KS))
def test_G_probabilities(d):
    ratios = []
    for r in cpu.G_ROWS:
        if r["d"] != d:
            continue
        B, H, Nq, Nk, ldp = r["B"], r["H"], r["Nq"], r["Nk"], r["ldp"]
        q, k, _ = cpu.attn_inputs(B, H, Nq, Nk, d)
        qc = kc = None
        if r["split"]:
            q, qc, k, kc = cpu.split_inputs(q, k, 7)
        acc0 = torch.rand((B - 1) * H, Nq, ldp, generator=torch.Generator().manual_seed(3)).half() if r["epi"] else None
        got, acc = _launch_probs(r, q, k, qc, kc, acc0)
        name = f"d={d} Nq={Nq} Nk={Nk} ldp={ldp} split={r['split']} epi={r['epi']}"
        assert torch.isfinite(got.float()).all(), f"{name}: non-finite probabilities"
        assert bool((got[..., Nk:] == 0).all()), f"{name}: pad columns [Nk, ldp) are not exactly zero"
        P, bound = cpu.probs_ref_bound(q, k, H, d, cpu.scale_of(r) * cpu.LOG2E, qc, kc)
        ratio, i = cpu.worst(got[..., :Nk], P, bound)
        bh, rem = divmod(i, Nq * Nk)
        n, key = divmod(rem, Nk)
        assert ratio <= 1.0, (f"{name}: |got - P| = {abs(float(got[bh, n, key]) - float(P[bh, n, key])):.3e} > bound {float(bound[bh, n, key]):.3e} at sample "
                              f"{bh // H}, head {bh % H}, query row {n} (block {n // 128}, wave {n % 128 // 32}), key {key} (k-tile {key // 32} of {(ldp + 31) // 32})")
        assert rel_l2(got[..., :Nk], P) < cpu.TOL
        assert float((got.double().sum(-1) - 1.0).abs().max()) <= Nk * 2.0 ** -11, f"{name}: a row does not sum to 1"
        if acc is not None:
            # acc += P with torch's fp16 in-place add of the kernel's own P, for the samples from first_cond_sample = 1 on (acc holds no
            # row of sample 0: a block of that sample must not touch it, which the equality over all of acc shows)
            want = acc0.clone()
            want += got[H:]
            assert torch.equal(acc, want), f"{name}: acc is not torch's fp16 acc += P"
        ratios.append(ratio)
    _summary("G", f"d={d} (KS = {cpu.G_KS[d]}): plain, split, acc, split + acc on both sides of ldp <= 96", ratios)


def test_H_masked_attention_at_full_counts_per_element():
    ratios = []
    for r in cpu.H_ROWS:
        B, H, Nq, Nk, d = r["B"], r["H"], r["Nq"], r["Nk"], r["d"]
        q, k, v = cpu.attn_inputs(B, H, Nq, Nk, d)
        counts = torch.full((B,), Nk, dtype=torch.int32, device="cuda")
        got = launch_fused(q, k, v, H, d, d ** -0.5, masked_counts=counts)
        ref, bound = cpu.fused_ref_bound(q, k, v, H, d, d ** -0.5 * cpu.LOG2E)
        ratios.append(check("H", f"icd_attention_masked d={d} Nq={Nq} Nk={Nk}", got, ref, bound, H, d, Nk, quiet=True))
    _summary("H", "icd_attention_masked, d in 24, 56, 88, 120, full counts", ratios)
