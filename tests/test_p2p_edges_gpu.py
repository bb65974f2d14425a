"""The prompt-to-prompt kernels (csrc/p2p.hip; the edit epilogue of attn_probs_kernel) against plain torch fp64 on the CPU at every dispatch
edge, judged per element.  Case tables, references, bounds and the conditions on the inputs live in test_p2p_edges.py.

A. icd_p2p_cross_edit_groups: the probabilities lie inside a slab with sentinel rows before and after; the sentinel rows, the base prompts'
   rows and (ld = 104) columns 96 .. 103 must come back bit for bit, the pad columns [nk, min(ld, 96)) zero, the edited rows inside
   bound_f16, and identity / permutation operators exactly.
B. The fused epilogue gives the bits of the plain probabilities followed by the stand-alone edit at ld >= 80; below 80, where the
   stand-alone entry does not go, it is held against the fp64 reference of A on its own plain probabilities.
C. LocalBlend with thresholds in gaps of the fp64 ratios: torch.equal over all elements, through both routes (reduce launch + workspace,
   and the workspace-less C entry), which must agree bit for bit.
D. accumulate: the table entry past one sweep of its capped grid, empty tensors, counts around multiples of 8.
"""
import ctypes as C

import pytest
import torch

import test_p2p_edges as cpu

pytestmark = pytest.mark.gpu
SENTINEL = cpu.SENTINEL


def _ops():
    from invertible_cd_amd import ops
    return ops


def _lib():
    from invertible_cd_amd import _lib
    return _lib


def sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                           # a device error poisons the context: launch nothing more in this session
        pytest.exit(f"{what}: device error after the launch, stopping the session: {e}", returncode=3)


# ======================================================================================================= A. the cross edit
def prob_slab(probs):
    """probs [R, nq, ld] (CPU) -> (device buffer [guard + R * nq + guard, ld] with sentinel guard rows, its [R, nq, ld] view)."""
    R, nq, ld = probs.shape
    g = cpu.GUARD_ROWS
    buf = torch.full((R * nq + 2 * g, ld), SENTINEL, dtype=torch.float16)
    buf[g:g + R * nq] = probs.reshape(R * nq, ld)
    buf = buf.cuda()
    return buf, buf[g:g + R * nq].view(R, nq, ld)


@pytest.mark.parametrize("i", range(len(cpu.CROSS_CASES)))
def test_cross_edit_against_fp64_under_guards(i):
    ops = _ops()
    c = cpu.cross_case(i)
    nk, ld, G, P, heads = c["nk"], c["ld"], c["G"], c["P"], c["heads"]
    name = f"cross edit {i}: rows {c['rows']} ld {ld} nk {nk} P {P} G {G} {'/'.join(sorted(set(c['kinds'])))}"
    buf, view = prob_slab(c["probs"])
    assert ops.p2p_cross_edit_supported(view[:, :, :nk])
    ops.p2p_cross_edit_groups(view[:, :, :nk], G, P, c["At"].cuda(), c["Dp"].cuda())
    sync(name)
    g = cpu.GUARD_ROWS
    out = buf.cpu()
    assert bool((out[:g] == SENTINEL).all()) and bool((out[-g:] == SENTINEL).all()), f"{name}: a sentinel row was written"
    got = out[g:-g].view(c["probs"].shape)
    rows_of = got.reshape(G, P, heads, c["nq"], ld)
    assert torch.equal(rows_of[:, 0], c["probs"].reshape(G, P, heads, c["nq"], ld)[:, 0]), f"{name}: a base prompt's rows changed"
    assert torch.equal(got[:, :, 96:], c["probs"][:, :, 96:]), f"{name}: columns 96 .. of a row changed"
    assert not got[:, :, nk:96].any(), f"{name}: pad columns [nk, min(ld, 96)) are not zero"
    assert torch.isfinite(got.float()).all()
    got_edit, _ = cpu.cross_edit_rows(c, got)
    ratio, at = cpu.worst(got_edit, c["want"], c["bound"])
    print(f"[p2p-edges A] {name}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, (f"{name}: |got - want| = {abs(float(got_edit.flatten()[at]) - float(c['want'].flatten()[at])):.3e} > bound "
                          f"{float(c['bound'].flatten()[at]):.3e} at (row, token) = {divmod(at % (c['rows'] * nk), nk)}")
    cpu.check_exact_kinds(c, got_edit, name)
    if "reweight" in c["kinds"]:
        assert float(got_edit.min()) < -0.1 and float(got_edit.max()) > 1.1


def test_cross_edit_front_end_refuses_views_the_kernel_cannot_take():
    ops = _ops()
    R, nq = 4, 8
    flat = torch.zeros(R * nq * 80 + 8, dtype=torch.float16, device="cuda")
    good = flat[:R * nq * 80].view(R, nq, 80)[:, :, :77]
    assert ops.p2p_cross_edit_supported(good)
    contiguous77 = torch.zeros(R, nq, 77, dtype=torch.float16, device="cuda")
    off_by_two = flat[2:2 + R * nq * 80].view(R, nq, 80)[:, :, :77]                    # 4 bytes off the 16-byte grid
    taller = torch.zeros(R, nq + 1, 80, dtype=torch.float16, device="cuda")[:, :nq, :77]      # stride(0) != nq * ld
    for bad in (contiguous77, off_by_two, taller, good.float(), good[0], good.cpu()):
        assert not ops.p2p_cross_edit_supported(bad)
    At, Dp = ops.p2p_pack_operator(torch.zeros(1, 77, 77, device="cuda"), torch.ones(1, 77, device="cuda"))
    for bad in (contiguous77, off_by_two, taller):
        with pytest.raises(AssertionError):
            ops.p2p_cross_edit_groups(bad, 1, 2, At, Dp)


# ================================================================================================== B. the fused edit epilogue
def run_fused(Nq, Nk, ld, d, G, P, b0, with_acc):
    """-> (plain, fused, acc0, acc, At, Dp, cond): the probabilities without and with the edit (and store) in the epilogue."""
    ops = _ops()
    H, B = cpu.FUSED_H, b0 + G * P
    gen = torch.Generator().manual_seed(Nq + 7 * Nk + 13 * ld + d)
    q = (torch.randn(B * Nq, H * d, generator=gen) * 0.5).half().cuda()
    k = (torch.randn(B * Nk, H * d, generator=gen) * 0.5).half().cuda()
    At, Dp = cpu.fused_operators(G, P, Nk, Nq + ld)
    scale = d ** -0.5
    plain = ops.attention_probs(q, k, B, H, Nq, Nk, d, scale, ld=ld)
    acc0 = (torch.rand((G * P * H, Nq, ld), generator=gen) * 3).half().cuda() if with_acc else None
    acc = acc0.clone() if with_acc else None
    fused = ops.attention_probs(q, k, B, H, Nq, Nk, d, scale, ld=ld, acc=acc, edit=(At.cuda(), Dp.cuda()), first_cond_sample=b0, edit_count=P - 1,
                                group_count=G)
    sync(f"fused edit Nq {Nq} Nk {Nk} ld {ld}")
    return plain, fused, acc0, acc, At, Dp, slice(b0 * H, B * H)


@pytest.mark.parametrize("case", cpu.FUSED_CASES, ids=[f"Nq{c[0]}-Nk{c[1]}-ld{c[2]}-d{c[3]}-G{c[4]}-P{c[5]}" for c in cpu.FUSED_CASES])
def test_fused_edit_epilogue_is_the_plain_probabilities_then_the_stand_alone_edit(case):
    ops = _ops()
    Nq, Nk, ld, d, G, P, b0, with_acc = case
    plain, fused, acc0, acc, At, Dp, cond = run_fused(*case)
    want = plain.clone()
    ops.p2p_cross_edit_groups(want[cond][:, :, :Nk], G, P, At.cuda(), Dp.cuda())
    sync("stand-alone edit")
    assert torch.isfinite(plain).all() and not torch.equal(want, plain)
    assert torch.equal(fused, want)
    if with_acc:
        w = acc0.clone()
        w += want[cond]
        assert torch.equal(acc, w)


@pytest.mark.parametrize("case", cpu.FUSED_NARROW, ids=[f"Nq{c[0]}-Nk{c[1]}-ld{c[2]}-d{c[3]}-G{c[4]}-P{c[5]}" for c in cpu.FUSED_NARROW])
def test_fused_edit_epilogue_below_80_columns_against_fp64(case):
    """`ld < 80` with an edit is HANDLED by attn_probs_kernel (test_p2p_edges.py::test_the_fused_edit_epilogue_handles_every_row_stride_up_to_96
    reads it off the code): the values are held here against the fp64 reference of section A, taken on the kernel's own plain probabilities."""
    Nq, Nk, ld, d, G, P, b0, with_acc = case
    plain, fused, acc0, acc, At, Dp, cond = run_fused(*case)
    H = cpu.FUSED_H
    pc, fc = plain[cond].cpu(), fused[cond].cpu()
    assert torch.isfinite(plain).all() and torch.equal(fused[:b0 * H], plain[:b0 * H])                      # the unrelated samples
    assert torch.equal(fc.reshape(G, P, H, Nq, ld)[:, 0], pc.reshape(G, P, H, Nq, ld)[:, 0])               # every group's base prompt
    assert not fc[:, :, Nk:].any()
    want, bound = cpu.edit_ref64(pc, At, Dp, G, P, Nk)
    got = fc[:, :, :Nk].reshape(G, P, H * Nq, Nk)[:, 1:]
    ratio, _ = cpu.worst(got, want, bound)
    print(f"[p2p-edges B] Nq {Nq} Nk {Nk} ld {ld} d {d} G {G} P {P}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0 and not torch.equal(fc, pc)
    if with_acc:
        w = acc0.clone()
        w += fused[cond]
        assert torch.equal(acc, w)


# ========================================================================================================== C. LocalBlend
def blend_device(c):
    """The case's tensors on the device, once per case: the maps keep their row stride."""
    if "dev" not in c:
        maps = []
        for m in c["maps"]:
            if m.stride(1) == m.shape[2]:
                maps.append(m.cuda())
            else:                                       # a view of a wider NaN-filled buffer
                rows, px, nw = m.shape
                buf = torch.full((rows, px, m.stride(1)), float("nan"), dtype=torch.float16)
                buf[:, :, :nw] = m
                maps.append(buf.cuda()[:, :, :nw])
        c["dev"] = (maps, c["x"].cuda())
    return c["dev"]


def blend_run(c, route, dev=None):
    """One LocalBlend call of a case (test_p2p_edges.blend_case and its kin) -> fp32 [G * P, C, H, W] on the CPU.
    route "ws": ops.local_blend_groups (the reduce launch and its workspace); "direct": icd_local_blend_groups, no workspace."""
    ops, L = _ops(), _lib()
    maps, x = dev or blend_device(c)
    G, P = c["G"], c["P"]
    if route == "ws":
        out = ops.local_blend_groups(maps, c["alpha"], (c["sub"], c["has_sub"]), c["th_pool"], c["th_sub"], c["active"], x, G, res=c["res"])
    else:
        n = len(maps)
        ptrs, heads = (C.c_void_p * n)(*[m.data_ptr() for m in maps]), (C.c_int32 * n)(*[m.shape[0] // (G * P) for m in maps])
        al, als = c["alpha"].float().cuda().contiguous(), c["sub"].float().cuda().contiguous()
        tp, ts = (C.c_float * G)(*c["th_pool"]), (C.c_float * G)(*c["th_sub"])
        fl = (C.c_int32 * G)(*[int(a) | (2 if s else 0) for a, s in zip(c["active"], c["has_sub"])])
        out = torch.empty(x.shape, device="cuda", dtype=torch.float32)
        L.check(L.load().icd_local_blend_groups(ptrs, heads, n, G, P, c["res"], c["alpha"].shape[1], maps[0].stride(1), al.data_ptr(), als.data_ptr(),
                                                tp, ts, fl, x.data_ptr(), int(x.dtype == torch.float32), x.shape[1], x.shape[2], x.shape[3],
                                                out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "icd_local_blend_groups")
    sync(f"local blend ({route})")
    return out.cpu()


def check_blend(c, name):
    got = blend_run(c, "ws")
    direct = blend_run(c, "direct")
    assert got.dtype == torch.float32 and got.shape == c["want"].shape
    bad = int((got != c["want"]).sum())
    assert torch.equal(got, c["want"]), f"{name}: {bad} of {got.numel()} elements differ from the fp64-mask blend"
    assert torch.equal(direct, got), f"{name}: the workspace-less entry and the reduce launch disagree"
    P = c["P"]
    for g in range(c["G"]):
        assert torch.equal(got[g * P], c["x"][g * P].float()), f"{name}: the base prompt of group {g} was blended"
    return got


@pytest.mark.parametrize("name", list(cpu.BLEND_CASES))
def test_local_blend_equals_the_fp64_mask_blend(name):
    c = cpu.blend_case(name)
    assert all(g >= cpu.BLEND_GAP for g in c["gaps"]) and 0.02 < c["on"][0] < 0.98
    check_blend(c, name)


def test_local_blend_groups_past_the_argument_block_each_equal_their_own_call():
    c = cpu.blend_many_groups()
    assert all(g >= cpu.BLEND_GAP for g in c["gaps"]) and 0.02 < sum(c["on"]) / len(c["on"]) < 0.98
    got = check_blend(c, f"{c['G']} groups")
    maps, x = blend_device(c)
    P, G = c["P"], c["G"]
    for g in range(G):
        one = cpu.group_slice(c, g)
        dev = ([m[g * (m.shape[0] // G):(g + 1) * (m.shape[0] // G)] for m in maps], x[g * P:(g + 1) * P].contiguous())
        for route in ("ws", "direct"):
            assert torch.equal(blend_run(one, route, dev), got[g * P:(g + 1) * P]), (g, route)


def test_local_blend_with_word_weights_that_are_all_zero():
    """0 / 0 compares false: a set substruct flag over all-zero substruct weights clears nothing, all-zero main weights blend nothing."""
    c = cpu.blend_zero_words()
    got = check_blend(c, "zero words")
    assert torch.equal(got[3], c["x"][2].float()) and not torch.equal(got[1], c["x"][0].float())


# ========================================================================================================== D. accumulate
def test_accumulate_table_entry_past_one_grid_sweep_with_empty_tensors_and_ragged_counts():
    ops = _ops()
    gen = torch.Generator().manual_seed(11)
    counts = [cpu.ACCUM_BIG] + cpu.ACCUM_COUNTS + [16] * 24
    assert len(counts) > 32 and 0 in counts and max(counts) > 512 * 256 * 8
    dst = [torch.rand(n, generator=gen).half().cuda() for n in counts]
    src = [torch.rand(n, generator=gen).half().cuda() for n in counts]
    want = [d.clone() for d in dst]
    for w, s in zip(want, src):
        w += s
    ops.accumulate_multi(dst, src)
    sync("accumulate (table)")
    for n, d, w in zip(counts, dst, want):
        assert torch.equal(d, w), n
    # the table entry itself with the empty tensor's null pointers and count 0 in the table
    L = _lib()
    again = [d.clone() for d in dst]
    table = torch.tensor([[a.data_ptr() for a in again], [b.data_ptr() for b in src], counts], dtype=torch.int64).cuda()
    assert again[counts.index(0)].data_ptr() == 0
    L.check(L.load().icd_accumulate_multi_n(table.data_ptr(), len(counts), max(counts), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "table")
    sync("accumulate (table, direct)")
    for w, s in zip(want, src):
        w += s
    for n, d, w in zip(counts, again, want):
        assert torch.equal(d, w), n


def test_accumulate_argument_entry_with_an_empty_tensor_and_ragged_counts():
    ops = _ops()
    gen = torch.Generator().manual_seed(12)
    counts = cpu.ACCUM_COUNTS
    dst = [torch.rand(n, generator=gen).half().cuda() for n in counts]
    src = [torch.rand(n, generator=gen).half().cuda() for n in counts]
    want = [d.clone() for d in dst]
    for w, s in zip(want, src):
        w += s
    ops.accumulate_multi(dst, src)
    sync("accumulate (arguments)")
    for n, d, w in zip(counts, dst, want):
        assert torch.equal(d, w), n
    empty = torch.zeros(0, dtype=torch.float16, device="cuda")
    ops.accumulate_multi([empty], [empty])              # nothing but an empty tensor: no launch
