"""CPU companion of test_p2p_edges_gpu.py: the case tables of the prompt-to-prompt kernels' edge tests (csrc/p2p.hip: the cross-attention
edit, LocalBlend, accumulate; the edit epilogue of attn_probs_kernel in csrc/attention.hip), their fp64 references, the conditions the
inputs must meet, and the argument refusals that return before any launch.

A. The cross edit.  want[e] = base @ A16 + D * cur[e] in fp64, A16 the fp16-rounded operator the kernel reads (ops.p2p_pack_operator);
   per element |got - want| <= bound_f16(want, S, 81) of test_gemm_edges.py with S = |base| @ |A16| + |D| |cur|: one fp16 rounding of the
   output plus the forward error of an fp32 sum of 80 products and one fused multiply-add in any order.  Identity (A = 0, D = 1) and
   permutation (A a permutation matrix, D = 0) operators are exact: one product per output summed with zeros, so the output is the input
   bit for bit / the base row's columns permuted bit for bit - which pins the MFMA fragment and accumulator layout at every row stride.
B. The fused epilogue.  The table of shapes; the `ld < 80` question is settled by reading the epilogue and restated here as a host
   function (fused_edit_columns): every column of a row is covered at any ld <= 96 that is a multiple of 8.
C. LocalBlend.  The reference is LocalBlend.get_mask in fp64 on the fp16 maps.  The thresholds are inputs and the tests choose them: per
   group and per kind (pooled main words, unpooled substruct words) the midpoint of the widest gap between consecutive distinct normalised
   ratios in (0.15, 0.6).  A gap of 1e-3 is asserted here as a condition on the inputs: an fp32 sum of at most 3 words x 130 heads of
   positive terms errs by under 3e-5 relative in any order, one division and the threshold's own fp32 rounding add 2e-7, so no pixel can
   cross a threshold 5e-4 away and the GPU tests compare all elements with torch.equal.
D. accumulate: the refusal of a misaligned pointer.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from p2p_sdxl_inputs import blend_inputs, blend_masks, blend_with
from test_gemm_edges import bound_f16, worst

from invertible_cd_amd import _lib, ops

SENTINEL = -7.0
GUARD_ROWS = 3
FAKE = 0x1000                                        # a 16-byte aligned non-null address that a refused call never dereferences
K_BOUND = 81                                         # 80 products and the D * cur term


# ======================================================================================================= A. the cross edit
# (heads, nq, ld, nk, n_prompts, groups, operator kinds - handed out in turn to the (group, edit) pairs, every pair with its own draw)
CROSS_CASES = [
    (1, 1, 80, 77, 2, 1, ("random",)),               # one row: 31 lanes of the only live wave have none, three waves have no query
    (1, 31, 88, 13, 3, 1, ("random",)),              # one short of a wave; ld = 88: the last 4-column group of n-tile 2 is skipped
    (2, 16, 96, 76, 2, 3, ("random",)),              # exactly one wave
    (3, 11, 104, 80, 5, 1, ("random",)),             # one row into the second wave; ld = 104: columns 96 .. 103 are nobody's
    (1, 127, 80, 1, 2, 1, ("random",)),              # one short of a block; one token
    (4, 32, 88, 77, 3, 3, ("random",)),              # exactly one block
    (3, 43, 96, 80, 2, 1, ("random",)),              # a second block of one row
    (3, 100, 104, 77, 3, 3, ("random",)),            # three blocks, the last with a partial wave and a query-less one
    (3, 43, 80, 77, 3, 1, ("identity",)),
    (3, 11, 104, 13, 2, 3, ("identity",)),
    (3, 100, 80, 77, 2, 1, ("perm",)),
    (3, 43, 88, 80, 3, 1, ("perm",)),
    (3, 11, 96, 76, 2, 3, ("perm",)),
    (1, 127, 104, 80, 5, 1, ("perm",)),
    (4, 32, 80, 77, 3, 1, ("refine",)),
    (3, 43, 96, 77, 2, 3, ("reweight",)),
    (3, 11, 88, 77, 5, 3, ("random", "perm", "reweight", "identity", "refine")),      # more than two edits, every one another kind
]
CROSS_ROWS, CROSS_LD, CROSS_NK, CROSS_P, CROSS_G = {1, 31, 32, 33, 127, 128, 129, 300}, {80, 88, 96, 104}, {1, 13, 76, 77, 80}, {2, 3, 5}, {1, 3}
CROSS_KINDS = {"random", "identity", "perm", "refine", "reweight"}
# (nk, ld, n_prompts, groups, fragment of the message)
CROSS_REFUSALS = [(81, 88, 2, 1, "tokens <= 80"), (77, 72, 2, 1, "row stride >= 80"), (77, 84, 2, 1, "multiple of 8"),
                  (77, 80, 1, 1, "need a base prompt"), (77, 80, 2, 0, "1 .. 65535 groups"), (77, 80, 2, 65536, "1 .. 65535 groups")]


def make_operator(kind, nk, gen):
    """(A fp32 [nk, nk] (row w, column n), D fp32 [nk], the permutation or None): new[n] = sum_w base[w] A[w][n] + D[n] cur[n]."""
    A, D, perm = torch.zeros(nk, nk), torch.zeros(nk), None
    if kind == "random":                             # sparse, as the replace mappers are
        A = torch.rand(nk, nk, generator=gen) * (torch.rand(nk, nk, generator=gen) < max(0.05, 1.5 / nk))
        D = torch.rand(nk, generator=gen)
    elif kind == "identity":                         # a_t = 0: outside the controller's step window for every token
        D = torch.ones(nk)
    elif kind == "perm":
        perm = torch.randperm(nk, generator=gen)
        A[perm, torch.arange(nk)] = 1.0
    elif kind == "refine":                           # a_t * (base[mapper] * alphas + cur * (1 - alphas)) + (1 - a_t) * cur
        src, al = torch.randint(0, nk, (nk,), generator=gen), (torch.rand(nk, generator=gen) < 0.7).float()
        a_t = 0.05 + 0.9 * torch.rand(nk, generator=gen)
        A[src, torch.arange(nk)] = a_t * al
        D = a_t * (1 - al) + (1 - a_t)
    elif kind == "reweight":                         # an equalizer on an identity mapper, a_t = 1: outputs leave [0, 1] on both sides
        eq = torch.ones(nk)
        pick = torch.randperm(nk, generator=gen)
        eq[pick[:max(1, nk // 8)]] = 5.0
        eq[pick[max(1, nk // 8):max(2, nk // 4)]] = -2.0
        A[torch.arange(nk), torch.arange(nk)] = eq
    else:
        raise ValueError(kind)
    return A, D, perm


@functools.lru_cache(maxsize=None)
def cross_case(i):
    """Inputs, fp64 reference and bound of CROSS_CASES[i], computed once and shared (nothing here is written to afterwards)."""
    heads, nq, ld, nk, P, G, kinds = CROSS_CASES[i]
    gen = torch.Generator().manual_seed(900 + i)
    R, rows, E = G * P * heads, heads * nq, G * (P - 1)
    probs = torch.zeros(R, nq, ld, dtype=torch.float16)
    probs[:, :, :nk] = torch.softmax(torch.randn(R, nq, nk, generator=gen) * 3.0, dim=-1).half()
    probs[:, :, 96:] = SENTINEL                      # ld = 104: the columns no token slot reaches
    kind_of = [kinds[j % len(kinds)] for j in range(E)]
    made = [make_operator(k, nk, gen) for k in kind_of]
    At, Dp = ops.p2p_pack_operator(torch.stack([m[0] for m in made]), torch.stack([m[1] for m in made]))
    A16 = At[:, :nk, :nk].transpose(1, 2).double().reshape(G, P - 1, nk, nk)
    D64 = Dp[:, :nk].double().reshape(G, P - 1, 1, nk)
    x = probs[:, :, :nk].double().reshape(G, P, rows, nk)
    base, cur = x[:, :1], x[:, 1:]
    want = base @ A16 + D64 * cur                    # [G, P - 1, rows, nk]
    S = base.abs() @ A16.abs() + D64.abs() * cur.abs()
    return dict(heads=heads, nq=nq, ld=ld, nk=nk, P=P, G=G, rows=rows, probs=probs, At=At, Dp=Dp, kinds=kind_of, perms=[m[2] for m in made],
                want=want, S=S, bound=bound_f16(want, S, K_BOUND))


def cross_edit_rows(c, t):
    """t [G * P * heads, nq, >= nk] -> the edited prompts' rows [G, P - 1, rows, nk] (and the base prompts' [G, 1, rows, nk])."""
    x = t[:, :, :c["nk"]].reshape(c["G"], c["P"], c["rows"], c["nk"])
    return x[:, 1:], x[:, :1]


def check_exact_kinds(c, got_edit, name):
    """The operators whose result is exact: got_edit [G, P - 1, rows, nk] fp16 against the input bits."""
    cur, base = cross_edit_rows(c, c["probs"])
    for j, kind in enumerate(c["kinds"]):
        g, e = divmod(j, c["P"] - 1)
        if kind == "identity":
            assert torch.equal(got_edit[g, e], cur[g, e]), f"{name}: identity operator of (group {g}, edit {e}) changed the row"
        if kind == "perm":
            assert torch.equal(got_edit[g, e], base[g, 0][:, c["perms"][j]]), f"{name}: permutation of (group {g}, edit {e}) is not exact"


def cross_edit_c(probs, groups, n_prompts, heads, nq, nk, ld, At=FAKE, D=FAKE):
    return _lib.load().icd_p2p_cross_edit_groups(C.c_void_p(probs), groups, n_prompts, heads, nq, nk, ld, C.c_void_p(At), C.c_void_p(D), None)


def test_the_cross_edit_table_holds_every_value_the_kernel_branches_on():
    assert len(CROSS_CASES) <= 18
    col = lambda f: {f(c) for c in CROSS_CASES}
    assert col(lambda c: c[0] * c[1]) == CROSS_ROWS and col(lambda c: c[2]) == CROSS_LD and col(lambda c: c[3]) == CROSS_NK
    assert col(lambda c: c[4]) == CROSS_P and col(lambda c: c[5]) == CROSS_G and {k for c in CROSS_CASES for k in c[6]} == CROSS_KINDS
    assert {c[2] for c in CROSS_CASES if "perm" in c[6]} == CROSS_LD                  # the layout is pinned at every row stride
    for i in range(len(CROSS_CASES)):                # every (group, edit) has an operator of its own
        c = cross_case(i)
        flat = c["At"].reshape(c["At"].shape[0], -1)
        if "identity" not in c["kinds"]:
            assert len({tuple(r.tolist()) for r in flat}) == flat.shape[0], i


@pytest.mark.parametrize("i", range(len(CROSS_CASES)))
def test_torch_fp32_stays_inside_the_cross_edit_bound(i):
    """The bound is a property of fp32 arithmetic: torch's fp32 product plus D * cur, rounded once, stays inside it, is exact for the
    identity and permutation operators, and the packed operator is zero outside its nk x nk corner."""
    c = cross_case(i)
    nk, G, P = c["nk"], c["G"], c["P"]
    cur, base = cross_edit_rows(c, c["probs"])
    A = c["At"][:, :nk, :nk].transpose(1, 2).float().reshape(G, P - 1, nk, nk)
    got = (base.float() @ A + c["Dp"][:, :nk].reshape(G, P - 1, 1, nk) * cur.float()).half()
    r, _ = worst(got, c["want"], c["bound"])
    print(f"[p2p-edges cpu A {i}] torch fp32 worst error / bound {r:.3f}")
    assert r <= 1.0
    check_exact_kinds(c, got, f"case {i}")
    assert not c["At"][:, nk:].any() and not c["At"][:, :, nk:].any() and not c["Dp"][:, nk:].any()
    if "reweight" in c["kinds"]:
        assert float(c["want"].min()) < -0.1 and float(c["want"].max()) > 1.1


def test_a_swapped_accumulator_group_fails_the_permutation_check_and_the_bound():
    """What the exact operators buy: the two 4-column halves of every 8-column accumulator group swapped (the half-wave index of the
    32 x 32 MFMA layout read the wrong way round) is caught by the permutation cases and, on a random operator, by the bound."""
    for i, c in ((j, cross_case(j)) for j in range(len(CROSS_CASES))):
        if c["nk"] != 80 or c["kinds"][0] not in ("perm", "random"):
            continue
        nk, G, P = c["nk"], c["G"], c["P"]
        cur, base = cross_edit_rows(c, c["probs"])
        A = c["At"][:, :nk, :nk].transpose(1, 2).float().reshape(G, P - 1, nk, nk)
        good = (base.float() @ A + c["Dp"][:, :nk].reshape(G, P - 1, 1, nk) * cur.float()).half()
        bad = good.reshape(G, P - 1, c["rows"], nk // 8, 2, 4).flip(-2).reshape(good.shape)
        if c["kinds"][0] == "perm":
            with pytest.raises(AssertionError, match="is not exact"):
                check_exact_kinds(c, bad, f"case {i}")
        assert worst(bad, c["want"], c["bound"])[0] > 1.0


@pytest.mark.parametrize("nk,ld,n_prompts,groups,fragment", CROSS_REFUSALS)
def test_cross_edit_refuses_before_any_launch(nk, ld, n_prompts, groups, fragment):
    lib = _lib.load()
    assert cross_edit_c(FAKE, groups, n_prompts, 2, 16, nk, ld) == -1
    assert fragment.encode() in lib.icd_last_error(), lib.icd_last_error()


def test_cross_edit_refuses_null_pointers_and_the_front_end_states_the_geometry():
    assert cross_edit_c(0, 1, 2, 2, 16, 77, 80) == -1 and cross_edit_c(FAKE, 1, 2, 2, 16, 77, 80, At=0) == -1
    assert cross_edit_c(FAKE, 1, 2, 0, 16, 77, 80) == -1 and cross_edit_c(FAKE, 1, 2, 2, 0, 77, 80) == -1
    for nk, ld, ok in ((77, 80, True), (80, 80, True), (1, 104, True), (13, 88, True), (81, 88, False), (77, 77, False), (77, 72, False),
                       (77, 84, False), (13, 16, False)):
        assert ops.p2p_cross_edit_geometry(nk, ld) == ok, (nk, ld)
    assert not ops.p2p_cross_edit_supported(torch.zeros(4, 8, 80, dtype=torch.float16)[:, :, :77])      # not on the device


# ================================================================================================== B. the fused edit epilogue
# (Nq, Nk, ld, d, groups, n_prompts, unrelated samples in front, with acc)
FUSED_CASES = [(33, 13, 80, 40, 1, 2, 0, False), (200, 77, 80, 64, 3, 2, 1, True), (33, 77, 88, 64, 1, 3, 1, True),
               (200, 80, 88, 40, 3, 2, 0, False), (33, 80, 96, 40, 3, 3, 0, True), (200, 13, 96, 64, 1, 2, 2, False),
               (200, 77, 96, 40, 1, 5, 0, True), (33, 80, 80, 64, 3, 2, 1, False)]
# row strides below the 80 columns the stand-alone entry asks for: one, two and three key tiles, each with a ragged last 8-column group
FUSED_NARROW = [(33, 13, 16, 40, 1, 2, 1, True), (200, 13, 16, 64, 3, 2, 0, False), (33, 8, 8, 40, 1, 2, 0, True),
                (33, 33, 40, 40, 1, 3, 0, True), (200, 70, 72, 64, 3, 2, 1, True)]
FUSED_H = 2


def fused_edit_columns(ldp):
    """The columns of a probability row that attn_probs_kernel's edit epilogue recombines and its flush then stores, restated from the
    kernel: nt = ceil(ldp / 32) key tiles; in tile kt the lane pair (g, lh) owns tokens 32 kt + 8 g + 4 lh .. + 3 and skips them when they
    end past ldp; the flush stores the 8-column segments that begin below ldp."""
    nt = (ldp + 31) >> 5
    edited = {32 * kt + 8 * g + 4 * lh + i for kt in range(min(nt, 3)) for g in range(4) for lh in range(2) for i in range(4)
              if 32 * kt + 8 * g + 4 * lh + 4 <= ldp}
    stored = {32 * kt + c8 + i for kt in range(min(nt, 3)) for c8 in range(0, 32, 8) for i in range(8) if 32 * kt + c8 < ldp}
    return edited, stored


def test_the_fused_edit_epilogue_handles_every_row_stride_up_to_96():
    """The `ld < 80` question, decided from the code: the geometry IS handled.  The epilogue takes the base prompt's probabilities from
    its own accumulators (five 16-key fragments, zero beyond the live key tiles and beyond Nk), not from 80 columns of memory as the
    stand-alone kernel does, and both its token-slot skip and its flush are written against ldp: at every ldp <= 96 that is a multiple of 8
    each column of the row is recombined once and stored once, none past the row.  So probs_validate keeps accepting it; the entry's plan
    takes the FEW instantiation with the edit, and test_p2p_edges_gpu.py holds the values against the fp64 reference of section A."""
    for ldp in range(8, 97, 8):
        edited, stored = fused_edit_columns(ldp)
        assert edited == stored == set(range(ldp)), ldp
    lib = _lib.load()
    for Nq, Nk, ld, d, G, P, b0, _ in FUSED_CASES + FUSED_NARROW:
        q = _lib.AttentionQuery(entry=1, B=b0 + G * P, H=FUSED_H, Nq=Nq, Nk=Nk, d=d, ldp=ld, flags=0, split=0, epi=2)
        info = _lib.AttentionInfo()
        assert lib.icd_attention_plan(C.byref(q), C.byref(info)) == 0, (Nk, ld, lib.icd_last_error())
        assert (info.EPI, info.FEW, info.KS) == (2, 1, 3 if d <= 48 else 5)
    bad = _lib.AttentionQuery(entry=1, B=2, H=FUSED_H, Nq=33, Nk=13, d=40, ldp=104, flags=0, split=0, epi=2)
    assert lib.icd_attention_plan(C.byref(bad), C.byref(_lib.AttentionInfo())) == -1       # past 96 columns the edit is refused


def test_the_fused_table_holds_every_value_asked_for():
    col = lambda j: {c[j] for c in FUSED_CASES}
    assert col(0) == {33, 200} and col(1) == {13, 77, 80} and col(2) == {80, 88, 96} and col(3) == {40, 64} and col(4) == {1, 3}
    assert col(7) == {False, True} and all(c[2] < 80 for c in FUSED_NARROW) and (33, 13, 16, 40, 1, 2, 1, True) in FUSED_NARROW


def fused_operators(G, P, Nk, seed):
    """Packed operators of a fused case: random, reweight and refine operators in turn, one per (group, edit)."""
    gen = torch.Generator().manual_seed(seed)
    made = [make_operator(("random", "reweight", "refine")[j % 3], Nk, gen) for j in range(G * (P - 1))]
    return ops.p2p_pack_operator(torch.stack([m[0] for m in made]), torch.stack([m[1] for m in made]))


def edit_ref64(plain, At, Dp, G, P, Nk):
    """(want, bound) [G, P - 1, rows, Nk] of the edit applied to the fp16 probabilities `plain` [G * P * H, Nq, ld] (CPU tensors)."""
    rows = plain.shape[0] // (G * P) * plain.shape[1]
    x = plain[:, :, :Nk].double().reshape(G, P, rows, Nk)
    A16 = At[:, :Nk, :Nk].transpose(1, 2).double().reshape(G, P - 1, Nk, Nk)
    D64 = Dp[:, :Nk].double().reshape(G, P - 1, 1, Nk)
    want = x[:, :1] @ A16 + D64 * x[:, 1:]
    return want, bound_f16(want, x[:, :1].abs() @ A16.abs() + D64.abs() * x[:, 1:].abs(), K_BOUND)


# ========================================================================================================== C. LocalBlend
BLEND_GAP = 1e-3
BLEND_WINDOW = (0.15, 0.6)
# name -> layer_heads, res, (H, W), C, x dtype, n_words, ld, P, substruct words, a word at alpha 0.5
BLEND_CASES = {
    "1 head": ((1,), 5, (20, 20), 4, torch.float16, 77, 77, 2, True, False),
    "15 heads": ((10, 5), 16, (64, 64), 4, torch.float16, 77, 77, 2, True, False),
    "16 heads": ((4, 8, 4), 16, (64, 64), 4, torch.float32, 77, 77, 3, True, False),
    "17 heads": ((10, 4, 3), 5, (20, 20), 1, torch.float16, 13, 80, 2, True, True),
    "63 heads": ((10, 20, 10, 20, 3), 5, (20, 20), 4, torch.float16, 77, 77, 2, False, False),
    "64 heads": ((20, 20, 20, 4), 16, (16, 16), 1, torch.float32, 13, 80, 2, True, False),
    "65 heads": ((20, 20, 20, 4, 1), 5, (20, 20), 4, torch.float16, 77, 77, 2, True, True),
    "129 heads": ((30, 30, 30, 30, 9), 5, (20, 20), 4, torch.float16, 77, 77, 2, True, False),
    "64 layers": ((1,) * 64, 5, (20, 20), 1, torch.float16, 77, 77, 2, True, False),
    "res 16 -> 24 x 40": ((3, 2), 16, (24, 40), 4, torch.float16, 77, 77, 2, True, False),
    "res 16 -> 8 x 8": ((3, 2), 16, (8, 8), 4, torch.float32, 77, 77, 2, True, False),
    "res 16 -> 17 x 23": ((2, 3), 16, (17, 23), 1, torch.float16, 77, 77, 3, True, True),
    "res 17 -> 68 x 68": ((2, 3), 17, (68, 68), 4, torch.float16, 13, 80, 2, True, False),
    "res 32 -> 128 x 128": ((2, 3), 32, (128, 128), 1, torch.float16, 77, 77, 2, True, False),
}
BLEND_TOTAL_HEADS, BLEND_RES = {1, 15, 16, 17, 63, 64, 65, 129}, {5, 16, 17, 32}
BLEND_SEEDS = {"res 16 -> 8 x 8": 1307}              # a draw on which the order of resize and normalisation shows (asserted below)
BLEND_MANY = 33                                      # groups of the second BLEND_MAX_GROUPS chunk


def blend_ratios(maps, alpha, pool, size):
    """LocalBlend.get_mask up to its threshold, in fp64 on the fp16 maps of one prompt group: [P, 1, H, W] normalised heat (NaN where the
    words' weights are all zero: 0 / 0).  maps: [P * heads_l, res * res, n_words] per layer, any row stride."""
    P, nw = alpha.shape
    res = math.isqrt(maps[0].shape[1])
    cols = torch.nonzero(alpha.sum(0)).flatten()     # the words alpha leaves out contribute exact zeros: only its columns are read
    if cols.numel() == 0:
        cols = torch.arange(1)
    al = alpha.double()[:, cols].reshape(P, 1, 1, 1, 1, -1)
    heat = torch.cat([(m[:, :, cols].double().reshape(P, -1, 1, res, res, cols.numel()) * al).sum(-1) for m in maps], dim=1).mean(1)
    if pool:
        heat = F.max_pool2d(heat, kernel_size=3, stride=1, padding=1)
    heat = F.interpolate(heat, size=size)
    return heat / heat.amax(dim=(2, 3), keepdim=True)


def gap_threshold(ratios):
    """(threshold, gap): the midpoint of the widest gap between consecutive distinct ratios inside BLEND_WINDOW; (0.3, None) without two."""
    v = torch.unique(ratios[(ratios > BLEND_WINDOW[0]) & (ratios < BLEND_WINDOW[1])])
    if v.numel() < 2:
        return 0.3, None
    gaps = v[1:] - v[:-1]
    i = int(gaps.argmax())
    return float((v[i] + v[i + 1]) / 2), float(gaps[i])


def mask64(maps, alpha, sub, th_pool, th_sub, size):
    on = blend_ratios(maps, alpha, True, size).gt(th_pool)
    mask = on[:1] + on
    if sub is not None:
        s = blend_ratios(maps, sub, False, size).gt(th_sub)
        mask = mask * ~(s[:1] + s)
    return mask


def blend_reference(maps, alpha, sub, has_sub, active, x, G):
    """Per group: thresholds in the widest gaps of the group's own fp64 ratios, and the blend they give.  -> dict(th_pool, th_sub: G floats,
    gaps: every gap that was used, want fp32 [G * P, C, H, W], on: mean of the edited prompts' masks over the active groups)."""
    GP = alpha.shape[0]
    P, size = GP // G, tuple(x.shape[2:])
    out = dict(th_pool=[], th_sub=[], gaps=[], want=[], on=[])
    for g in range(G):
        rows = slice(g * P, (g + 1) * P)
        mg = [m[g * (m.shape[0] // G):(g + 1) * (m.shape[0] // G)] for m in maps]
        tp, gp = gap_threshold(blend_ratios(mg, alpha[rows], True, size))
        ts, gs = gap_threshold(blend_ratios(mg, sub[rows], False, size)) if has_sub[g] else (0.3, None)
        out["th_pool"].append(tp)
        out["th_sub"].append(ts)
        if not active[g]:
            out["want"].append(x[rows].float())
            continue
        out["gaps"] += [gp] + ([gs] if has_sub[g] else [])
        mask = mask64(mg, alpha[rows], sub[rows] if has_sub[g] else None, tp, ts, size)
        out["want"].append(blend_with(mask, x[rows]).float())
        out["on"].append(float(mask[1:].float().mean()))
    out["want"] = torch.cat(out["want"])
    return out


def strided_maps(maps, ld):
    """The maps as views [rows, res * res, n_words] of NaN-filled buffers with row stride ld (a read past n_words shows in the heat)."""
    if ld == maps[0].shape[2]:
        return maps
    out = []
    for m in maps:
        buf = torch.full((m.shape[0], m.shape[1], ld), float("nan"), dtype=torch.float16)
        buf[:, :, :m.shape[2]] = m
        out.append(buf[:, :, :m.shape[2]])
    return out


@functools.lru_cache(maxsize=None)
def blend_case(name):
    layer_heads, res, hw, Cc, dtype, n_words, ld, P, with_sub, half_word = BLEND_CASES[name]
    seed = BLEND_SEEDS.get(name, 1000 + list(BLEND_CASES).index(name))
    maps, alpha, sub, x = blend_inputs(seed, P, 0, 0, res, hw, dtype, layer_heads=list(layer_heads), channels=Cc, n_words=n_words)
    if half_word:
        alpha[:, 5] = 0.5
    c = dict(maps=strided_maps(maps, ld), alpha=alpha, sub=sub, has_sub=[with_sub], active=[True], x=x, G=1, P=P, res=res, ld=ld)
    c.update(blend_reference(c["maps"], alpha, sub, c["has_sub"], c["active"], x, 1))
    return c


@functools.lru_cache(maxsize=None)
def blend_many_groups():
    """BLEND_MANY groups of two prompts at res 5, one layer of one head, C = 1, 5 x 5 latents: every third group without substruct words,
    groups 4, 20 and 32 (one of them in the second chunk) inactive."""
    G, P = BLEND_MANY, 2
    maps, alpha, sub, x = blend_inputs(1100, G * P, 0, 0, 5, (5, 5), torch.float16, layer_heads=[1], channels=1)
    has_sub, active = [g % 3 != 1 for g in range(G)], [g not in (4, 20, 32) for g in range(G)]
    c = dict(maps=maps, alpha=alpha, sub=sub, has_sub=has_sub, active=active, x=x, G=G, P=P, res=5, ld=77)
    c.update(blend_reference(maps, alpha, sub, has_sub, active, x, G))
    return c


@functools.lru_cache(maxsize=None)
def blend_zero_words():
    """Three groups of two prompts: group 0 has the substruct flag set and substruct weights that are all zero, group 1 has main weights
    that are all zero, group 2 is ordinary.  0 / 0 compares false against any threshold: group 0 is blended by its main words alone and
    group 1 comes back as its base prompt."""
    G, P = 3, 2
    maps, alpha, sub, x = blend_inputs(1200, G * P, 0, 0, 16, (64, 64), torch.float16, layer_heads=[3, 2])
    sub[0:2] = 0
    alpha[2:4] = 0
    c = dict(maps=maps, alpha=alpha, sub=sub, has_sub=[True] * G, active=[True] * G, x=x, G=G, P=P, res=16, ld=77)
    c.update(blend_reference(maps, alpha, sub, c["has_sub"], c["active"], x, G))
    return c


def group_slice(c, g):
    """Group g of a many-group case as a one-group case of its own (the same thresholds and reference rows)."""
    P, G = c["P"], c["G"]
    rows = slice(g * P, (g + 1) * P)
    return dict(maps=[m[g * (m.shape[0] // G):(g + 1) * (m.shape[0] // G)] for m in c["maps"]], alpha=c["alpha"][rows], sub=c["sub"][rows],
                has_sub=[c["has_sub"][g]], active=[c["active"][g]], x=c["x"][rows], G=1, P=P, res=c["res"], ld=c["ld"],
                th_pool=[c["th_pool"][g]], th_sub=[c["th_sub"][g]], want=c["want"][rows])


def test_the_blend_table_holds_every_value_asked_for():
    t = list(BLEND_CASES.values())
    assert {sum(c[0]) for c in t} >= BLEND_TOTAL_HEADS and {c[1] for c in t} == BLEND_RES
    assert any(len(set(c[0])) > 1 for c in t) and any(len(c[0]) == 64 for c in t)
    assert {c[2] for c in t if c[1] == 16} >= {(16, 16), (24, 40), (8, 8), (17, 23), (64, 64)} and (17, (68, 68)) in {(c[1], c[2]) for c in t}
    assert {c[3] for c in t} == {1, 4} and {c[4] for c in t} == {torch.float16, torch.float32}
    assert {(c[5], c[6]) for c in t} == {(13, 80), (77, 77)} and any(c[9] for c in t) and {c[8] for c in t} == {False, True}
    assert {c[1] ** 2 % 16 == 0 for c in t} == {False, True} and max(c[1] ** 2 for c in t) == 1024


@pytest.mark.parametrize("name", list(BLEND_CASES))
def test_blend_thresholds_sit_in_gaps_and_the_masks_have_both_sides(name):
    """Conditions on the inputs, on the fp64 reference alone: every threshold a case uses sits in a gap of at least BLEND_GAP, and the
    edited prompts' masks are neither empty nor full."""
    c = blend_case(name)
    print(f"[p2p-edges cpu C] {name}: thresholds {c['th_pool'][0]:.4f} / {c['th_sub'][0]:.4f}, gaps {c['gaps']}, mask on {c['on'][0]:.3f}")
    assert all(g is not None and g >= BLEND_GAP for g in c["gaps"]) and len(c["gaps"]) == 1 + int(c["has_sub"][0])
    assert 0.02 < c["on"][0] < 0.98
    assert torch.equal(c["want"][0], c["x"][0].float())
    assert BLEND_WINDOW[0] < c["th_pool"][0] < BLEND_WINDOW[1] and BLEND_WINDOW[0] < c["th_sub"][0] < BLEND_WINDOW[1]


def test_many_groups_and_zero_words_meet_the_same_conditions():
    c = blend_many_groups()
    assert c["G"] > 32 and all(g is not None and g >= BLEND_GAP for g in c["gaps"])
    assert len(c["gaps"]) == sum(1 + int(s) for s, a in zip(c["has_sub"], c["active"]) if a)
    assert 0.02 < sum(c["on"]) / len(c["on"]) < 0.98 and len(set(c["th_pool"])) == c["G"]
    for g in range(c["G"]):
        rows = slice(2 * g, 2 * g + 2)
        assert torch.equal(c["want"][2 * g], c["x"][2 * g].float())
        assert c["active"][g] or torch.equal(c["want"][rows], c["x"][rows].float())
    print(f"[p2p-edges cpu C] {c['G']} groups: smallest gap {min(c['gaps']):.2e}")
    z = blend_zero_words()
    assert z["gaps"][1] is None and z["gaps"][2] is None and all(g >= BLEND_GAP for g in z["gaps"] if g is not None)
    x = z["x"].float()
    assert torch.equal(z["want"][2], x[2]) and torch.equal(z["want"][3], x[2])                  # no main words: the base prompt
    only_main = blend_with(mask64([m[:m.shape[0] // 3] for m in z["maps"]], z["alpha"][:2], None, z["th_pool"][0], 0.3, (64, 64)), z["x"][:2])
    assert torch.equal(z["want"][:2], only_main.float()) and not torch.equal(z["want"][1], x[0]) and not torch.equal(z["want"][1], x[1])


def test_the_fp64_reference_is_the_shared_torch_expression():
    """mask64 against blend_masks of p2p_sdxl_inputs.py (the expression the older LocalBlend tests use) evaluated in double."""
    c = blend_case("15 heads")
    for th in (c["th_pool"][0], c["th_sub"][0]):
        main, full = blend_masks(c["maps"], c["alpha"], c["sub"], th, (64, 64), torch.float64)
        assert torch.equal(main, mask64(c["maps"], c["alpha"], None, th, th, (64, 64)))
        assert torch.equal(full, mask64(c["maps"], c["alpha"], c["sub"], th, th, (64, 64)))


def test_the_8x8_latent_tells_the_reference_from_a_maximum_over_the_whole_map():
    """The reference normalises after its nearest resize.  Under an 8 x 8 latent the resize reads every other pixel of a 16 x 16 map, so
    the unpooled substruct heat is divided by the largest SAMPLED pixel.  local_blend_kernel took the maximum over all 256 pixels until
    this case was written (threshold at the map's size, then resize the mask): the two differ here, and at no latent >= the map."""
    def at_map_size(c):
        r = c["res"]
        on = blend_ratios(c["maps"], c["alpha"], True, (r, r)).gt(c["th_pool"][0])
        s = blend_ratios(c["maps"], c["sub"], False, (r, r)).gt(c["th_sub"][0])
        mask = (on[:1] + on) * ~(s[:1] + s)
        return blend_with(F.interpolate(mask.double(), size=tuple(c["x"].shape[2:])).bool(), c["x"]).float()
    assert not torch.equal(at_map_size(blend_case("res 16 -> 8 x 8")), blend_case("res 16 -> 8 x 8")["want"])
    for name in ("res 16 -> 24 x 40", "res 16 -> 17 x 23", "64 heads", "15 heads"):
        assert torch.equal(at_map_size(blend_case(name)), blend_case(name)["want"]), name


def test_fp32_heat_cannot_cross_a_threshold_in_a_gap():
    """The argument for BLEND_GAP, tried on the largest sum of the table: the heat summed in fp32 in two different orders moves the
    normalised ratios by far less than half a gap."""
    c = blend_case("129 heads")
    cols = torch.nonzero(c["alpha"].sum(0)).flatten()
    al = c["alpha"][:, cols]
    P, res = c["P"], c["res"]
    terms = torch.cat([(m[:, :, cols].float().reshape(P, -1, res * res, cols.numel()) * al.reshape(P, 1, 1, -1)) for m in c["maps"]], dim=1)
    ref = terms.double().sum(-1).mean(1)
    ref = ref / ref.amax(1, keepdim=True)
    fwd = torch.zeros(P, res * res)
    for h in range(terms.shape[1]):
        for w in range(terms.shape[3]):
            fwd = fwd + terms[:, h, :, w]
    bwd = terms.flip(1).sum(-1).sum(1)
    for s in (fwd, bwd):
        s = s / terms.shape[1]
        assert float(((s / s.amax(1, keepdim=True)).double() - ref).abs().max()) < 0.1 * BLEND_GAP


def blend_c(n_layers=1, res=16, n_groups=1, n_prompts=2, n_words=77, ld=77, ws=None, ws_bytes=0, flags=1, heads=1):
    """icd_local_blend_groups_ws on addresses that a refused call never reads (the per-layer and per-group arrays are host arrays)."""
    lib = _lib.load()
    ptrs, hd = (C.c_void_p * max(n_layers, 1))(*[FAKE] * max(n_layers, 1)), (C.c_int32 * max(n_layers, 1))(*[heads] * max(n_layers, 1))
    th, fl = (C.c_float * max(n_groups, 1))(), (C.c_int32 * max(n_groups, 1))(*[flags] * max(n_groups, 1))
    return lib.icd_local_blend_groups_ws(ptrs, hd, n_layers, n_groups, n_prompts, res, n_words, ld, C.c_void_p(FAKE), C.c_void_p(FAKE), th, th, fl,
                                         C.c_void_p(FAKE), 0, 4, 64, 64, C.c_void_p(FAKE), C.c_void_p(ws) if ws else None, ws_bytes, None)


def test_local_blend_refuses_before_any_launch():
    lib = _lib.load()
    need = lib.icd_local_blend_workspace_bytes(3, 2, 16)
    assert need == 3 * 2 * 2 * 256 * 4
    for kw, fragment in ((dict(n_layers=65), "1..64 layers"), (dict(res=33), "res*res <= 1024"), (dict(n_layers=0), "1..64 layers"),
                         (dict(n_words=77, ld=76), "ld >= n_words"), (dict(heads=0), "has no maps"),
                         (dict(n_groups=3, ws=FAKE, ws_bytes=need - 1), "icd_local_blend_workspace_bytes asks for"),
                         (dict(n_groups=3, ws=FAKE + 2, ws_bytes=need + 2), "icd_local_blend_workspace_bytes asks for")):
        assert blend_c(**kw) == -1, kw
        assert fragment.encode() in lib.icd_last_error(), (kw, lib.icd_last_error())
    null_sub = lib.icd_local_blend_groups_ws((C.c_void_p * 1)(FAKE), (C.c_int32 * 1)(1), 1, 1, 2, 16, 77, 77, C.c_void_p(FAKE), None, (C.c_float * 1)(),
                                             (C.c_float * 1)(), (C.c_int32 * 1)(3), C.c_void_p(FAKE), 0, 4, 64, 64, C.c_void_p(FAKE), None, 0, None)
    assert null_sub == -1 and b"alpha_sub is NULL" in lib.icd_last_error()
    with pytest.raises(AssertionError, match="1..64 layers"):
        ops.local_blend_groups([None] * 65, torch.zeros(2, 77), None, [0.3], [0.3], [True], None, 1)


# ========================================================================================================== D. accumulate
ACCUM_BIG = 512 * 256 * 8 + 8 * 300 + 5              # past one sweep of the capped grid (512 blocks x 256 threads x 8), with a scalar tail
ACCUM_COUNTS = [23, 24, 25, 2047, 2048, 2049, 0, 1, 7, 8, 9]


def test_accumulate_refuses_a_pointer_off_the_16_byte_grid():
    lib = _lib.load()
    cn = (C.c_int64 * 2)(64, 64)
    for dst, src in (((FAKE, FAKE + 8), (FAKE, FAKE)), ((FAKE, FAKE), (FAKE + 2, FAKE))):
        assert lib.icd_accumulate_multi((C.c_void_p * 2)(*dst), (C.c_void_p * 2)(*src), cn, 2, None) == -1
        assert b"not 16-byte aligned" in lib.icd_last_error()
    assert lib.icd_accumulate_multi((C.c_void_p * 2)(FAKE, FAKE), (C.c_void_p * 2)(FAKE, FAKE), cn, 33, None) == -1
    assert lib.icd_accumulate_multi_n(C.c_void_p(FAKE + 4), 40, 64, None) == -1 and b"8-byte aligned" in lib.icd_last_error()
    assert lib.icd_accumulate_multi_n(C.c_void_p(FAKE), 65536, 64, None) == -1
