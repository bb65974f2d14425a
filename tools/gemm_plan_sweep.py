#!/usr/bin/env python3
"""Descriptors for the planner of icd_gemm (csrc/gemm.hip), and the recording of what it does with them.

    python tools/gemm_plan_sweep.py --write        # tests/golden/gemm_plans.json from the loaded library

cases() is a deterministic list of (name, descriptor) with dummy host pointers (icd_gemm_plan dereferences nothing): every GEMM and conv
shape of the SD1.5 and SDXL forwards, a cross of edge shapes, each with no / the requested / half the requested / an ample split-K
workspace, the epilogues, every tuning flag, conv mode, the fused cross-attention launch, operands around the 2^31-byte limits and the
refusal table of tests/test_gemm_edges.py.  It generates INPUTS only - nothing here restates the planner.  record() asks the library:
per descriptor the return code and the eight fields of icd_gemm_plan_info, per distinct (M, N, K) icd_gemm_workspace_bytes.
tests/test_gemm_plans.py replays cases() against the golden file, which was written once from the planner as it stood before gemm_run
was taken apart and is not to be regenerated: a plan that changes on purpose changes its rows by hand, with the reason in the commit.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from invertible_cd_amd import _lib                                                          # noqa: E402
from invertible_cd_amd.unet_config import SD15, SDXL                                        # noqa: E402
from test_gemm_edges import REFUSALS, conv_desc, dense_desc, dummy                          # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plans.json")
FIELDS = ("kernel", "tile_m", "tile_n", "ksplit", "ln_inline", "xattn", "cfg", "group_m")
GEGLU, F32, TRANS, RF32, LNC = _lib.ICD_GEMM_GEGLU, _lib.ICD_GEMM_OUT_F32, _lib.ICD_GEMM_OUT_TRANS, _lib.ICD_GEMM_RESID_F32, _lib.ICD_GEMM_LN_COMPUTE
TUNE = dict(WM2=0x40000, WM4=0x80000, FORCE_BIG=0x100000, NO_BIG=0x200000, BN256=0x400000, NO_LN_INLINE=0x800000, PP_V1=0x10000000,
            NO_PP=0x20000000)
AMPLE = 1 << 40

EDGE_M = (1, 127, 128, 255, 256, 257, 2048, 8192, 32768, 131072)
EDGE_N = (8, 136, 320, 640, 1280, 2560, 5120, 10240)
EDGE_K = (8, 72, 320, 640, 1024, 1280, 2048, 5120, 8192, 11520)
# the shapes the tuning flags, epilogues and LN_COMPUTE are crossed with: one per planner regime (a full chip of big tiles, a partly filled
# one, a split-K candidate, a launch below the big tiles, one with 40 n-tiles)
PROBE = ((8192, 1280, 1280), (2048, 2560, 1280), (2048, 1280, 1280), (512, 1280, 5120), (255, 640, 2048), (8192, 10240, 1280), (32768, 320, 320))


def big_cfg(i):
    return (i + 1) << 24


def unet_shapes(cfg, res, B):
    """(kind, M, N, K, extra) of every GEMM / conv launch of one forward: latent res x res, B samples, 77 context tokens."""
    ch, L, X, temb = cfg.block_out_channels, cfg.num_levels, cfg.cross_dim, cfg.temb_dim
    hw = [(res >> i) ** 2 for i in range(L)]
    out = [("conv", B * hw[0], ch[0], 9 * 8, dict(H=res, C0=8)), ("conv", B * hw[0], 8, 9 * ch[0], dict(H=res, C0=ch[0])),      # conv_in / conv_out, channels padded to 8
           ("dense", B, temb, ch[0], {}), ("dense", B, temb, temb, {}), ("dense", B, ch[0], cfg.time_cond_proj_dim, {})]
    if cfg.add_in_dim:
        out.append(("dense", B, temb, cfg.add_in_dim, {}))
    lvl_of = [i for i in range(L) for _ in range(cfg.layers_per_block)] + [L - 1, L - 1] + [L - 1 - i for i in range(L) for _ in range(cfg.layers_per_block + 1)]
    for (_, ci, co), lvl in zip(cfg.resnet_names(), lvl_of):
        M, side = B * hw[lvl], res >> lvl
        out += [("conv", M, co, 9 * ci, dict(H=side, C0=ci)), ("conv", M, co, 9 * co, dict(H=side, C0=co)), ("dense", B, co, temb, {})]
        if ci != co:
            out.append(("dense", M, co, ci, {}))
    for i in range(L - 1):
        side = res >> i
        out.append(("conv", B * hw[i + 1], ch[i], 9 * ch[i], dict(H=side, C0=ch[i], stride=2)))
        out.append(("conv", B * hw[i], ch[i + 1], 9 * ch[i + 1], dict(H=side >> 1, C0=ch[i + 1], upsample=1)))
        out.append(("phase", B * hw[i + 1], ch[i + 1], 4 * ch[i + 1], dict(H=side >> 1, C0=ch[i + 1])))
    tlvl = [i for i in range(L) if cfg.down_has_attn[i] for _ in range(cfg.layers_per_block)] + [L - 1] + \
           [L - 1 - i for i in range(L) if cfg.up_has_attn[i] for _ in range(cfg.layers_per_block + 1)]
    for (_, c, _, _, _), lvl in zip(cfg.transformer_names(), tlvl):
        M = B * hw[lvl]
        out += [("dense", M, c, c, {}), ("ln", M, c, c, {}), ("ln", M, 2 * c, c, {}), ("trans", M, c, c, dict(rps=hw[lvl])),
                ("dense", B * 77, c, X, {}), ("trans", B * 77, c, X, dict(rps=77, ldo=80)), ("geglu", M, 8 * c, c, {}), ("dense", M, c, 4 * c, {})]
        if hw[lvl] % 256 == 0 and c % 128 == 0:
            out.append(("xattn", M, c, c, dict(rps=hw[lvl])))
    return out


def _conv(M, N, K, H, C0, stride=1, upsample=0, C1=0, flags=0, **fields):
    """Square conv geometry with B = M / (Hout Wout) samples; K fixes the taps (9 or 1) over C0 + C1 channels."""
    Ho = H * 2 if upsample else (H + stride - 1) // stride
    d = conv_desc(dict(B=1, H=H, W=H, C0=C0, C1=C1, Co=N, stride=stride), flags)
    d.M, d.K, d.ldw, d.Hout, d.Wout, d.rows_per_sample, d.upsample = M, K, K, Ho, Ho, Ho * Ho, upsample
    d.ksize = 3 if K == 9 * (C0 + C1) else 1
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _xattn(M, N, K, rps, nk=77, tile=0, flags=0, **fields):
    ldvt = (nk + 7) // 8 * 8
    kw = dict(rows_per_sample=rps, xattn_k=dummy(), xattn_vt=dummy(), xattn_nk=nk, xattn_ldk=N, xattn_ldvt=ldvt, xattn_vt_bs=N * ldvt,
              xattn_scale=0.125, tune_xattn_tile=tile)
    if flags & LNC:
        kw.update(ln_stats=dummy(), ln_colsum=dummy())
    kw.update(fields)
    return dense_desc(M, N, K, flags, **kw)


def _ln(M, N, K, flags=0, **fields):
    return dense_desc(M, N, K, flags | LNC, ln_stats=dummy(), ln_colsum=dummy(), **fields)


def _of_kind(kind, M, N, K, x, flags=0):
    if kind == "conv":
        return _conv(M, N, K, flags=flags, **x)
    if kind == "phase":
        d = conv_desc(dict(B=M // (x["H"] ** 2), H=x["H"], W=x["H"], C0=x["C0"], C1=0, Co=N), flags, tap_base=x.get("tap_base", 4))
        return d
    if kind == "ln":
        return _ln(M, N, K, flags)
    if kind == "trans":
        return dense_desc(M, N, K, flags | TRANS, rows_per_sample=x["rps"], ldo=x.get("ldo", x["rps"]))
    if kind == "geglu":
        return dense_desc(M, N, K, flags | GEGLU, ldo=N // 2, bias=dummy())
    if kind == "xattn":
        return _xattn(M, N, K, x["rps"], flags=flags | LNC)
    return dense_desc(M, N, K, flags, bias=dummy(), resid=dummy(), ldr=N)


def _with_ws(name, make, need):
    """The descriptor without workspace, with the requested bytes, with half of them, and with more than any split needs."""
    sizes = [("ws0", 0), ("ample", AMPLE)] + ([("ws", need), ("half", need // 2)] if need > 0 else [])
    for tag, n in sizes:
        d = make()
        d.splitk_ws, d.splitk_ws_bytes = (dummy() if n else None), n
        yield f"{name} {tag}", d


def cases(ws_bytes):
    """[(name, descriptor)]; ws_bytes(M, N, K) supplies the 'requested workspace' inputs (the library's icd_gemm_workspace_bytes)."""
    out = []
    add = lambda name, d: out.append((name, d))
    # ---- 1. the UNet forwards
    seen = set()
    for cfg, res, batches in ((SD15, 64, (1, 2, 8, 32)), (SDXL, 128, (1, 2, 8, 16))):
        for B in batches:
            for kind, M, N, K, x in unet_shapes(cfg, res, B):
                key = (kind, M, N, K, tuple(sorted(x.items())))
                if key in seen:
                    continue
                seen.add(key)
                for nm, d in _with_ws(f"unet {kind} {M}x{N}x{K} {x}", lambda: _of_kind(kind, M, N, K, x), ws_bytes(M, N, K)):
                    add(nm, d)
    # ---- 2. edge shapes x workspace
    for M in EDGE_M:
        for N in EDGE_N:
            for K in EDGE_K:
                for nm, d in _with_ws(f"edge {M}x{N}x{K}", lambda: dense_desc(M, N, K), ws_bytes(M, N, K)):
                    add(nm, d)
    # ---- 3. epilogues, tuning flags and forced tiles on the probe shapes
    for M, N, K in PROBE:
        need, tag = ws_bytes(M, N, K), f"{M}x{N}x{K}"
        ws = dict(splitk_ws=dummy(), splitk_ws_bytes=need) if need else {}
        if N % 64 == 0:
            add(f"geglu {tag}", dense_desc(M, N, K, GEGLU, ldo=N // 2, **ws))
        add(f"out_f32 flag {tag}", dense_desc(M, N, K, F32, **ws))
        add(f"resid_f32 {tag}", dense_desc(M, N, K, RF32, resid=dummy(), ldr=N, **ws))
        add(f"out_f32 twin {tag}", dense_desc(M, N, K, out_f32=dummy(), **ws))
        add(f"carries {tag}", dense_desc(M, N, K, resid=dummy(), ldr=N, resid_carry=dummy(), out_carry=dummy(), **ws))
        add(f"out_carry {tag}", dense_desc(M, N, K, out_carry=dummy()))
        add(f"batched {tag}", dense_desc(M, N, K, batch=4, zdiv=2))
        add(f"Nw<N {tag}", dense_desc(M, N, K, Nw=N - 8))
        for rps, ldo in ((256, 256), (256, 272), (M // 4 if M % 128 == 0 else 77, None), (77, 80), (100, 100)):
            if rps and M % rps == 0 or rps in (77, 100):
                add(f"trans rps {rps} ldo {ldo or rps} {tag}", dense_desc(M, N, K, TRANS, rows_per_sample=rps, ldo=ldo or rps, **ws))
        for name, f in TUNE.items():
            add(f"tune {name} {tag}", dense_desc(M, N, K, f, **ws))
            add(f"tune {name} ln {tag}", _ln(M, N, K, f, **ws))
        add(f"tune NO_BIG|WM2 {tag}", dense_desc(M, N, K, TUNE["NO_BIG"] | TUNE["WM2"], **ws))
        add(f"tune NO_BIG|WM4 {tag}", dense_desc(M, N, K, TUNE["NO_BIG"] | TUNE["WM4"], **ws))
        for i in range(9):                                   # 7 and 8 name no tile
            add(f"cfg {i} {tag}", dense_desc(M, N, K, big_cfg(i), **ws))
            add(f"cfg {i} no ws {tag}", dense_desc(M, N, K, big_cfg(i)))
            add(f"cfg {i} ln {tag}", _ln(M, N, K, big_cfg(i)))
            if N % 64 == 0:
                add(f"cfg {i} geglu {tag}", dense_desc(M, N, K, big_cfg(i) | GEGLU, ldo=N // 2))
            add(f"cfg {i} carry {tag}", dense_desc(M, N, K, big_cfg(i), out_carry=dummy()))
        for gm in (0, 4):
            for f in (0, TUNE["NO_BIG"]):
                add(f"group_m {gm} flags {f:#x} {tag}", dense_desc(M, N, K, f, tune_group_m=gm))
    # ---- 4. LN_COMPUTE: n-tiles on both sides of 12 for every tile width, every disqualifier of the inline statistics
    for M in (2048, 8192):
        for N in (1280, 2560, 3072, 3328, 3840, 4160, 5120, 10240):
            for K in (320, 1280):
                add(f"ln {M}x{N}x{K}", _ln(M, N, K))
                add(f"ln BN256 {M}x{N}x{K}", _ln(M, N, K, TUNE["BN256"]))
                add(f"ln geglu {M}x{N}x{K}", _ln(M, N, K, GEGLU, ldo=N // 2))
    M, N, K = 8192, 1280, 1280
    add("ln trans", _ln(M, N, K, TRANS, rows_per_sample=1024, ldo=1024))
    add("ln resid_f32", _ln(M, N, K, RF32, resid=dummy(), ldr=N))
    add("ln out_carry", _ln(M, N, K, out_carry=dummy()))
    add("ln resid_carry", _ln(M, N, K, resid=dummy(), ldr=N, resid_carry=dummy()))
    add("ln split-K", _ln(512, 1280, 5120, splitk_ws=dummy(), splitk_ws_bytes=AMPLE))
    add("ln eps", _ln(M, N, K, ln_eps=1e-6))
    add("ln precomputed statistics", dense_desc(M, N, K, ln_stats=dummy(), ln_colsum=dummy()))
    add("ln inline, lda != K", _ln(M, N, K, lda=K + 8))
    add("ln separate pass, lda != K", _ln(M, N, K, TUNE["NO_LN_INLINE"], lda=K + 8))
    # ---- 5. conv mode
    for C0, C1 in ((64, 0), (320, 0), (64, 64), (320, 640), (24, 8), (72, 0)):
        for stride, up in ((1, 0), (2, 0), (1, 1)):
            for B, H in ((1, 8), (2, 32), (8, 64)):
                for Co in (8, 640):
                    Ho = H * 2 if up else (H + stride - 1) // stride
                    mk = lambda f=0: _conv(B * Ho * Ho, Co, 9 * (C0 + C1), H, C0, stride, up, C1, f, a1=dummy() if C1 else None)
                    need = ws_bytes(B * Ho * Ho, Co, 9 * (C0 + C1))
                    for nm, d in _with_ws(f"conv C {C0}+{C1} s{stride} u{up} B{B} H{H} Co{Co}", mk, need):
                        add(nm, d)
                    for name in ("WM4", "FORCE_BIG", "NO_PP"):
                        add(f"conv C {C0}+{C1} s{stride} u{up} B{B} H{H} Co{Co} {name}", mk(TUNE[name]))
    for i in range(7):
        add(f"conv cfg {i}", _conv(8 * 32 * 32, 1280, 9 * 640, 32, 640, flags=big_cfg(i)))
        add(f"conv cfg {i} carry", _conv(8 * 32 * 32, 1280, 9 * 640, 32, 640, flags=big_cfg(i), out_carry=dummy(), resid=dummy(), ldr=1280, resid_carry=dummy()))
    add("conv 1x1", _conv(8 * 32 * 32, 640, 320, 32, 320))
    add("conv 1x1 general", _conv(8 * 32 * 32, 640, 24, 32, 24))
    add("conv pad_hi stride 2", _conv(8 * 16 * 16, 128, 9 * 128, 32, 128, stride=2, flags=8))
    add("conv transposed output on a big tile", _conv(8 * 32 * 32, 1280, 9 * 640, 32, 640, flags=TRANS | TUNE["FORCE_BIG"], ldo=1024))
    add("conv transposed output, 128-wide", _conv(8 * 32 * 32, 1280, 9 * 640, 32, 640, flags=TRANS | TUNE["NO_BIG"]))
    add("conv batched", _conv(8 * 32 * 32, 1280, 9 * 640, 32, 640, batch=2))
    add("conv rows_per_sample unset", _conv(8 * 32 * 32, 1280, 9 * 640, 32, 640, rows_per_sample=0))
    for t0 in (0, 1, 3, 4):
        for C0, B, H, Co in ((16, 2, 6, 24), (640, 8, 32, 640), (1280, 8, 16, 1280)):
            add(f"phase t0 {t0} C {C0} B{B} H{H}", conv_desc(dict(B=B, H=H, W=H, C0=C0, C1=0, Co=Co), tap_base=t0))
            add(f"phase t0 {t0} C {C0} B{B} H{H} carry", conv_desc(dict(B=B, H=H, W=H, C0=C0, C1=0, Co=Co), tap_base=t0, out_carry=dummy()))
    for B in (255, 256):                                     # 8 MiB per sample: under and over conv_fast's 2 GiB - 4 MiB per source
        add(f"conv source {B} x 8 MiB", _conv(B * 65536, 320, 576, 256, 64))
        add(f"conv second source {B} x 8 MiB", _conv(B * 65536, 320, 9 * 128, 256, 64, C1=64, a1=dummy()))
    # ---- 6. query projection + cross-attention in one launch
    for rps in (256, 1024, 4096):
        for B in (1, 2, 6, 7):
            for N in (128, 512, 1280, 4096):
                for tile in (0, 2, 4, 5, 6):
                    for f in (0, LNC):
                        add(f"xattn rps {rps} B{B} N{N} tile {tile} flags {f}", _xattn(B * rps, N, 640, rps, tile=tile, flags=f))
    for nk in (77, 80, 81, 96):
        for B in (1, 8):
            for tile in (0, 2, 4, 5, 6):
                add(f"xattn keys {nk} B{B} tile {tile}", _xattn(B * 1024, 1280, 1280, 1024, nk=nk, tile=tile, flags=LNC, bias=dummy()))
    add("xattn NO_LN_INLINE", _xattn(8192, 1280, 1280, 1024, flags=LNC | TUNE["NO_LN_INLINE"]))
    add("xattn group_m 4", _xattn(8192, 4096, 1280, 1024, tile=2, tune_group_m=4))
    # ---- 7. operands around the 31-bit offsets of the ping-pong tiles (pp_operands_ok: 2^31 - 4096 bytes)
    for M in (1048573, 1048574, 1048575):                    # A: ((M - 1) 1024 + 1024) 2 bytes
        add(f"A extent M {M}", dense_desc(M, 256, 1024))
        add(f"A extent M {M} cfg 4", dense_desc(M, 256, 1024, big_cfg(4)))
    for lda in (131056, 131064, 131072):                     # ... through the row stride: (8191 lda + 1024) 2 bytes
        add(f"A extent lda {lda}", dense_desc(8192, 1280, 1024, lda=lda))
    for ldw in (104856, 104864, 104872):                     # W: (10239 ldw + 1024) 2 bytes
        add(f"W extent ldw {ldw}", dense_desc(8192, 10240, 1024, ldw=ldw))
        add(f"W extent ldw {ldw} conv", _conv(8 * 32 * 32, 10240, 9 * 640, 32, 640, ldw=ldw * 2))
    add("negative lda", dense_desc(8192, 1280, 1280, lda=-1280))
    # ---- 8. the refusal table, and the two accepted descriptors whose checks moved in front of the tile choice
    for name, make, _ in REFUSALS:
        add(f"refusal: {name}", make())
        d = make()
        d.flags |= TUNE["FORCE_BIG"]
        add(f"refusal + FORCE_BIG: {name}", d)
    add("null a0", dense_desc(128, 128, 64, a0=None))
    add("M = 0", dense_desc(0, 128, 64))
    add("xattn without vt", _xattn(256, 128, 64, 256, xattn_vt=None))
    add("xattn + GEGLU", _xattn(256, 128, 64, 256, flags=GEGLU, ldo=64))
    add("xattn lda % 8", _xattn(256, 128, 64, 256, lda=68))
    add("xattn + out_carry", _xattn(256, 128, 64, 256, out_carry=dummy()))
    add("conv channels % 8", _conv(64, 8, 9 * 24, 8, 12, C1=12))
    add("conv C0 = 0 on a big tile", _conv(8 * 32 * 32, 640, 9 * 64, 32, 0, C1=64))
    add("conv C0 = 0, 128-wide", _conv(64, 8, 9 * 64, 8, 0, C1=64))
    add("conv Hin = 0", _conv(64, 8, 72, 8, 8, Hin=0))
    add("phase with upsample", conv_desc(dict(B=1, H=4, W=4, C0=8, C1=0, Co=8), tap_base=0, upsample=1))
    add("out_remap_w = 1", conv_desc(dict(B=1, H=4, W=1, C0=8, C1=0, Co=8), tap_base=0))
    add("carry ldo % 8", dense_desc(128, 128, 64, out_carry=dummy(), ldo=132))
    return out


def record(lib):
    """({"plans": [[rc, kernel, tile_m, tile_n, ksplit, ln_inline, xattn, cfg, group_m]], "workspace": [bytes]}, names, messages): the plans
    in the order of cases(), the workspace of every distinct (M, N, K) with positive dimensions in sorted order."""
    ws = lambda M, N, K: int(lib.icd_gemm_workspace_bytes(M, N, K))
    cs = cases(ws)
    plans, msgs = [], []
    for _, d in cs:
        info = _lib.GemmPlanInfo()
        rc = lib.icd_gemm_plan(C.byref(d), C.byref(info))
        plans.append([rc] + [getattr(info, f) for f in FIELDS])
        msgs.append(lib.icd_last_error().decode() if rc else "")
    shapes = sorted({(d.M, d.N, d.K) for _, d in cs if d.M > 0 and d.N > 0 and d.K > 0})
    return {"plans": plans, "workspace": [ws(*s) for s in shapes]}, [n for n, _ in cs], msgs


def check_coverage(plans):
    ok = [p for p in plans if p[0] == 0]
    col = lambda f: {p[1 + FIELDS.index(f)] for p in ok}
    assert col("cfg") >= set(range(-1, 7)) | {100, 101}, sorted(col("cfg"))
    assert col("group_m") >= {1, 4, 8} and col("ln_inline") == {0, 1} and col("xattn") == {0, 1}
    assert col("ksplit") >= set(range(1, 9)), sorted(col("ksplit"))
    assert col("kernel") == {0, 1} and col("tile_m") >= {128, 192, 256} and col("tile_n") >= {128, 256, 320}
    assert sum(p[0] != 0 for p in plans) >= len(REFUSALS)


if __name__ == "__main__":
    got, names, _ = record(_lib.load())
    assert len(set(names)) == len(names), "case names must be unique"
    check_coverage(got["plans"])
    print(f"{len(names)} descriptors, {sum(p[0] != 0 for p in got['plans'])} refused, {len(got['workspace'])} workspace shapes")
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            f.write('{"fields": ' + json.dumps(["rc"] + list(FIELDS)) + ',\n"plans": [\n' +
                    ",\n".join(json.dumps(p, separators=(",", ":")) for p in got["plans"]) + '],\n"workspace": ' +
                    json.dumps(got["workspace"], separators=(",", ":")) + "}\n")
        print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
