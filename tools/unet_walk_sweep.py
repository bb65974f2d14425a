#!/usr/bin/env python3
"""Inputs for the dry walk of the UNet executor (csrc/runtime.hip), and the recording of what it answers.

    python tools/unet_walk_sweep.py --write        # tests/golden/unet_walk.json from the loaded library

create / set_option / finalize / workspace_bytes_ex / kv_cache_bytes are host-only: the dry walk runs the executor's whole control flow
against an arena that only counts, so its byte count moves whenever a buffer is allocated, sized or released differently, and finalize's
message (how many tensors are not bound on an empty handle, and the first of them) moves whenever a tensor lookup appears, disappears or
changes its place.  cases() is a deterministic list of (name, config, options, shape) - inputs only.  record() asks the library.
tests/test_unet_walk.py replays cases() against the golden file, which was written once from the executor as it stood BEFORE it was
taken apart into one function per block and is not to be regenerated: a walk that changes on purpose changes its rows with the reason
in the commit.  (ICD_AMD_LIB selects the build that is recorded.)
"""
import ctypes as C
import json
import os
import sys
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from invertible_cd_amd import _lib                                                          # noqa: E402
from invertible_cd_amd.unet_config import SD15, SDXL                                        # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "unet_walk.json")
FIELDS = ("workspace_bytes", "kv_cache_bytes", "attention_layers")
NO_BIG = 0x200000                                            # ICD_GEMM_TUNE_NO_BIG
SPLIT_BITS = tuple(1 << i for i in range(10))                # ICD_SPLIT_GN .. ICD_SPLIT_UP_ALL
DEFAULTS = dict(residual=3, split_mask=_lib.ICD_SPLIT_DEFAULT, xattn_fusion=2, ffn_fusion=2, upsample_phases=1, ln_inline_stats=1, gemm_tune=0)
OPTION_IDS = dict(residual=_lib.ICD_UNET_OPT_RESIDUAL_MODE, split_mask=_lib.ICD_UNET_OPT_SPLIT_MASK, xattn_fusion=_lib.ICD_UNET_OPT_XATTN_FUSION,
                  ffn_fusion=_lib.ICD_UNET_OPT_FFN_FUSION, upsample_phases=_lib.ICD_UNET_OPT_UPSAMPLE_PHASES,
                  ln_inline_stats=_lib.ICD_UNET_OPT_LN_INLINE_STATS, gemm_tune=_lib.ICD_UNET_OPT_GEMM_TUNE)

CONFIGS = {
    "sd15": SD15,
    "sdxl": SDXL,
    "sd15_tiny": SD15.scaled((64, 128, 256, 256), cross_dim=64),
    "sdxl_tiny": SDXL.scaled((64, 128, 256), cross_dim=128, heads=(2, 4, 8)),
    # two levels, attention on the first only, one resnet per level, no guidance embedding
    "two_level": replace(SD15, name="two_level", block_out_channels=(64, 128), down_has_attn=(True, False), up_has_attn=(False, True),
                         transformer_layers=(1, 1), num_heads=(2, 4), cross_dim=40, layers_per_block=1, time_cond_proj_dim=0),
    # three levels, two transformer blocks in the middle one, attention everywhere
    "three_level": replace(SD15, name="three_level", block_out_channels=(32, 64, 64), down_has_attn=(True, True, True),
                           up_has_attn=(True, True, True), transformer_layers=(1, 2, 1), num_heads=(4, 4, 2), cross_dim=48),
    # a C = 320 level (the fused feed-forward) above a channel-keeping one
    "c320": replace(SDXL, name="c320", block_out_channels=(320, 320, 128), down_has_attn=(True, True, False), up_has_attn=(False, True, True),
                    transformer_layers=(1, 1, 1), num_heads=(5, 5, 2), cross_dim=64, pooled_dim=64),
    # head dim 64 on C = 256 and C = 512 (the fused cross-attention launch on its 256-wide and 128-wide hosts)
    "d64": replace(SD15, name="d64", block_out_channels=(256, 512), down_has_attn=(True, True), up_has_attn=(True, True),
                   transformer_layers=(1, 1), num_heads=(4, 8), cross_dim=64),
}

BATCHES = (1, 2, 8, 32)
NCTX = (8, 77, 96, 154)


def latents(cfg):
    """(H, W): the smallest legal (one pixel at the deepest level), 16 x 16, 64 x 64, a non-square one, 128 x 128."""
    div = 1 << (cfg.num_levels - 1)
    return ((div, div), (16, 16), (64, 64), (16, 3 * div), (128, 128))


def option_sets():
    """Each option one at a time from the defaults, plus the pairs that interact."""
    sets = [{}]
    masks = (0,) + SPLIT_BITS + (_lib.ICD_SPLIT_DEFAULT, _lib.ICD_SPLIT_ALL)
    sets += [dict(residual=r, split_mask=m) for r in range(4) for m in masks]
    sets += [dict(xattn_fusion=v) for v in range(3)]
    sets += [dict(ffn_fusion=f, gemm_tune=g) for f in range(3) for g in (0, NO_BIG)]
    sets += [dict(upsample_phases=v) for v in (0, 1)] + [dict(ln_inline_stats=v) for v in (0, 1)]
    out, seen = [], set()
    for s in sets:
        full = dict(DEFAULTS, **s)
        key = tuple(sorted(full.items()))
        if key not in seen:
            seen.add(key)
            out.append(full)
    return out


def opt_name(o):
    return " ".join(f"{k}={v:#x}" if k in ("split_mask", "gemm_tune") else f"{k}={v}" for k, v in o.items() if v != DEFAULTS[k]) or "defaults"


def cases():
    """[(name, config name, options, (B, H, W, n_ctx, probs_mode))]."""
    out, seen = [], set()

    def add(cn, o, shape):
        name = f"{cn} | {opt_name(o)} | B{shape[0]} {shape[1]}x{shape[2]} ctx{shape[3]} probs{shape[4]}"
        if name not in seen:
            seen.add(name)
            out.append((name, cn, o, shape))

    opts = option_sets()
    for cn, cfg in CONFIGS.items():
        lat = latents(cfg)
        # the defaults over every batch and latent, and every context length and materialisation rule on two latents
        for B in BATCHES:
            for H, W in lat:
                add(cn, opts[0], (B, H, W, 77, 0))
        for n in NCTX:
            for pm in (0, 1, 2):
                add(cn, opts[0], (2, 16, 16, n, pm))
                add(cn, opts[0], (1, 64, 64, n, pm))
        # every option set over six shapes: the one-pixel level, both sides of each fusion rule's size threshold, a non-square latent
        for o in opts[1:]:
            add(cn, o, (1,) + lat[0] + (8, 0))
            add(cn, o, (2, 16, 16, 77, 1))
            add(cn, o, (8, 64, 64, 77, 0))
            add(cn, o, (2,) + lat[3] + (96, 2))
            add(cn, o, (32, 64, 64, 154, 0))
            add(cn, o, (8, 128, 128, 96, 0))
    return out


# ---- what a case reaches, from its inputs alone (coverage of the sweep; tests/test_unet_walk.py asserts it)
def reaches(cfg, o, shape):
    """Which branches of the walk the case takes: {"xattn": fused cross-attention launch somewhere, "ffn": fused feed-forward somewhere,
    "up3x3": the 3 x 3 upsampler although the phase form is on}.  The two rules are those documented at icd_unet_set_option."""
    B, H, W, nctx, pm = shape
    x = f = False
    for lvl, has in enumerate(cfg.down_has_attn):
        up_has = cfg.up_has_attn[cfg.num_levels - 1 - lvl]
        if not (has or up_has or lvl == cfg.num_levels - 1):
            continue
        Cc, HW = cfg.block_out_channels[lvl], (H >> lvl) * (W >> lvl)
        M, d = B * HW, cfg.block_out_channels[lvl] // cfg.num_heads[lvl]
        auto = Cc % 256 == 0 and (M // 256) * (Cc // 256) >= 64 and B * ((HW + 191) // 192) * (Cc // 256) <= 512
        mat = pm != 0                                        # (a dry walk materialises every cross-attention layer under rules 1 and 2)
        x |= (not mat) and d == 64 and Cc % 128 == 0 and HW % 256 == 0 and nctx <= 96 and (o["xattn_fusion"] == 1 or (o["xattn_fusion"] == 2 and auto))
        f |= Cc == 320 and (o["ffn_fusion"] == 1 or (o["ffn_fusion"] == 2 and M >= 65536 and o["gemm_tune"] == 0))
    return dict(xattn=x, ffn=f, up3x3=bool(o["upsample_phases"]) and (W >> (cfg.num_levels - 1)) < 2)


def c_config(cfg):
    c = _lib.UNetConfig()
    c.in_channels, c.out_channels, c.num_levels = cfg.in_channels, cfg.out_channels, cfg.num_levels
    for i in range(cfg.num_levels):
        c.block_out_channels[i] = cfg.block_out_channels[i]
        c.down_has_attn[i], c.up_has_attn[i] = int(cfg.down_has_attn[i]), int(cfg.up_has_attn[i])
        c.transformer_layers[i], c.num_heads[i] = cfg.transformer_layers[i], cfg.num_heads[i]
    c.layers_per_block, c.cross_dim, c.use_linear_projection = cfg.layers_per_block, cfg.cross_dim, int(cfg.use_linear_projection)
    c.time_cond_proj_dim, c.addition_time_embed_dim = cfg.time_cond_proj_dim, cfg.addition_time_embed_dim
    c.add_in_dim, c.norm_groups = cfg.add_in_dim, cfg.norm_groups
    return c


def record(lib):
    """({"rows": [[workspace_bytes_ex, kv_cache_bytes, attention layers]], "finalize": {"config | options": [rc, message]}}, names)."""
    cs = cases()
    rows, fin, handles = [], {}, {}
    for name, cn, o, (B, H, W, nctx, pm) in cs:
        key = f"{cn} | {opt_name(o)}"
        if key not in handles:
            h = C.c_void_p()
            c = c_config(CONFIGS[cn])
            assert lib.icd_unet_create(C.byref(c), C.byref(h)) == 0, lib.icd_last_error()
            for k, v in o.items():
                assert lib.icd_unet_set_option(h, OPTION_IDS[k], v) == 0, lib.icd_last_error()
            rc = lib.icd_unet_finalize(h)                    # nothing is bound: the count of tensors the walk asks for, and the first
            fin[key] = [rc, lib.icd_last_error().decode() if rc else ""]
            handles[key] = h
        h = handles[key]
        rows.append([int(lib.icd_unet_workspace_bytes_ex(h, B, H, W, nctx, pm)), int(lib.icd_unet_kv_cache_bytes(h, B, nctx)),
                     int(lib.icd_unet_num_attention_layers(h))])
    for h in handles.values():
        lib.icd_unet_destroy(h)
    return {"rows": rows, "finalize": fin}, [c[0] for c in cs]


def check_coverage(cs):
    """Both fusion rules fire for some cases and not for others, every residual mode appears, the 3 x 3 upsampler fallback is reached."""
    hit = [reaches(CONFIGS[cn], o, shape) for _, cn, o, shape in cs]
    for k in ("xattn", "ffn", "up3x3"):
        assert any(h[k] for h in hit) and not all(h[k] for h in hit), k
    # ... under the measured rule (mode 2) as well as the forced one
    assert any(h["xattn"] for h, c in zip(hit, cs) if c[2]["xattn_fusion"] == 2) and any(h["ffn"] for h, c in zip(hit, cs) if c[2]["ffn_fusion"] == 2)
    assert {c[2]["residual"] for c in cs} == {0, 1, 2, 3}
    assert {c[2]["split_mask"] for c in cs} >= set(SPLIT_BITS) | {0, _lib.ICD_SPLIT_DEFAULT, _lib.ICD_SPLIT_ALL}


if __name__ == "__main__":
    got, names = record(_lib.load())
    assert len(set(names)) == len(names), "case names must be unique"
    check_coverage(cases())
    print(f"{len(names)} cases on {len(got['finalize'])} handles, library {_lib.LIB_PATH}")
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            f.write('{"fields": ' + json.dumps(list(FIELDS)) + ',\n"rows": [\n' +
                    ",\n".join(json.dumps(r, separators=(",", ":")) for r in got["rows"]) + '],\n"finalize": {\n' +
                    ",\n".join(json.dumps(k) + ": " + json.dumps(v) for k, v in got["finalize"].items()) + "}}\n")
        print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
