#!/usr/bin/env python3
"""Two builds of the library, one machine: the same bits out of icd_unet_forward and the same launches, in the same order.

    ICD_AMD_LIB=/path/to/other/libicd_amd.so python tools/unet_ab_exact.py [--cases name,name] [--timeout 180]

For a refactor of the executor (csrc/runtime.hip) that must not move a launch.  Per case two fresh child processes, each under a time
limit: one loads the tree's library, the other the build named by ICD_AMD_LIB.  A child runs the case's forwards on synthetic weights with
the profiler on and prints, per forward, the sha256 of the eps bytes and the ordered launch list (family, M, N, K, aux, tile_m, tile_n,
plan_flags, ksplit) of icd_profile_dump.  The tool compares the two printouts and stops at the first child that exits abnormally - nothing
more is started on the GPU after that.  A one-off comparison, not a test: a committed hash would break on the next kernel change.
"""
import hashlib
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> dict(cfg, H, W, options, and what else the case needs); B = 2, n_ctx = 77 throughout
SD15_TINY = ("sd15_tiny", 16, 16)
CASES = {
    **{f"sd15_tiny residual={r}": dict(shape=SD15_TINY, options={"residual": r}) for r in range(4)},
    "sd15_tiny 8x8 (one-pixel level: 3x3 upsampler)": dict(shape=("sd15_tiny", 8, 8)),
    "sd15_tiny 8x8 upsample_phases=0": dict(shape=("sd15_tiny", 8, 8), options={"upsample_phases": 0}),
    "sd15_tiny upsample_phases=0": dict(shape=SD15_TINY, options={"upsample_phases": 0}),
    "sdxl_tiny defaults (precise time embedding)": dict(shape=("sdxl_tiny", 16, 16)),
    "sdxl_tiny split_mask without TEMB (fp16 time embedding)": dict(shape=("sdxl_tiny", 16, 16), options={"split_mask": 447 & ~128}),
    "sd15_tiny timestep_cond": dict(shape=SD15_TINY, cond=True),
    "sd15_tiny timestep_cond + fp16 time embedding": dict(shape=SD15_TINY, cond=True, options={"split_mask": 447 & ~128}),
    "c320 ffn_fusion=1": dict(shape=("c320", 16, 16), options={"ffn_fusion": 1}),
    "d64 xattn_fusion=1": dict(shape=("d64", 16, 16), options={"xattn_fusion": 1}),
    "sd15_tiny kv_cache: first call then a valid cache": dict(shape=SD15_TINY, forwards=2),
    "sd15_tiny ln_inline_stats=0": dict(shape=SD15_TINY, options={"ln_inline_stats": 0}),
    "sd15_tiny hook materialising every layer": dict(shape=SD15_TINY, controller="every"),
    "sd15_tiny AttentionStore (second half of the batch; probs epilogue on the second step)": dict(shape=SD15_TINY, controller="store", forwards=2),
}


def child(name):
    import importlib.util
    import torch
    from invertible_cd_amd import _lib, p2p, synthetic, unet
    spec = importlib.util.spec_from_file_location("unet_walk_sweep", os.path.join(ROOT, "tools", "unet_walk_sweep.py"))
    sweep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sweep)
    case = CASES[name]
    cn, H, W = case["shape"]
    cfg, B = sweep.CONFIGS[cn], 2
    sd = {k: v.half().float() for k, v in synthetic.synthetic_state_dict(cfg, seed=7).items()}
    inp = synthetic.synthetic_inputs(cfg, B, H, W, seed=7, n_ctx=77)
    model = unet.UNet2DConditionModel(cfg, sd)
    model.set_precision(None)                      # the handle's own options, not the sampler's precision policy
    for k, v in case.get("options", {}).items():
        model.set_option(k, v)
    kw = dict(encoder_hidden_states=inp["context"].half().cuda())
    if case.get("cond"):
        kw["timestep_cond"] = torch.randn(B, cfg.time_cond_proj_dim, generator=torch.Generator().manual_seed(12)).half().cuda()
    if cfg.addition_time_embed_dim:
        kw["added_cond_kwargs"] = {"text_embeds": inp["text_embeds"].half().cuda(), "time_ids": inp["time_ids"].cuda()}
    if case.get("controller") == "store":
        p2p.register_attention_control(types.SimpleNamespace(unet=model), p2p.AttentionStore())
    elif case.get("controller") == "every":
        class Every:                               # a reference-style controller the adapter cannot short-cut: it gets every layer
            num_att_layers = 0

            def __call__(self, attn, is_cross, place):
                return attn
        p2p.register_attention_control(types.SimpleNamespace(unet=model), Every())
    x = inp["latents"].half().cuda()
    out = []
    for _ in range(case.get("forwards", 1)):
        _lib.profile_enable(True)
        try:
            eps = model(x, torch.tensor(519), **kw).sample
            torch.cuda.synchronize()
            recs = [[_lib.PROF_KINDS[r.kind], r.M, r.N, r.K, r.aux, r.tile_m, r.tile_n, r.plan_flags, r.ksplit] for r in _lib._profile_records()]
        finally:
            _lib.profile_enable(False)
        assert torch.isfinite(eps).all()
        out.append({"sha256": hashlib.sha256(eps.cpu().numpy().tobytes()).hexdigest(), "launches": recs})
    print("RESULT " + json.dumps(out))


def run_child(name, lib, timeout):
    env = dict(os.environ)
    env.pop("ICD_AMD_LIB", None)
    if lib:
        env["ICD_AMD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or len(lines) != 1:
        print(f"  child exited with status {r.returncode}:\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
        return None
    return json.loads(lines[0][len("RESULT "):])


def main(argv):
    other = os.environ.get("ICD_AMD_LIB")
    if not other or not os.path.exists(other):
        sys.exit("set ICD_AMD_LIB to the other build of libicd_amd.so")
    timeout = int(argv[argv.index("--timeout") + 1]) if "--timeout" in argv else 180
    names = argv[argv.index("--cases") + 1].split(",") if "--cases" in argv else list(CASES)
    print(f"tree build against {os.path.basename(os.path.dirname(os.path.dirname(other))) or other}: eps bytes and launch lists, B = 2, 77 context tokens")
    differ = 0
    for name in names:
        try:
            a = run_child(name, None, timeout)
            b = run_child(name, other, timeout) if a is not None else None
        except subprocess.TimeoutExpired:
            print(f"{name}: a child ran into its time limit of {timeout} s; stopping")
            return 2
        if a is None or b is None:
            print(f"{name}: abnormal exit; stopping")
            return 2
        for i, (fa, fb) in enumerate(zip(a, b)):
            same_bits, same_launches = fa["sha256"] == fb["sha256"], fa["launches"] == fb["launches"]
            fam = {}
            for rec in fa["launches"]:
                fam[rec[0]] = fam.get(rec[0], 0) + 1
            print(f"{name} [forward {i + 1}]: eps {'EQUAL' if same_bits else 'DIFFER'} ({fa['sha256'][:16]} / {fb['sha256'][:16]}), "
                  f"{len(fa['launches'])} / {len(fb['launches'])} launches {'EQUAL' if same_launches else 'DIFFER'}  "
                  + " ".join(f"{k}:{v}" for k, v in sorted(fam.items())))
            if not same_launches:
                first = next((j for j, (p, q) in enumerate(zip(fa["launches"], fb["launches"])) if p != q), min(len(fa["launches"]), len(fb["launches"])))
                print(f"    first difference at launch {first}: {fa['launches'][first:first + 1]} / {fb['launches'][first:first + 1]}")
            differ += (not same_bits) + (not same_launches)
    print(f"{len(names)} cases, {differ} differences")
    return 1 if differ else 0


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1])
    else:
        sys.exit(main(sys.argv))
