#!/usr/bin/env python3
"""icd_attention_wide against the three-launch materialised path (icd_gemm scores -> icd_softmax_rows -> icd_gemm apply, chunked to
<= 1 GiB of fp32 scores) it replaces in the VAE mid-block: same process, the two forms alternating rep by rep, device events around
each timed batch of calls.

  * the attention alone at d = 512, H = 1: B = 8 N = 1024, B = 8 N = 4096, B = 2 N = 16384 (256^2, 512^2 and 1024^2 images);
  * AutoencoderKL.decode (fp16 path, full SD width, synthetic weights) with fused_attention True / False at 512^2 B = 8 and 1024^2 B = 2.

The table names the kernel sources' digest and, per attention row, the share of the least time the chip could take:
max(4 B N^2 d flop / 2.5 PFLOP/s, 8 B N d bytes / 6.3 TB/s).

    python tools/attn_wide_bench.py [--reps 7] [--out profiles/attn_wide.txt] [--no-vae]
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from invertible_cd_amd import _lib, ops, synthetic, vae

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--no-vae", action="store_true")
a = ap.parse_args()
MFMA, HBM = 2.5e15, 6.3e12


def materialised(q, k, vt, B, N, Cc, ld, scale):
    """the scores branch of AutoencoderKL._attend"""
    o = torch.empty((B * N, Cc), device=q.device, dtype=torch.float16)
    step = max(1, min(B, (1 << 30) // (N * ld * 4)))
    for b0 in range(0, B, step):
        bc = min(step, B - b0)
        s = ops.attention_scores(q[b0 * N:(b0 + bc) * N], k[b0 * N:(b0 + bc) * N], bc, 1, N, N, Cc, scale, ld)
        pr = ops.softmax_rows(s.reshape(bc * N, ld), N, ld).reshape(bc, N, ld)
        ops.attention_apply(pr, vt[b0:b0 + bc], bc, 1, N, Cc, out=o[b0 * N:(b0 + bc) * N])
    return o


def alternate(fns, inner, reps):
    """median ms per call of each fn: warm every form, then `reps` rounds in which the forms take turns, `inner` calls per turn"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1) / inner)
    return [(statistics.median(m), min(m), max(m)) for m in ms]


lines = [f"icd_attention_wide vs the materialised path; kernels_sha {_lib.build_sha()}; {torch.cuda.get_device_name(0)}; median (min - max) of "
         f"{a.reps} alternating rounds", "",
         "attention alone, d = 512, H = 1, fp16 (TFLOP/s of 4 B N^2 d; floor = max(flop / 2.5 PFLOP/s, q k v out bytes / 6.3 TB/s), MFMA-bound in every row)",
         f"{'B':>3} {'N':>6} | {'wide ms':>22} {'TF/s':>6} {'of floor':>8} | {'materialised ms':>22} {'TF/s':>6} | {'wide / mat':>10} {'rel-L2 between':>14}"]
d = 512
for B, N in ((8, 1024), (8, 4096), (2, 16384)):
    g = torch.Generator(device="cuda").manual_seed(N)
    q, k = (torch.randn(B * N, d, device="cuda", generator=g).half() for _ in range(2))
    vt = torch.randn(B, d, N, device="cuda", generator=g).half()
    scale, ld = d ** -0.5, N
    ow, om = ops.attention_wide(q, k, vt, B, 1, N, N, d, scale), materialised(q, k, vt, B, N, d, ld, scale)
    rel = float((ow.float() - om.float()).norm() / om.float().norm())
    del ow, om
    inner = max(1, min(20, int(2e12 / (4 * B * N * N * d))))
    (w, wlo, whi), (m, mlo, mhi) = alternate([lambda: ops.attention_wide(q, k, vt, B, 1, N, N, d, scale),
                                              lambda: materialised(q, k, vt, B, N, d, ld, scale)], inner, a.reps)
    flop = 4.0 * B * N * N * d
    floor = max(flop / MFMA, 8.0 * B * N * d / HBM) * 1e3
    lines.append(f"{B:>3} {N:>6} | {w:>8.3f} ({wlo:.3f} - {whi:.3f}) {flop / w / 1e9:>6.0f} {floor / w:>8.1%} | {m:>8.3f} ({mlo:.3f} - {mhi:.3f}) "
                 f"{flop / m / 1e9:>6.0f} | {w / m:>10.3f} {rel:>14.2e}")
    print(lines[-1], flush=True)
    del q, k, vt
    torch.cuda.empty_cache()

if not a.no_vae:
    lines += ["", "AutoencoderKL.decode, fp16 path, full SD width (mid-block: one head of 512 channels), ms per image",
              f"{'image':>9} {'B':>3} | {'fused_attention=True':>28} | {'fused_attention=False':>28} | {'True / False':>12}"]
    sd = synthetic.synthetic_vae_state_dict(vae.SD_VAE, seed=0, device="cuda", dtype=torch.float16)
    mw, mm = vae.AutoencoderKL(vae.SD_VAE, sd, fused_attention=True), vae.AutoencoderKL(vae.SD_VAE, sd, fused_attention=False)
    del sd
    for size, B in ((64, 8), (128, 2)):
        z = torch.randn(B, 4, size, size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(size))
        (w, wlo, whi), (m, mlo, mhi) = alternate([lambda: mw.decode(z)["sample"], lambda: mm.decode(z)["sample"]], 1, a.reps)
        lines.append(f"{size * 8:>4}^2    {B:>3} | {w / B:>10.2f} ({wlo / B:.2f} - {whi / B:.2f}) | {m / B:>10.2f} ({mlo / B:.2f} - {mhi / B:.2f}) | {w / m:>12.3f}")
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()

text = "\n".join(lines) + "\n"
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
