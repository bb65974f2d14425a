#!/usr/bin/env python3
"""Real images into the VAE and uint8 images out of it: the host route against the device route (informational, no pass criterion).

    python tools/vae_ingest_bench.py [--n 8] [--reps 5]

In: n image files (PNG, seeded noise) of 512 x 512 and of 1024 x 768 -> the [n, 4, 64, 64] latent of the full-width SD VAE (synthetic
weights).  Host route: generation.load_512 per file (PIL resize), Generator.image2latent's `float() / 127.5 - 1`, the fp32 upload,
vae.encode.  Device route: load_512(..., device=) per file (the raw bytes uploaded), vae.encode_images at 512.  Both are wall time
around a synchronise, the median of --reps after a warm-up, split into the file decode (common to both), the rest of the host work and
the device work; the kernels in front of the encoder are also timed with events.  Out: generation._to_uint8_device's torch expression
against icd_image_to_u8 on an [n, 3, 512, 512] fp16 sample, events, after a warm-up.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def wall(fn, reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def events(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from PIL import Image
    from invertible_cd_amd import _lib, generation, ops, synthetic, vae
    n, reps = args.n, args.reps
    m = vae.AutoencoderKL(vae.SD_VAE, synthetic.synthetic_vae_state_dict(vae.SD_VAE, seed=0, device="cuda", dtype=torch.float16), max_chunk=8)
    print(f"# {torch.cuda.get_device_name(0)}, kernel sources {_lib.build_sha()}, n = {n}, median of {reps} after a warm-up")
    print("# the host route and the torch expression are the parent commit's only routes and are unchanged: their figures are the parent's")
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        for H, W in ((512, 512), (768, 1024)):
            paths = []
            for i in range(n):
                paths.append(os.path.join(tmp, f"{H}x{W}_{i}.png"))
                Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(paths[-1])

            def host_prepare(arrs):
                arr = np.concatenate([np.array(i).reshape(1, 512, 512, 3) for i in arrs])
                x = (torch.from_numpy(arr).float() / 127.5 - 1).permute(0, 3, 1, 2)
                return x.to("cuda", dtype=torch.float16)

            host = lambda: m.encode(host_prepare([generation.load_512(p) for p in paths]))["latent_dist"].mean
            dev = lambda: m.encode_images([generation.load_512(p, device="cuda") for p in paths], 512)["latent_dist"].mean
            assert torch.equal(host(), dev())
            decode = wall(lambda: [np.array(Image.open(p).convert("RGB")) for p in paths], reps)
            raw = [np.array(Image.open(p).convert("RGB")) for p in paths]
            h_rest = wall(lambda: host_prepare([np.array(Image.fromarray(r).resize((512, 512))) for r in raw]), reps)
            d_rest = wall(lambda: ops.vae_ingest(torch.stack([torch.from_numpy(r).to("cuda") for r in raw]), 512), reps)
            x = host_prepare([generation.load_512(p) for p in paths]).contiguous()
            u8 = torch.stack([torch.from_numpy(r).to("cuda") for r in raw])
            enc = events(lambda: m.encode(x), reps)
            print(f"{n} files of {W} x {H} -> latent:")
            print(f"  host route   {wall(host, reps):8.2f} ms wall   (file decode {decode:.2f}; PIL resize, / 127.5 - 1, fp32 -> fp16 upload {h_rest:.2f})")
            print(f"  device route {wall(dev, reps):8.2f} ms wall   (file decode {decode:.2f}; byte upload + icd_vae_ingest {d_rest:.2f})")
            print(f"  events: icd_pack_nchw {events(lambda: ops.pack_nchw(x), reps):.3f} ms | icd_vae_ingest (2 launches) "
                  f"{events(lambda: ops.vae_ingest(u8, 512), reps):.3f} ms | the encoder itself {enc:.2f} ms")
    s = (torch.randn(n, 3, 512, 512, generator=torch.Generator().manual_seed(1)) * 0.7).half().cuda()

    def chain():
        image = (s / 2 + 0.5).clamp(0, 1)
        return (image.permute(0, 2, 3, 1) * 255).to(torch.uint8).contiguous()

    assert torch.equal(chain(), ops.image_to_u8(s))
    print(f"[{n}, 3, 512, 512] fp16 sample -> uint8 NHWC: torch expression {events(chain, reps) * 1e3:.1f} us | icd_image_to_u8 "
          f"{events(lambda: ops.image_to_u8(s), reps) * 1e3:.1f} us (events)")


if __name__ == "__main__":
    main()
