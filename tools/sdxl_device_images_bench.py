#!/usr/bin/env python3
"""SDXL images in and out: the host route against the device route at B = 8, 1024 x 1024 (informational, no pass criterion).

    python tools/sdxl_device_images_bench.py [--n 8] [--size 1024] [--reps 20] [--warmup 3]

In: n images of size x size (seeded noise) -> the first operand of the fp32-fidelity encoder, split3 fp16 [n * size^2, 24].  Host route:
_ImageProcessor.preprocess of the PIL images, the cast to fp16 and upload, the upcast, vae._pack32 (prepare_latents in front of
the encoder).  Device route: the uint8 batch already on the device -> icd_vae_ingest_f32 and the zero fill of the lo half that an fp16
pipeline asks for (encode_images(rule='image_processor', image_dtype=float16)); also shown with the upload of the bytes in front.
Out: a decoded fp32 sample [n, 3, size, size] on the device -> _ImageProcessor.postprocess(..., 'pil') (copy to the host, numpy, PIL)
against 'uint8_device' (icd_image_to_u8_round).  The encoder and the decoder between the two ends are the same launches on both routes and
are not run.  Wall time around a synchronise: the median (and the fastest) of --reps timed repetitions after --warmup untimed ones.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return f"{statistics.median(ts):9.3f} ms median, {min(ts):9.3f} ms fastest"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from PIL import Image
    from invertible_cd_amd import _lib, ops, vae
    from invertible_cd_amd.pipelines import _ImageProcessor
    n, S, reps, warmup = args.n, args.size, args.reps, args.warmup
    ip = _ImageProcessor()
    print(f"# {torch.cuda.get_device_name(0)}, kernel sources {_lib.build_sha()}, n = {n}, {S} x {S}, {reps} timed repetitions after "
          f"{warmup} warm-up repetitions, wall time around a synchronise")
    arr = np.random.default_rng(0).integers(0, 256, (n, S, S, 3), dtype=np.uint8)
    pils = [Image.fromarray(a) for a in arr]
    host_u8 = torch.from_numpy(arr)
    dev_u8 = host_u8.cuda()

    def host_in():
        x = ip.preprocess(pils).to(device="cuda", dtype=torch.float16)
        return vae._pack32(x.float(), torch.device("cuda"))

    def dev_in(u8=dev_u8):
        a, _ = ops.vae_ingest_f32(u8, S)
        a[:, 8:16].zero_()
        return a

    assert torch.equal(host_in().view(torch.int16), dev_in().view(torch.int16))
    print(f"ingest, {n} images -> split3 operand of conv_in:")
    print(f"  host route   (preprocess, fp16 upload, upcast, _pack32)          {wall(host_in, reps, warmup)}")
    print(f"  device route (icd_vae_ingest_f32, lo half zeroed)                {wall(dev_in, reps, warmup)}")
    print(f"  device route with the upload of the uint8 batch in front         {wall(lambda: dev_in(host_u8.cuda()), reps, warmup)}")
    sample = (torch.randn(n, 3, S, S, generator=torch.Generator().manual_seed(1)) * 0.7).cuda()
    host_out = lambda: ip.postprocess(sample, output_type="pil")
    dev_out = lambda: ip.postprocess(sample, output_type="uint8_device")
    assert np.array_equal(np.stack([np.array(i) for i in host_out()]), dev_out().cpu().numpy())
    print(f"output, decoded fp32 sample [{n}, 3, {S}, {S}] -> images:")
    print(f"  host route   (postprocess 'pil': copy to the host, numpy, PIL)   {wall(host_out, reps, warmup)}")
    print(f"  device route (postprocess 'uint8_device': icd_image_to_u8_round) {wall(dev_out, reps, warmup)}")


if __name__ == "__main__":
    main()
