"""FID feature extraction at full width: images/s of FidInception.features for one batch size, timed with HIP events, and the share of
that time spent in icd_conv2d (every convolution of the batch timed on its own in a second pass).  Report only.

    python tools/fid_bench.py [--batch 40] [--size 512] [--iters 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from invertible_cd_amd import inception, ops, synthetic  # noqa: E402


def _timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=40)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    cfg = inception.FID_INCEPTION
    model = inception.FidInception(cfg, synthetic.synthetic_inception_state(cfg, seed=0), "cuda")
    images = torch.randint(0, 256, (a.batch, a.size, a.size, 3), dtype=torch.uint8, device="cuda")
    model.features(images)                                       # warm-up: tables, allocator
    total = _timed(lambda: model.features(images), a.iters)
    conv_ms, calls, real = 0.0, [], ops.conv2d

    def record(*args, **kw):
        calls.append((args, kw))
        return real(*args, **kw)
    ops.conv2d = record
    model.features(images)
    ops.conv2d = real
    for args, kw in calls:
        conv_ms += _timed(lambda: real(*args, **kw), a.iters)
    print(f"fid_bench: {torch.cuda.get_device_name(0)}, batch {a.batch}, {a.size} x {a.size} uint8 on the device, full width")
    print(f"  features: {total:.2f} ms per batch = {a.batch / total * 1e3:.0f} images/s")
    print(f"  icd_conv2d: {len(calls)} launches, {conv_ms:.2f} ms when timed one by one = {100 * conv_ms / total:.0f} % of the batch")


if __name__ == "__main__":
    main()
