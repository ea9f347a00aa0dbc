#!/usr/bin/env python3
"""The exact squared error of two 8-bit batches on the GPU: ``image_sse_u8`` (csrc/image.hip) beside the only route the library had
to the same quantity before it -- two ``image_u8_to_f32`` and ``mse_per_image`` -- on one build, in one process, on a 256 x 3 x 256 x
256 pair in each combination of the two layouts.

Per combination the two routes alternate in rounds; every call is timed on its own with device events after a warm-up, and the
median and the spread of all its timings are printed, with the device time of the kernels of one call as torch's profiler sees them
(the event times include the launches; for work this short they are a large part).  Also the bytes each route has to move and the
rate the median amounts to.  The new route's integers are compared with the float route's figure first.  A script, not a test:

  python scripts/u8_metrics_bench.py [--repeats 100] [--warmup 10]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = (256, 3, 256, 256)
ROUNDS = 10


def time_calls(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def device_time(fn):
    """(kernels and memsets of one call, the sum of their device durations in us)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    work = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()]
    if not work:
        raise RuntimeError("the profiler recorded no device work")
    return len(work), sum(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total for e in work)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing here can be timed on a CPU")
    from cbench_basic_amd.benchmark.metrics import psnr_from_sse
    from cbench_basic_amd.nn import kernels as K
    B, C, H, W = SHAPE
    samples = B * C * H * W
    print(f"device: {torch.cuda.get_device_name(0)}; pair {SHAPE} uint8; warmup {args.warmup}, {ROUNDS} alternating rounds, "
          f"{args.repeats} calls per route, one call per timing, device events")
    new_bytes, old_bytes = 2 * samples, 2 * (samples + 4 * samples) + 2 * 4 * samples
    print(f"bytes to move: image_sse_u8 {new_bytes / 1e6:.1f} MB (both batches once); 2 x image_u8_to_f32 + mse_per_image "
          f"{old_bytes / 1e6:.1f} MB (bytes read and floats written, floats read again) = {old_bytes / new_bytes:.1f}x")
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, SHAPE, dtype=torch.uint8, generator=g)
    y = (x.int() + torch.randint(-8, 9, SHAPE, generator=g)).clamp(0, 255).to(torch.uint8)
    for la in ("chw", "hwc"):
        for lb in ("chw", "hwc"):
            a = x.cuda() if la == "chw" else x.cuda().contiguous(memory_format=torch.channels_last)
            b = y.cuda() if lb == "chw" else y.cuda().contiguous(memory_format=torch.channels_last)
            assert K.image_layout_of(a) == la and K.image_layout_of(b) == lb
            routes = {"image_sse_u8": lambda: K.image_sse_u8(a, b),
                      "2 x u8_to_f32 + mse": lambda: K.mse_per_image(K.image_u8_to_f32(a), K.image_u8_to_f32(b))}
            sse = routes["image_sse_u8"]().sum(1).cpu()
            mse = routes["2 x u8_to_f32 + mse"]().double().cpu()
            exact = psnr_from_sse(sse.numpy(), C * H * W)
            gap = float((torch.from_numpy(exact) + 10 * torch.log10(mse)).abs().max())
            times = {k: [] for k in routes}
            for r in range(ROUNDS):     # alternate the two routes so that both see the same state of the machine
                for k, fn in routes.items():
                    times[k] += time_calls(fn, args.warmup if r == 0 else 2, max(1, args.repeats // ROUNDS))
            print(f"a {la}, b {lb}: PSNR of the batch {psnr_from_sse(int(sse.sum()), samples):.6f} dB; "
                  f"max |exact - float| per image {gap:.2e} dB")
            med = {}
            for k, fn in routes.items():
                t = sorted(times[k])
                med[k] = statistics.median(t)
                n, dev = device_time(fn)
                nbytes = new_bytes if k == "image_sse_u8" else old_bytes
                print(f"  {k:20s}: median {med[k] * 1e3:8.1f} us  min {t[0] * 1e3:8.1f}  p90 {t[int(0.9 * (len(t) - 1))] * 1e3:8.1f}  "
                      f"max {t[-1] * 1e3:8.1f}  ({len(t)} calls); device work of one call: {n} kernels / memsets, {dev:8.1f} us "
                      f"= {nbytes / (dev * 1e-6) / 1e12:.2f} TB/s")
            print(f"  parent route / image_sse_u8: {med['2 x u8_to_f32 + mse'] / med['image_sse_u8']:.1f}x at the medians")


if __name__ == "__main__":
    main()
