#!/usr/bin/env python3
"""MS-SSIM on the GPU: the fused HIP evaluation (csrc/msssim.hip) beside the torch-op path (``impl="torch"``, what every call
took before the kernel) on the same build, at one Kodak-shaped item and at the harness's 24-image dataset.

Per shape and path: the median and the spread of ``--repeats`` single calls timed with device events after ``--warmup`` calls, and
the device kernels one call launches, counted by torch's profiler (the kernel path's count is also fixed by its source: 5 scale
launches, 4 poolings, 1 finish).  Also the algorithmic HBM traffic of the fused evaluation and the rate the median time amounts
to.  A script, not a test:

  python scripts/msssim_bench.py [--repeats 50] [--warmup 10]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1, 3, 512, 768), (24, 3, 512, 768)]


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


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower()]
    if not kernels:
        raise RuntimeError("the profiler recorded no device kernel")
    return len(kernels)


def traffic_bytes(B, C, H, W):
    """x and y read once per scale with the 10-sample halo of a 32 x 32 tile left to the caches, pooled levels written once."""
    total, h, w = 0, H, W
    for s in range(5):
        total += 2 * 4 * B * C * h * w                 # read both images of this level (scale pass)
        if s < 4:
            total += 2 * 4 * B * C * h * w             # read them again (pooling pass)
            h, w = h // 2 + h % 2, w // 2 + w % 2
            total += 2 * 4 * B * C * h * w             # write the next level
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing here can be timed on a CPU")
    from cbench_basic_amd.benchmark.ms_ssim import ms_ssim
    print(f"device: {torch.cuda.get_device_name(0)}; warmup {args.warmup}, repeats {args.repeats}, one call per timing, device events")
    for shape in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.rand(shape, generator=g)
        y = (x + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
        x, y = x.cuda(), y.cuda()
        paths = {"hip": lambda: ms_ssim(y, x, size_average=False), "torch": lambda: ms_ssim(y, x, size_average=False, impl="torch")}
        diff = float((paths["hip"]() - paths["torch"]()).abs().max())
        # alternate the two paths so that both see the same state of the machine
        rounds = 5
        times = {k: [] for k in paths}
        for r in range(rounds):
            for k, fn in paths.items():
                times[k] += time_calls(fn, args.warmup if r == 0 else 2, max(1, args.repeats // rounds))
        print(f"shape {shape}: max |hip - torch| per image {diff:.2e}")
        for k, fn in paths.items():
            t = sorted(times[k])
            n = count_kernels(fn)
            print(f"  {k:5s}: median {statistics.median(t) * 1e3:9.1f} us  min {t[0] * 1e3:9.1f}  p90 {t[int(0.9 * (len(t) - 1))] * 1e3:9.1f}"
                  f"  ({len(t)} calls)   device kernels per call: {n}")
        med = {k: statistics.median(v) for k, v in times.items()}
        nbytes = traffic_bytes(*shape)
        print(f"  torch / hip: {med['torch'] / med['hip']:.1f}x;  algorithmic traffic of the fused path {nbytes / 1e6:.1f} MB "
              f"= {nbytes / (med['hip'] * 1e-3) / 1e12:.2f} TB/s at the median (workspace allocation and launches included)")


if __name__ == "__main__":
    main()
