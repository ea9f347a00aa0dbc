#!/usr/bin/env python3
"""Stand-alone times of the synthesis transform's split-fp16 layers: g_s layers 1-3 of the hyperprior codec at batch 256
(both fused row-phase launches of each), HIP events around warmed-up repetitions.

Each mode sets the library's switches for the whole layer: `default`, `direct` (BASIC_CONV_DEBUG=1024: split-fp16
activations by direct loads, no LDS patch) and `f32` (BASIC_CONV_F32=1: the fp32 kernel).  When `default` and `direct` both
run, the script prints whether their outputs are equal bit for bit.

    python3 scripts/micro/gs_split_layers.py [--modes default,direct,f32] [--reps 20] [--batch 256] [--root TREE]

--root times the package of another checkout of this repository (e.g. the parent commit's, built in place).
"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="default,direct")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from cbench_basic_amd.nn import kernels as K  # noqa: E402

LAYERS = [("g_s.1 192->128 @16", 192, 16), ("g_s.2 128->128 @32", 128, 32), ("g_s.3 128->128 @64", 128, 64)]
MODES = {"default": {}, "direct": {"BASIC_CONV_DEBUG": "1024"}, "f32": {"BASIC_CONV_F32": "1"}}


def set_mode(mode):
    for k in ("BASIC_CONV_DEBUG", "BASIC_CONV_F32"):
        os.environ.pop(k, None)
    os.environ.update(MODES[mode])


print(f"# {K.__file__}  batch {args.batch}  reps {args.reps}", flush=True)
total = {}
for name, cin, hw in LAYERS:
    g = torch.Generator().manual_seed(0)
    w = torch.randn(cin, 128, 5, 5, generator=g) * (1.0 / (cin * 25) ** 0.5)
    b = torch.randn(128, generator=g) * 0.1
    gamma = torch.rand(128, 128, generator=g) * 0.02 + 0.1 * torch.eye(128)
    beta = torch.rand(128, generator=g) + 0.5
    plan = K.ConvPlan(w, b, 2, 2, 1, True, K.ACT_IGDN, gamma, beta)
    x = torch.randn(args.batch, cin, hw, hw, generator=g).cuda()
    outs = {}
    for mode in args.modes.split(","):
        set_mode(mode)
        y = plan(x)
        for _ in range(3):
            plan(x, out=y)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            plan(x, out=y)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        total[mode] = total.get(mode, 0.0) + ms
        if mode in ("default", "direct"):
            outs[mode] = y.clone()
        print(f"{name:20s} {mode:8s} {ms:8.3f} ms", flush=True)
    if len(outs) == 2:
        print(f"{name:20s} default == direct: {torch.equal(outs['default'], outs['direct'])}", flush=True)
    del x, y, outs
    torch.cuda.empty_cache()
for mode, ms in total.items():
    print(f"{'three layers':20s} {mode:8s} {ms:8.3f} ms", flush=True)
set_mode("default")
