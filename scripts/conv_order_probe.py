#!/usr/bin/env python3
"""HIP-event timing of the whole-cout launches of plain-activation layers whose staging follows the 32-channel slices'
(profiles/conv_order.txt): forced with BASIC_CONV_DEBUG=8, 200 launches after 4 warm-up."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbench_basic_amd.nn import kernels as K

os.environ["BASIC_CONV_DEBUG"] = "8"
# name, cin, cout, transposed, activation, input batch x height x width (5 x 5, stride 2 throughout)
LAYERS = [
    ("ha5_128: conv 128->128 relu, 16 x 128 x 128 x 128 (512 blocks: whole anyway)", 128, 128, False, K.ACT_RELU, 16, 128, 128),
    ("h_a.2 of 96 tiles of 512 x 512: conv 128->128 relu, 96 x 128 x 32 x 32 (forced)", 128, 128, False, K.ACT_RELU, 96, 32, 32),
    ("mean-scale h_s.1: deconv 192->192 leaky, 256 x 192 x 8 x 12 (forced)", 192, 192, True, K.ACT_LEAKY_RELU, 256, 8, 12),
    ("mean-scale h_s.2: deconv 192->288 leaky, 256 x 192 x 16 x 24 (whole anyway)", 192, 288, True, K.ACT_LEAKY_RELU, 256, 16, 24),
]
REPS = 200
for name, cin, cout, tr, act, B, H, W in LAYERS:
    g = torch.Generator().manual_seed(0)
    w = torch.randn((cin, cout, 5, 5) if tr else (cout, cin, 5, 5), generator=g) * 0.02
    plan = K.ConvPlan(w, torch.randn(cout, generator=g), 2, 2, 1 if tr else 0, tr, act, None, None)
    x = torch.randn(B, cin, H, W, generator=g).cuda()
    y = plan(x)
    for _ in range(3):
        plan(x, out=y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        plan(x, out=y)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / REPS
    print(f"{name:84s} {ms:8.4f} ms {plan.flops(B, H, W) / ms / 1e9:6.1f} TFLOP/s, {plan.launches(B, H, W)} launch(es)")
