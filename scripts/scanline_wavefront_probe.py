#!/usr/bin/env python3
"""GPU probe: the scan-line ENCODE call under the raster schedule (ScanlinePlan.set_encode_schedule("raster"): whatever kernel
the library picks without the wavefront) against the wavefront schedule, BaSIC context-model coder, C = 192, same seeded y and
prior, one process.  Per shape: warm-up, then ROUNDS alternating rounds of N launches each, timed with device events (the call
= memset + prior transpose + the persistent launch); prints per schedule the median and the min .. max of the rounds' means --
the spread the auto rule has to clear -- and checks that both schedules gave the same integers.

    PROBE=1x32x48,2x32x48 ROUNDS=5 N=10 python scripts/scanline_wavefront_probe.py
    BASIC_SCAN_PROFILE=1 PROBE=1x32x48 ROUNDS=1 N=1 python scripts/scanline_wavefront_probe.py     (per-step breakdown on stderr)

Kernel times: run it once under  rocprofv3 --kernel-trace --stats -- python scripts/scanline_wavefront_probe.py ."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import (GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder,  # noqa: E402
                                                                        TopoGroupDynamicMaskConv2dContextModel as Ctx)

C = 192
ROUNDS, N = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("N", "10"))
c = Coder(in_channels=C, default_topo_group_method="scanline", topo_group_context_model=Ctx(in_channels=C, out_channels=2 * C))
g = torch.Generator().manual_seed(1)
with torch.no_grad():
    for p in c.parameters():
        p.copy_(torch.randn(p.shape, generator=g) * (0.03 if p.dim() > 1 else 0.02))
c = c.eval().cuda()
c.update_state()
c._ready()
shapes = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("PROBE", "1x32x48,2x32x48,1x48x32,1x16x16,4x16x16").split(",")]
print(f"scan-line encode call, C = {C}, 5x5 window: {ROUNDS} alternating rounds of {N} launches per schedule, ms per call: median (min .. max of the rounds)")
for B, H, W in shapes:
    y = (torch.randn(B, C, H, W, generator=g) * 2).cuda()
    prior = torch.stack([torch.randn(B, C, H, W, generator=g), torch.rand(B, C, H, W, generator=g) * 3 + 0.1], 2).reshape(B, 2 * C, H, W).cuda()
    sl = c._scanline_plan(c._plan(H, W, None), prior, B, width=W, height=H)
    tab = c._scale_table_dev
    out, kern, times = {}, {}, {"raster": [], "wavefront": []}
    for sched in times:
        sl.set_encode_schedule(sched)
        for _ in range(3):
            out[sched] = sl.encode(y, prior, tab)
        sl.check()
        kern[sched] = sl.last_kernel()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out["raster"], out["wavefront"]))
    for _ in range(ROUNDS):
        for sched in times:
            sl.set_encode_schedule(sched)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(N):
                sl.encode(y, prior, tab)
            ev[1].record()
            torch.cuda.synchronize()
            times[sched].append(ev[0].elapsed_time(ev[1]) / N)
    sl.check()
    sl.set_encode_schedule("auto")
    sl.encode(y, prior, tab)
    sl.check()
    s = 5 // 2 + 2
    steps = {"raster": H * W, "wavefront": W + s * (H - 1)}
    line = f"B={B:2d} {H:2d}x{W:2d}:"
    for sched, t in times.items():
        med = statistics.median(t)
        line += f" {sched} [{kern[sched]}] {steps[sched]:4d} steps {med:7.3f} ({min(t):7.3f} .. {max(t):7.3f}) = {med / steps[sched] * 1e3:6.2f} us/step |"
    r, w = statistics.median(times["raster"]), statistics.median(times["wavefront"])
    print(f"{line} raster / wavefront x{r / w:5.2f} | same integers: {same} | auto takes: {sl.last_kernel()}", flush=True)
