#!/usr/bin/env python3
"""GPU probe: the scan-line AR y-coder (BaSIC context-model coder, C = 192): per-step launch path vs persistent kernel."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import (GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder,
                                                                        TopoGroupDynamicMaskConv2dContextModel as Ctx)
C = 192
c = Coder(in_channels=C, default_topo_group_method="scanline", topo_group_context_model=Ctx(in_channels=C, out_channels=2 * C))
g = torch.Generator().manual_seed(1)
with torch.no_grad():
    for p in c.parameters():
        p.copy_(torch.randn(p.shape, generator=g) * (0.03 if p.dim() > 1 else 0.02))
c = c.eval().cuda()
c.update_state()


def lanes_probe(lanes_list, shapes, runs, rows=False, decode_schedule="auto"):
    """--lanes K [K ...]: lane streams (stream_lanes = K) against one stream per image.  Per shape and K, `runs` runs of five calls
    each (the median of a run is its figure; min - max over the runs is the spread): GPU time of the persistent decode launch
    (ScanlinePlan.decode, or the whole per-step decode where the planner leaves the call to it), GPU time of the y rANS encode (pack
    + batched encoder), wall time of coder.encode / coder.decode, and the bytes.  K = 1 uses only what the library had before lanes,
    so the same script measures the commit before them.  BASIC_SCAN_PROFILE=1 adds the kernel's per-step split (stderr).
    --rows: the same figures with row streams (stream_rows = True: one stream per latent row and lane; the decode launch is the
    wavefront's where the planner takes it, BASIC_SCAN_KERNEL forces another); without it the script uses nothing the library lacked
    before row streams, so the same --lanes run on the commit before them is the yardstick.
    --decode-schedule raster | wavefront | band (with --rows): the coder's scanline_decode_schedule -- the wavefront or the band decode
    launch instead of the raster kernels; a shape the launch does not fit is reported and skipped.  Left at auto the script sets
    nothing, so --rows on the commit before the schedule measures the raster decode launch the same calls took there."""
    import numpy as np
    from cbench_basic_amd.nn import kernels as K

    def gpu_ms(fn, n=5):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    def wall_ms(fn, n=5):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    spread = lambda v: f"{np.median(v):8.3f} ({min(v):.3f} - {max(v):.3f})"
    for B, H, W in shapes:
        y = (torch.randn(B, C, H, W, generator=g) * 2).cuda()
        prior = torch.stack([torch.randn(B, C, H, W, generator=g), torch.rand(B, C, H, W, generator=g) * 3 + 0.1], 2).reshape(B, 2 * C, H, W).cuda()
        n = H * W * C
        for lanes in lanes_list:
            if hasattr(c, "stream_lanes"):   # (set on every row; a library from before the lanes has no such attribute and runs K = 1 only)
                c.stream_lanes = lanes
            elif lanes != 1:
                raise SystemExit("this library has no lane streams: --lanes 1 only")
            if rows:
                c.stream_rows = True
            if decode_schedule != "auto":
                c.scanline_decode_schedule = decode_schedule
            c.batch_stream_mode = "per_image"   # (K = 1 at batch 1: framed like the lanes, so that the bytes compare)
            R = H if rows else 1   # streams per image and lane
            sym, idx, _, plan = c._run_encode(y, prior)
            data = c.encode(y, prior=prior)
            nstreams = B * R * lanes
            lens = np.frombuffer(data, dtype="<u4", count=nstreams, offset=4).astype(np.int64)
            woff = np.concatenate([[0], np.cumsum(lens // 4)]).astype(np.int64)
            d_words = torch.from_numpy(np.frombuffer(data, dtype=np.int32, count=int(woff[-1]), offset=4 + 4 * nstreams).copy()).cuda()
            d_woff = torch.from_numpy(woff).cuda()
            try:
                sl = c._scanline_plan(plan, prior, B, decode=True, width=W, height=H)
            except Exception as e:   # a forced schedule the call does not fit
                if "does not fit" not in str(e):
                    raise
                print(f"B={B:3d} {H}x{W} K={lanes:2d} rows [{decode_schedule}]: does not fit", flush=True)
                continue
            if sl is None:
                dec, served = (lambda: c._run_decode_impl(d_words, d_woff, prior, B, H, W, True, plan)), "per-step"
            elif rows:
                dec, served = (lambda: sl.decode(c._tables, d_words, d_woff, prior, B, H, W, c._scale_table_dev, lanes=lanes, rows=True)), None
            elif lanes == 1:
                dec, served = (lambda: sl.decode(c._tables, d_words, d_woff, prior, B, H, W, c._scale_table_dev)), None
            else:
                dec, served = (lambda: sl.decode(c._tables, d_words, d_woff, prior, B, H, W, c._scale_table_dev, lanes=lanes)), None
            if rows:
                pack = (lambda: K.lanes_pack(sym, idx, B * H, W, C, lanes)) if lanes > 1 else (lambda: (sym, idx))
                rans = lambda: c._tables.encode_batch_begin(*[t.reshape(-1) for t in pack()], n // lanes // H)
            elif lanes == 1:
                rans = lambda: c._tables.encode_batch_begin(sym.reshape(-1), idx.reshape(-1), n)
            else:
                rans = lambda: c._tables.encode_batch_begin(*[t.reshape(-1) for t in K.lanes_pack(sym, idx, B, H * W, C, lanes)], n // lanes)
            dec(); rans()
            if sl is not None:
                sl.check()
                served = sl.last_kernel()
            out = c.decode(data, prior=prior)
            assert torch.equal(out, c.decode(data, prior=prior))
            r = dict(dec=[], rans=[], enc_wall=[], dec_wall=[])
            for _ in range(runs):
                r["dec"].append(gpu_ms(dec)); r["rans"].append(gpu_ms(rans))
                r["enc_wall"].append(wall_ms(lambda: c.encode(y, prior=prior))); r["dec_wall"].append(wall_ms(lambda: c.decode(data, prior=prior)))
            print(f"B={B:3d} {H}x{W} K={lanes:2d}{' rows' if rows else ''} [{served}]: decode launch {spread(r['dec'])} ms | y rANS encode {spread(r['rans'])} ms | "
                  f"coder.encode {spread(r['enc_wall'])} ms | coder.decode {spread(r['dec_wall'])} ms | {len(data)} bytes ({len(data) / B:.0f} per image)", flush=True)


if "--lanes" in sys.argv or "--rows" in sys.argv:
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[1], help="lane counts to measure (1 = one stream per image)")
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 32, 48, 64, 16, 16], help="B H W [B H W ...]")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", action="store_true", help="row streams (stream_rows = True) at every lane count")
    ap.add_argument("--decode-schedule", choices=("auto", "raster", "wavefront", "band"), default="auto",
                    help="the coder's scanline_decode_schedule (needs --rows)")
    a = ap.parse_args()
    if a.decode_schedule != "auto" and not a.rows:
        ap.error("--decode-schedule needs --rows: only row streams have a decode schedule")
    lanes_probe(a.lanes, [tuple(a.shapes[i: i + 3]) for i in range(0, len(a.shapes), 3)], a.runs, rows=a.rows, decode_schedule=a.decode_schedule)
    sys.exit(0)

shapes = ((1, 32, 48), (8, 16, 16), (64, 16, 16), (24, 32, 48))
if os.environ.get("PROBE_SMALL_BATCHES"):   # where does the per-step path take over?
    shapes = ((2, 32, 48), (3, 32, 48), (4, 32, 48), (6, 32, 48))
for B, H, W in shapes:
    y = (torch.randn(B, C, H, W, generator=g) * 2).cuda()
    prior = torch.stack([torch.randn(B, C, H, W, generator=g), torch.rand(B, C, H, W, generator=g) * 3 + 0.1], 2).reshape(B, 2 * C, H, W).cuda()
    res = {}
    for mode in ((True,) if os.environ.get("PROBE_PERSISTENT_ONLY") else (False, True)):
        c.use_persistent_scanline = mode
        c.persistent_scanline_max_batch = 1024
        for what in ("enc", "dec"):
            if what == "enc":
                fn = lambda: c.encode(y, prior=prior)
            else:
                data = c.encode(y, prior=prior)
                fn = lambda: c.decode(data, prior=prior)
            fn(); fn()
            torch.cuda.synchronize()
            t0 = time.time()
            n = 3
            for _ in range(n):
                out = fn()
            torch.cuda.synchronize()
            res[(mode, what)] = (time.time() - t0) / n * 1e3
    res.setdefault((False, 'enc'), float('nan')); res.setdefault((False, 'dec'), float('nan'))
    print(f"B={B:3d} {H}x{W}: per-step enc {res[(False, 'enc')]:8.2f} ms dec {res[(False, 'dec')]:8.2f} ms | persistent enc {res[(True, 'enc')]:8.2f} ms dec {res[(True, 'dec')]:8.2f} ms"
          f"   ({H * W} steps: {res[(True, 'enc')] / (H * W) * 1e3:.1f} us/step enc)", flush=True)
