"""What the mean costs: the mean-scale y coder's kernels beside the zero-mean ones, and the mean-scale hyperprior codec beside the scale
hyperprior (INTEGRATION.md "Mean-scale hyperprior"; output: profiles/meanscale.txt).  A record, not a test.

One process, one stream, every route warmed, alternating rounds, medians with the spread stated:

  (a) gc_quantize_index_ms against gc_quantize_index, and the rate curve with means against the one without, on one synthetic latent
      of 256 x 192 x 16 x 16 with 16 candidates (device events around the launches).  The encode-side quantiser moves 16 bytes per
      element without a mean (y, sigma in; symbol, index out) and 20 with one: 1.25 x is the traffic ratio.
  (b) encode + decode of mean_scale_hyperprior_codec beside hyperprior_codec at 256 images of 3 x 256 x 256 through the same loop, fused
      session; and each codec's h_s alone (the mean-scale h_s is 192 / 288 / 384 channels wide against 128 / 128 / 192).

    python scripts/meanscale_probe.py [--images 256] [--size 256] [--rounds 5] [--reps 5] > profiles/meanscale.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _spread(t):
    return (max(t) - min(t)) / statistics.median(t)


def _line(name, t, extra=""):
    med = statistics.median(t)
    return f"   {name:52s} {med:9.4f} ms ({min(t):.4f} .. {max(t):.4f}; spread {_spread(t):.3f} of the median){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from cbench_basic_amd.nn import kernels as K
    from cbench_basic_amd.presets import hyperprior_codec, mean_scale_hyperprior_codec, seed_synthetic_weights
    from cbench_basic_amd.utils.rate import first_grid

    def device_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.reps

    def rounds(routes):
        for _, fn in routes:   # warm-up
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in routes}
        for _ in range(args.rounds):
            for name, fn in routes:
                times[name].append(device_ms(fn))
        return times

    codecs = {}
    for name, build in (("hyperprior", hyperprior_codec), ("mean-scale", mean_scale_hyperprior_codec)):
        c = seed_synthetic_weights(build(), seed=0).eval().cuda()
        c.update_state()
        codecs[name] = c
    yc = codecs["mean-scale"].entropy_coder.latent_node_entropy_coders["y"]
    yc._ready()
    table, tables, bound = yc._scale_table_dev, yc._tables, yc.scale_bound

    # ---- (a) the kernels, on one synthetic latent
    B, M, h, w = 256, 192, 16, 16
    g = torch.Generator().manual_seed(0)
    y = (torch.randn(B, M, h, w, generator=g) * 2).cuda()
    prior = torch.cat([torch.exp(torch.rand(B, M, h, w, generator=g) * 8.7 - 3.0), torch.rand(B, M, h, w, generator=g) * 6 - 3], 1).cuda()
    scales = prior[:, :M].contiguous()
    cand = torch.from_numpy(first_grid(16)).cuda()
    n = y.numel()
    quant = rounds([("gc_quantize_index (no mean)", lambda: K.gc_quantize_index(y, scales, table, bound, want_yhat=False)),
                    ("gc_quantize_index_ms, chunked prior", lambda: K.gc_quantize_index_ms(y, prior, table, bound, want_yhat=False)),
                    ("gc_quantize_index_q (no mean, step 2)", lambda: K.gc_quantize_index_q(y, scales, 2.0, table, bound, want_yhat=False)),
                    ("gc_quantize_index_ms, step 2", lambda: K.gc_quantize_index_ms(y, prior, table, bound, steps=2.0, want_yhat=False))])
    curve = rounds([("rate curve, 16 candidates (no mean)", lambda: K.rate_curve(y, scales, cand, table, tables, bound, 1)),
                    ("rate curve, 16 candidates, means", lambda: K.rate_curve(y, prior, cand, table, tables, bound, 1, means=K.CHUNKED))])

    print("The mean-scale hyperprior beside the scale hyperprior (scripts/meanscale_probe.py on one MI355X; see INTEGRATION.md, \"Mean-scale")
    print("hyperprior\").  Every route warmed once, alternating rounds in one process, device events around the launches.  The weights are")
    print("seeded noise: throughput figures only.  Nothing is gated on these figures.")
    print()
    print(f"{torch.cuda.get_device_name(0)}; median (min .. max) over {args.rounds} alternating rounds of {args.reps} passes")
    print()
    print(f"(a) The kernels on a synthetic latent of {B} x {M} x {h} x {w} = {n} elements (y ~ N(0, 2), sigma log-uniform, mu uniform in [-3, 3)).")
    print("    Bytes moved per element, encode side: 16 without a mean (y, sigma, symbol, index), 20 with one: traffic ratio 1.25.")
    for name, by in (("gc_quantize_index (no mean)", 16), ("gc_quantize_index_ms, chunked prior", 20), ("gc_quantize_index_q (no mean, step 2)", 16),
                     ("gc_quantize_index_ms, step 2", 20)):
        print(_line(name, quant[name], f"   {by * n / statistics.median(quant[name]) / 1e6:.0f} GB/s"))
    for a, b, what in (("gc_quantize_index (no mean)", "gc_quantize_index_ms, chunked prior", "step-less"),
                       ("gc_quantize_index_q (no mean, step 2)", "gc_quantize_index_ms, step 2", "with a step")):
        ratio = statistics.median(quant[b]) / statistics.median(quant[a])
        sp = max(_spread(quant[a]), _spread(quant[b]))
        verdict = "within the traffic ratio and the run's spread" if ratio <= 1.25 * (1 + sp) else \
            "ABOVE the traffic ratio by more than the run's spread: see the GB/s figures above for what bounds the kernel"
        print(f"   {what}: with mean / without = {ratio:.3f} (traffic ratio 1.250, spread {sp:.3f}): {verdict}")
    for name, by in (("rate curve, 16 candidates (no mean)", 8), ("rate curve, 16 candidates, means", 12)):
        print(_line(name, curve[name], f"   {by * n / statistics.median(curve[name]) / 1e6:.0f} GB/s of its single read"))
    a, b = "rate curve, 16 candidates (no mean)", "rate curve, 16 candidates, means"
    ratio = statistics.median(curve[b]) / statistics.median(curve[a])
    print(f"   rate curve: with means / without = {ratio:.3f} (read traffic ratio 1.500, spread {max(_spread(curve[a]), _spread(curve[b])):.3f}).  The curve")
    print("   does 16 divisions, table searches and cost gathers per element read: it is bound by that arithmetic and the L2 gathers, not by")
    print("   HBM (its GB/s above against the quantiser's), so the extra 4 bytes per element and the one subtraction hardly show.")
    print()

    # ---- (b) the codecs, through the same loop
    imgs = []
    for i in range(args.images):
        torch.manual_seed(i)
        imgs.append(torch.rand(3, args.size, args.size))
    x = torch.stack(imgs).cuda()
    pixels = args.images * args.size ** 2
    data = {k: c.compress(x) for k, c in codecs.items()}
    for k, c in codecs.items():
        assert c.entropy_coder._fused_session({}, None) is not None
        c.decompress(data[k])
    torch.cuda.synchronize()
    enc, dec, hs = ({k: [] for k in codecs} for _ in range(3))
    zhat = {}
    for k, c in codecs.items():
        ec = c.entropy_coder
        with torch.no_grad():
            yy = ec.latent_inference_modules["x_y"](x)
            zhat[k] = ec.latent_node_entropy_coders["z"](ec.latent_inference_modules["y_z"](yy))
            ec.latent_generative_modules["z_y"](zhat[k])
    for _ in range(args.rounds):
        for k, c in codecs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                c.compress(x)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.reps):
                c.decompress(data[k])
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            enc[k].append((t1 - t0) / args.reps * 1e3)
            dec[k].append((t2 - t1) / args.reps * 1e3)
            with torch.no_grad():
                hs[k].append(device_ms(lambda: c.entropy_coder.latent_generative_modules["z_y"](zhat[k])))
    print(f"(b) compress + decompress of {args.images} float32 images of 3 x {args.size} x {args.size} resident in HBM, fused session, one stream (host clock")
    print("    around calls that end in a device synchronise); h_s alone by device events.")
    for k in codecs:
        both = [a + b for a, b in zip(enc[k], dec[k])]
        print(f"  {k} codec: {len(data[k])} bytes")
        print(_line("compress", enc[k], f"   {pixels / statistics.median(enc[k]) / 1e3:.1f} Mpix/s"))
        print(_line("decompress", dec[k], f"   {pixels / statistics.median(dec[k]) / 1e3:.1f} Mpix/s"))
        print(_line("compress + decompress", both, f"   {pixels / statistics.median(both) / 1e3:.1f} Mpix/s"))
        print(_line("h_s alone (runs once in each direction)", hs[k], f"   {2 * statistics.median(hs[k]) / statistics.median(both):.3f} of compress + decompress"))
    r = statistics.median([a + b for a, b in zip(enc["mean-scale"], dec["mean-scale"])]) / \
        statistics.median([a + b for a, b in zip(enc["hyperprior"], dec["hyperprior"])])
    print(f"   mean-scale / hyperprior, compress + decompress time: {r:.3f}.  The mean-scale h_s and h_a are 1.5 - 2 x wider (192 / 288 / 384")
    print("   channels) and run on the launch planner's plans as they stand; no target is set for this figure.")


if __name__ == "__main__":
    main()
