"""What skip coding costs and saves (INTEGRATION.md "Skip coding"; output: profiles/skip.txt).  A record, not a test.

For the bench shape (256 x 3 x 256 x 256) and a Kodak-shaped batch-1 call (1 x 3 x 512 x 768), with 1 and 8 stream lanes, at skip_rows in
{0, 8, 12, 16, 20}, the scale hyperprior codec with the seeded synthetic weights:

  * the share of y that is skipped (from the device's own indexes) and the container's bytes;
  * the y coder's rANS launches alone, encode and decode, on the compacted arrays (device events);
  * the compaction's and the expansion's three launches each (device events);
  * compress_skip + decompress_skip through the fused session (host clock around calls that end in a device synchronise);
  * PSNR of the reconstruction.

One process, one stream, every route warmed, alternating rounds, medians with the spread stated.  The baseline of every call time is
compress + decompress of the PARENT commit at the same shape: run this script in a checkout of the parent with --baseline-out FILE
(it then times compress / decompress alone and needs nothing of skip coding), and here with --baseline FILE.

    python scripts/skip_probe.py --baseline parent.json [--rounds 5] [--reps 3] > profiles/skip.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("bench", (256, 3, 256, 256)), ("kodak", (1, 3, 512, 768))]
LANES = [1, 8]
ROWS = [0, 8, 12, 16, 20]


def _spread(t):
    return (max(t) - min(t)) / statistics.median(t)


def _fmt(t):
    return f"{statistics.median(t):9.3f} ({_spread(t):.3f})"


def _pictures(shape):
    imgs = []
    for i in range(shape[0]):
        torch.manual_seed(i)
        imgs.append(torch.rand(*shape[1:]))
    return torch.stack(imgs).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline", default=None, help="JSON written by --baseline-out in a checkout of the parent commit")
    ap.add_argument("--baseline-out", default=None, help="time compress / decompress alone and write them here (works without skip coding)")
    args = ap.parse_args()
    from cbench_basic_amd.nn import kernels as K
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e3

    def device_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.reps

    def rounds(routes, timer):
        for _, fn in routes:   # warm-up
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in routes}
        for _ in range(args.rounds):
            for name, fn in routes:
                times[name].append(timer(fn))
        return times

    plain, out = {}, []
    for sname, shape in SHAPES:
        x = _pictures(shape)
        for lanes in LANES:
            codec = seed_synthetic_weights(hyperprior_codec(stream_lanes=lanes), seed=0).eval().cuda()
            codec.update_state()
            ec = codec.entropy_coder
            assert ec._fused_session({}, None) is not None
            data = codec.compress(x)
            t = rounds([("compress", lambda: codec.compress(x)), ("decompress", lambda: codec.decompress(data))], host_ms)
            plain[f"{sname}/{lanes}"] = dict(compress=t["compress"], decompress=t["decompress"], bytes=len(data))
            if args.baseline_out:
                continue
            # ---- the pieces, on the codec's own latent
            yc = ec.latent_node_entropy_coders["y"]
            with torch.no_grad():
                y = ec.latent_inference_modules["x_y"](x)
                zhat = ec.latent_node_entropy_coders["z"](ec.latent_inference_modules["y_z"](y))
                prior = ec.latent_generative_modules["z_y"](zhat)[..., : y.shape[-2], : y.shape[-1]].contiguous()
            sym, idx, _ = K.gc_quantize_index(y, prior, yc._scale_table_dev, yc.scale_bound, want_yhat=False)
            ns, per = shape[0] * lanes, y[0].numel() // lanes
            rows = []
            for r in ROWS:
                sym_c, idx_c, seg = K.skip_compact(sym, idx, ns, r)
                host_words, off = yc._tables.encode_batch_end(yc._tables.encode_batch_begin(sym_c, idx_c, per, seg=seg))
                d_words = torch.from_numpy(host_words.view("int32").copy()).cuda()
                d_off = torch.from_numpy(off).cuda()
                container = codec.compress_skip(x, r)
                xhat = codec.decompress_skip(container)
                mse = float(((xhat.clamp(0, 1) - x) ** 2).mean())
                pieces = rounds([("enc", lambda: yc._tables.encode_batch(sym_c, idx_c, seg, per + 2)),
                                 ("dec", lambda: yc._tables.decode_batch(d_words, d_off, idx_c, seg)),
                                 ("compact", lambda: K.skip_compact(sym, idx, ns, r)),
                                 ("expand", lambda: K.skip_expand(sym_c, idx, ns, r))], device_ms)
                calls = rounds([("compress_skip", lambda: codec.compress_skip(x, r)),
                                ("decompress_skip", lambda: codec.decompress_skip(container))], host_ms)
                rows.append(dict(r=r, share=float((idx < r).float().mean()), bytes=len(container), psnr=-10 * torch.log10(torch.tensor(mse)).item(),
                                 **pieces, **calls))
            out.append((sname, shape, lanes, rows))
    if args.baseline_out:
        with open(args.baseline_out, "w") as f:
            json.dump(plain, f)
        return
    base = json.load(open(args.baseline)) if args.baseline else None

    print("Skip coding of the scale hyperprior's y latent (scripts/skip_probe.py on one MI355X; see INTEGRATION.md, \"Skip coding\").")
    print(f"{torch.cuda.get_device_name(0)}; median over {args.rounds} alternating rounds of {args.reps} passes, in ms, with the spread")
    print("(max - min) / median in brackets.  rANS enc / dec: the y coder's launches alone on the compacted arrays; compact / expand: the")
    print("three launches of basic_skip_compact_dev / basic_skip_expand_dev (device events).  Calls: compress_skip / decompress_skip through")
    print("the fused session, host clock around calls that end in a device synchronise.  The weights are seeded noise: their sigma does")
    print("not predict y, so the PSNR column says what dropping these symbols does to THIS latent and is meaningless as a quality claim.")
    print("Nothing is gated on these figures.")
    for sname, shape, lanes, rows in out:
        key = f"{sname}/{lanes}"
        print()
        print(f"{sname}: {' x '.join(str(v) for v in shape)}, stream_lanes = {lanes}")
        mine = plain[key]
        both = [a + b for a, b in zip(mine["compress"], mine["decompress"])]
        print(f"   compress + decompress, this tree:            {_fmt(both)}   {mine['bytes']} bytes")
        ref = both
        if base is not None:
            b = base[key]
            ref = [a + c for a, c in zip(b["compress"], b["decompress"])]
            print(f"   compress + decompress, the PARENT commit:    {_fmt(ref)}   {b['bytes']} bytes   (the baseline below)")
            print(f"   this tree / parent: {statistics.median(both) / statistics.median(ref):.3f}")
        print("   rows  skipped     bytes   rANS enc        rANS dec        compact         expand          compress_skip   decompress_skip  "
              "both/baseline  PSNR dB")
        for row in rows:
            call = [a + b for a, b in zip(row["compress_skip"], row["decompress_skip"])]
            print(f"   {row['r']:4d}  {row['share']:7.3f}  {row['bytes']:8d}  {_fmt(row['enc'])} {_fmt(row['dec'])} {_fmt(row['compact'])} "
                  f"{_fmt(row['expand'])} {_fmt(row['compress_skip'])} {_fmt(row['decompress_skip'])}  "
                  f"{statistics.median(call) / statistics.median(ref):8.3f}      {row['psnr']:6.2f}")


if __name__ == "__main__":
    main()
