#!/usr/bin/env python3
"""Lane streams on Kodak-shaped items through the harness (profiles/lanes_kodak.txt): batch 1, one stream, 24 synthetic 3 x 512 x 768
items (y: 192 x 32 x 48 = 294,912 symbols), the hyperprior codec and the topo-group checkerboard codec, stream_lanes K swept.

  python scripts/lanes_kodak_probe.py                          # K = 1 4 16 64, both codecs, three runs each
  python scripts/lanes_kodak_probe.py --lanes 1 --runs 3       # what a tree without the lane argument can run (K = 1 only)

Per line: Mpix/s over the dataset's wall time, the item's compress / decompress ms (the harness's time_compress / time_decompress:
upload, transforms, entropy stage, framing, download of the bytes), the mean string length in bytes and its difference per extra
stream against K = 1.  One warm-up item before every timed pass (plan building, table upload, graph capture)."""
import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(kind, lanes):
    from cbench_basic_amd import presets
    kw = dict(stream_lanes=lanes) if lanes != 1 else {}     # K = 1 also runs on a tree whose presets have no such argument
    torch.manual_seed(0)   # the constructors draw the biases seed_synthetic_weights leaves alone from the global generator: same codec at every K
    codec = presets.hyperprior_codec(**kw) if kind == "hyperprior" else presets.topogroup_ar_codec(method="checkerboard", **kw)
    codec = presets.seed_synthetic_weights(codec, seed=0).eval().to("cuda")
    codec.update_state()
    return codec


def one_pass(codec, items, out_dir):
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark
    codec.decompress(codec.compress(items[0].to("cuda")))
    torch.cuda.synchronize()
    bench = BasicLosslessCompressionBenchmark(codec, items, distortion_metric=None, output_dir=out_dir)
    m = bench.run_benchmark(ignore_exist_metrics=True)
    bench.close()
    pick = lambda end: next(v for k, v in m.items() if k.endswith(end))
    return dict(wall_ms=pick("time_wall_dataset"), enc_ms=pick("time_compress"), dec_ms=pick("time_decompress"), nbytes=pick("compressed_length"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lanes", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--codecs", nargs="+", choices=["hyperprior", "checkerboard"], default=["hyperprior", "checkerboard"])
    ap.add_argument("--items", type=int, default=24)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    from cbench_basic_amd.data import RandomImageDataset, batched
    items = list(batched(RandomImageDataset(num=args.items, size=(3, args.height, args.width)), 1))
    mpix = args.items * args.height * args.width / 1e6
    print(f"# {args.label or 'lanes_kodak_probe'}: {args.items} items 3 x {args.height} x {args.width}, batch 1, one stream, {args.runs} runs per line", flush=True)
    print("# codec        K  run   Mpix/s  compress_ms  decompress_ms  bytes/item  extra_bytes/extra_stream", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for kind in args.codecs:
            base = None
            for K in args.lanes:
                codec = build(kind, K)
                for run in range(args.runs):
                    r = one_pass(codec, items, os.path.join(tmp, f"{kind}_{K}_{run}"))
                    if K == 1 and base is None:
                        base = r["nbytes"]
                    extra = "-" if K == 1 or base is None else f"{(r['nbytes'] - base) / (K - 1):.2f}"
                    print(f"{kind:12s} {K:3d}  {run:3d}  {mpix / (r['wall_ms'] / 1000):7.2f}  {r['enc_ms']:11.2f}  {r['dec_ms']:13.2f}  {r['nbytes']:10.1f}  {extra}",
                          flush=True)
                del codec
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
