#!/usr/bin/env python3
"""What the 8-bit image path is worth on one MI355X (profiles/u8_path.txt): float32 against uint8 on both legs of the hyperprior codec.

  python scripts/u8_path_probe.py                      # every leg, written to profiles/u8_path.txt
  python scripts/u8_path_probe.py --float-only         # the float legs alone: what a tree without the uint8 path can run

A  compress() of a HOST batch of 256 x 3 x 256 x 256 on the fused session: float32 pageable / pinned (201 MB uploaded),
   uint8 pageable / pinned (50 MB uploaded, converted on the device), uint8 pinned over [B][H][W][C] memory.
B  decompress() of that batch's string: into a float32 device tensor (today's result); today's way to a host picture (torch ops
   on the float result, then .cpu()); output_dtype=uint8 on the device; uint8 straight into a pinned host tensor.
C  the harness on 24 Kodak-shaped items (3 x 512 x 768) at batch 1, stream_lanes 1 and 64, float32 items against uint8 items
   (time_compress / time_decompress per item, Mpix/s over the dataset's wall time).

Every leg is timed in three rounds, the legs of a section alternating inside a round; a round's figure is the median of its
repetitions, a line gives the median of the three rounds and their spread (min .. max)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 3


def build(lanes=1):
    from cbench_basic_amd import presets
    torch.manual_seed(0)
    codec = presets.hyperprior_codec(**(dict(stream_lanes=lanes) if lanes != 1 else {}))
    codec = presets.seed_synthetic_weights(codec, seed=0).eval().to("cuda")
    codec.update_state()
    return codec


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def alternate(legs, reps, emit, unit="ms"):
    """legs: [(name, fn)].  One warm-up call each, then ROUNDS rounds over all legs in turn."""
    for _, fn in legs:
        fn()
    rounds = {name: [] for name, _ in legs}
    for _ in range(ROUNDS):
        for name, fn in legs:
            rounds[name].append(timed(fn, reps))
    for name, _ in legs:
        r = rounds[name]
        emit(f"{name:58s} {statistics.median(r):9.3f} {unit}   ({min(r):.3f} .. {max(r):.3f})   rounds " + " ".join(f"{v:.3f}" for v in r))
    return {name: statistics.median(r) for name, r in rounds.items()}


def section_batch(args, emit):
    codec = build()
    B, H, W = args.batch, args.size, args.size
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g)
    f32 = u8.float().div(255)
    emit(f"# A  compress() of a host batch {B} x 3 x {H} x {W} (float32 {f32.numel() * 4 / 1e6:.0f} MB, uint8 {u8.numel() / 1e6:.0f} MB), fused session, "
         f"{args.reps} repetitions per round")
    data = codec.compress(f32)
    legs = [("compress float32 pageable", lambda x=f32: codec.compress(x)), ("compress float32 pinned", lambda x=f32.pin_memory(): codec.compress(x))]
    if not args.float_only:
        hwc = u8.permute(0, 2, 3, 1).contiguous().pin_memory().permute(0, 3, 1, 2)
        assert codec.compress(u8) == data and codec.compress(hwc) == data
        legs += [("compress uint8 pageable", lambda x=u8: codec.compress(x)), ("compress uint8 pinned", lambda x=u8.pin_memory(): codec.compress(x)),
                 ("compress uint8 pinned, [B][H][W][C] memory", lambda x=hwc: codec.compress(x))]
    alternate(legs, args.reps, emit)
    emit(f"# B  decompress() of that batch's string ({len(data)} bytes), {args.reps} repetitions per round")

    def torch_route():
        return codec.decompress(data).clamp_(0, 1).mul_(255).round_().to(torch.uint8).cpu()
    legs = [("decompress -> float32 on the device", lambda: codec.decompress(data)),
            ("decompress -> float32, torch clamp/mul/round/byte, .cpu()", torch_route)]
    if not args.float_only:
        sess = codec.entropy_coder._fused_session({}, None)
        pinned = torch.empty((B, 3, H, W), dtype=torch.uint8).pin_memory()
        assert torch.equal(sess.decode(data, output_dtype=torch.uint8, out=pinned), torch_route())
        legs += [("decompress(output_dtype=uint8) -> uint8 on the device", lambda: codec.decompress(data, output_dtype=torch.uint8)),
                 ("decompress(output_dtype=uint8).cpu() (pageable)", lambda: codec.decompress(data, output_dtype=torch.uint8).cpu()),
                 ("session decode -> uint8 in a pinned host tensor", lambda: sess.decode(data, output_dtype=torch.uint8, out=pinned))]
    alternate(legs, args.reps, emit)


def section_harness(args, emit):
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark
    from cbench_basic_amd.data import RandomImageDataset, batched
    H, W, N = 512, 768, args.items
    emit(f"# C  harness, {N} items 3 x {H} x {W}, batch 1, one stream; per line: median of {ROUNDS} alternating passes (min .. max)")
    g = torch.Generator().manual_seed(2)
    u8_items = [torch.randint(0, 256, (1, 3, H, W), dtype=torch.uint8, generator=g) for _ in range(N)]
    kinds = [("float32", [x.float().div(255) for x in u8_items])]
    if not args.float_only:
        kinds.append(("uint8", u8_items))
        kinds.append(("uint8 hwc", [x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for x in u8_items]))
    with tempfile.TemporaryDirectory() as tmp:
        for K in args.lanes:
            codec = build(K)
            res = {name: [] for name, _ in kinds}
            for rnd in range(ROUNDS + 1):                      # pass 0 warms up
                for name, items in kinds:
                    codec.decompress(codec.compress(items[0]))
                    torch.cuda.synchronize()
                    bench = BasicLosslessCompressionBenchmark(codec, items, distortion_metric=None, output_dir=os.path.join(tmp, f"{K}_{name}_{rnd}"))
                    m = bench.run_benchmark(ignore_exist_metrics=True)
                    bench.close()
                    if rnd:
                        pick = lambda end: next(v for k, v in m.items() if k.endswith(end))
                        res[name].append((pick("time_compress"), pick("time_decompress"), N * H * W / 1e6 / (pick("time_wall_dataset") / 1e3),
                                          pick("compressed_length")))
            for name, _ in kinds:
                cols = list(zip(*res[name]))
                fmt = lambda v: f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"
                emit(f"stream_lanes {K:3d}  {name:10s} compress_ms {fmt(cols[0])}  decompress_ms {fmt(cols[1])}  Mpix/s {fmt(cols[2])}  bytes/item {cols[3][0]:.1f}")
            del codec
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--float-only", action="store_true", help="the float legs alone (a tree without the uint8 path)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--items", type=int, default=24)
    ap.add_argument("--lanes", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "u8_path.txt"))
    args = ap.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit(f"## {args.label}{' (float legs only)' if args.float_only else ''}")
    section_batch(args, emit)
    section_harness(args, emit)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
