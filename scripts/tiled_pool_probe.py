"""Pooled tiles of many pictures, measured (the record is profiles/tiled_pool.txt).

24 synthetic uint8 pictures in [H][W][C] host memory, Kodak's mix of 512 x 768 and 768 x 512 (18 and 6), the hyperprior codec with
seeded weights, tiles of 256: every picture is six full tiles, 144 in all.
  1. The yardstick: the loop of compress_tiled + decompress_tiled(output_dtype=uint8) over the pictures, one picture per call -- the
     path as it was before pooled calls existed, which they leave unchanged.  Against it compress_tiled_items +
     decompress_tiled_items over all 24 at max_batch 24 and 144.  Every route is warmed once, then timed in alternating rounds
     (loop, 24, 144, loop, ...), a host clock around work that ends in a device synchronise; the pooled routes' containers and
     pictures are compared with the loop's before anything is timed.
  2. The two new launches alone, pictures and reconstructions resident on the device: image_tiles_gather of the 144 tiles against the
     24 image_tiles_to_f32 launches it replaces, image_tiles_scatter against the 24 image_tiles_from_f32 launches; each a host clock
     around `--reps` repetitions that end in a device synchronise (the pooled entries stage their table and wait for that copy, so
     device events alone would leave part of their cost out).
Three rounds each; the spread is stated beside every median.

    python scripts/tiled_pool_probe.py [--pictures 24 --tile 256 --rounds 3 --reps 200] [--commit TEXT] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts, scale=1e3):
    m = statistics.median(ts)
    return f"{m * scale:9.2f} ({min(ts) * scale:.2f} .. {max(ts) * scale:.2f}; spread {(max(ts) - min(ts)) / m:.3f} of the median)"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=24)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--commit", default="not stated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing here is measured on a CPU")
    from cbench_basic_amd import presets
    from cbench_basic_amd.nn import kernels as K
    from cbench_basic_amd.utils.tiling import TileGrid, pool_tiles
    from scripts.tiled_probe import picture

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    T, N = args.tile, args.pictures
    codec = presets.seed_synthetic_weights(presets.hyperprior_codec(), seed=0).eval().cuda()
    codec.update_state()
    sizes = [(768, 512) if k % 4 == 3 else (512, 768) for k in range(N)]
    pictures = []
    for k, (H, W) in enumerate(sizes):      # one seeded picture per shape, rolled so that no two pictures are equal
        rolled = torch.roll(picture(H, W), shifts=(7 * k, 13 * k), dims=(2, 3))
        pictures.append(rolled.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    assert all(K.image_layout_of(p) == "hwc" and not p.is_cuda for p in pictures)
    grids = [TileGrid(H, W, T, T) for H, W in sizes]
    tiles = sum(len(g) for g in grids)
    mpix = sum(H * W for H, W in sizes) / 1e6
    say(f"commit: {args.commit}")
    say(f"{N} pictures, uint8 [H][W][C] host memory, {sum(1 for s in sizes if s == (512, 768))} of 512 x 768 and {sum(1 for s in sizes if s == (768, 512))} of "
        f"768 x 512, {mpix:.1f} Mpix; hyperprior codec, seeded weights; tiles of {T} x {T}: {tiles} tiles in {len(pool_tiles(grids))} size(s); "
        f"{torch.cuda.get_device_name(0)}")

    calls = {}

    def loop():
        out, n = [], 0
        for p in pictures:
            data = codec.compress_tiled(p, tile=T)
            n += codec.last_items_calls
            out.append((data, codec.decompress_tiled(data, output_dtype=torch.uint8)))
            n += codec.last_items_calls
        calls["loop"] = n
        return out

    def pooled(max_batch):
        def run():
            data = codec.compress_tiled_items(pictures, tile=T, max_batch=max_batch)
            n = codec.last_items_calls
            back = codec.decompress_tiled_items(data, output_dtype=torch.uint8, max_batch=max_batch)
            calls[max_batch] = n + codec.last_items_calls
            return list(zip(data, back))
        return run

    routes = [("loop", loop), (24, pooled(24)), (144, pooled(144))]
    want = timed(loop)[1]
    for name, fn in routes[1:]:              # warm, and the same bytes and pictures as the loop
        got = timed(fn)[1]
        assert [d for d, _ in got] == [d for d, _ in want], name
        assert all(torch.equal(a, b) for (_, a), (_, b) in zip(got, want)), name
    del got
    times = {name: [] for name, _ in routes}
    for _ in range(args.rounds):
        for name, fn in routes:
            times[name].append(timed(fn)[0])
    say()
    say(f"1. compress + decompress of the {N} pictures, ms for all of them, median (min .. max) over {args.rounds} alternating rounds; outputs equal")
    say(f"   loop of compress_tiled + decompress_tiled, {calls['loop']:3d} calls   {fmt(times['loop'])}")
    for mb in (24, 144):
        say(f"   pooled, max_batch {mb:3d},                    {calls[mb]:3d} calls   {fmt(times[mb])}")
    base = statistics.median(times["loop"])
    spread = (max(times["loop"]) - min(times["loop"])) / base
    for mb in (24, 144):
        m = statistics.median(times[mb])
        say(f"   max_batch {mb}: {base / m:.2f}x the loop ({mpix / m:.1f} against {mpix / base:.1f} Mpix/s); the loop's own spread is {spread:.3f} of its median")

    say()
    say(f"2. the launches alone, {tiles} tiles, device-resident; microseconds for all tiles, host clock over {args.reps} repetitions, median over {args.rounds} rounds")
    dev = [p.cuda() for p in pictures]
    chunk = pool_tiles(grids)[0]
    assert len(chunk.tiles) == tiles
    groups = [g.groups()[0] for g in grids]
    assert all(len(g.groups()) == 1 for g in grids)      # full tiles only: a picture's tiles are one group, and one slice of the pooled batch
    starts = [sum(len(g) for g in grids[:k]) for k in range(N)]
    batch = K.image_tiles_gather(dev, chunk.tiles, T, T)
    path_in = K.image_tiles_last_path()
    singles = [K.image_tiles_to_f32(p, g) for p, g in zip(dev, groups)]
    assert torch.equal(batch, torch.cat(singles))
    canv_a = [torch.zeros_like(p) for p in dev]
    canv_b = [torch.zeros_like(p) for p in dev]
    K.image_tiles_scatter(batch, canv_a, chunk.tiles, T, T)
    path_out = K.image_tiles_last_path()
    for rec, c, g in zip(singles, canv_b, groups):
        K.image_tiles_from_f32(rec, c, g)
    assert all(torch.equal(a, b) and torch.equal(a, p) for a, b, p in zip(canv_a, canv_b, dev))
    del singles
    work = {
        "gather, one launch": lambda: K.image_tiles_gather(dev, chunk.tiles, T, T),
        f"cut, {N} launches": lambda: [K.image_tiles_to_f32(p, g) for p, g in zip(dev, groups)],
        "scatter, one launch": lambda: K.image_tiles_scatter(batch, canv_a, chunk.tiles, T, T),
        f"paste, {N} launches": lambda: [K.image_tiles_from_f32(batch[s:s + len(g.indices)], c, g) for s, c, g in zip(starts, canv_b, groups)],
    }
    micro = {name: [] for name in work}
    for _ in range(args.rounds):
        for name, fn in work.items():
            def window(fn=fn):
                for _ in range(args.reps):      # results are dropped at once: the allocator hands the same block out again
                    fn()
            micro[name].append(timed(window)[0] / args.reps)
    moved = 5 * 3 * T * T * tiles      # one byte and one float per sample
    for name in work:
        m = statistics.median(micro[name])
        say(f"   {name:22s} {fmt(micro[name], 1e6)}   {moved / m / 1e9:7.0f} GB/s of {moved / 1e6:.0f} MB")
    say(f"   paths: gather {path_in}, scatter {path_out} (1 = wide)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
