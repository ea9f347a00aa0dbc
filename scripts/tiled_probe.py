"""Tiled coding of one large picture, measured (the record is profiles/tiled_coding.txt).

A synthetic uint8 4096 x 6144 picture in [H][W][C] host memory, the hyperprior codec with seeded weights, tiles of 256 and of 512:
  1. what the whole-picture compress() does at this size;
  2. compress_tiled + decompress_tiled(output_dtype=uint8): one upload, a cut kernel and a paste kernel per chunk;
  3. the same tiles pre-cut into contiguous host items (not timed) through compress_items / decompress_items(output_dtype=uint8),
     chunks of the same size: one copy per item into the batch and a conversion pass each way; nothing is pasted;
  4. one compress / decompress(output_dtype=uint8) per tile.
Every route is warmed once, then timed in three alternating rounds (2, 3, 4, 2, 3, 4, ...), each timing a host clock around work that
ends in a device synchronise; medians and the min..max spread are printed.  The two kernels alone are timed with device events against
the bytes they move (one byte and one float per sample).

    python scripts/tiled_probe.py [--height 4096 --width 6144 --tiles 256 512 --rounds 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def picture(H, W):
    """uint8 [1, 3, H, W] over [H][W][C] host memory: smooth with some noise, made on the GPU from a seed."""
    g = torch.Generator(device="cuda").manual_seed(1)
    yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    base = torch.stack([(yy / H + xx / W) / 2, (torch.sin(yy / 37) * torch.cos(xx / 53) + 1) / 2, (xx * yy) / (H * W)], dim=-1)
    hwc = (base + 0.1 * torch.rand(H, W, 3, device="cuda", generator=g)).clamp(0, 1).mul(255).round().to(torch.uint8)
    return hwc.cpu()[None].permute(0, 3, 1, 2)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=6144)
    ap.add_argument("--tiles", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--call-mpix", type=float, default=8.4, help="pixels per encode() / decode() call, in 2^20 pixels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing here is measured on a CPU")
    from cbench_basic_amd import presets
    from cbench_basic_amd.nn import kernels as K
    from cbench_basic_amd.utils.tiling import TileGrid, unpack_tiled

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    H, W = args.height, args.width
    mpix = H * W / 1e6
    codec = presets.seed_synthetic_weights(presets.hyperprior_codec(), seed=0).eval().cuda()
    codec.update_state()
    img = picture(H, W)
    assert K.image_layout_of(img) == "hwc"
    say(f"picture: uint8 {H} x {W} x 3, [H][W][C] host memory, {mpix:.1f} Mpix; hyperprior codec, seeded weights; {torch.cuda.get_device_name(0)}")

    # 1. the whole picture in one call
    try:
        s = codec.compress(img)
        say(f"1. compress(whole picture): returned {len(s)} bytes")
        del s
    except Exception as e:      # whatever it is, it is the record
        say(f"1. compress(whole picture): {type(e).__name__}: {str(e).splitlines()[0] if str(e) else ''}")
    torch.cuda.synchronize()

    for T in args.tiles:
        grid = TileGrid(H, W, T, T)
        per_call = max(1, int(args.call_mpix * 2 ** 20) // (T * T))
        items = []
        for k in range(len(grid)):
            y, x, h, w = grid.tile_rect(k)
            items.append(img[:, :, y:y + h, x:x + w].contiguous(memory_format=torch.channels_last))
        state = {}

        def tiled():
            state["data"] = codec.compress_tiled(img, tile=(T, T), max_batch=per_call)
            state["calls"] = codec.last_items_calls
            return codec.decompress_tiled(state["data"], output_dtype=torch.uint8, max_batch=per_call)

        def as_items():
            state["strings"] = codec.compress_items(items, max_batch=per_call)
            return codec.decompress_items(state["strings"], max_batch=per_call, output_dtype=torch.uint8)

        def per_tile():
            return [codec.decompress(codec.compress(x), output_dtype=torch.uint8) for x in items]

        routes = [("2. compress_tiled + decompress_tiled", tiled), ("3. compress_items + decompress_items", as_items),
                  ("4. one compress + decompress per tile", per_tile)]
        for _, fn in routes:      # warm every shape the timed window uses
            timed(fn)
        assert unpack_tiled(state["data"])[5] == state["strings"]      # the routes write the same bytes
        times = {name: [] for name, _ in routes}
        for _ in range(args.rounds):
            for name, fn in routes:
                times[name].append(timed(fn)[0])
        say()
        say(f"tiles of {T} x {T}: {grid.rows} x {grid.cols} = {len(grid)} tiles, at most {per_call} per call ({state['calls']} calls each way), "
            f"container {len(state['data'])} bytes = {8 * len(state['data']) / (H * W):.3f} bpp")
        for name, _ in routes:
            t = times[name]
            med = statistics.median(t)
            say(f"  {name:40s} median {med * 1e3:8.1f} ms = {mpix / med:7.1f} Mpix/s   (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f} ms over {len(t)} rounds)")
        a, b = times[routes[0][0]], times[routes[1][0]]
        say(f"  route 2 over route 3, medians: {statistics.median(a) / statistics.median(b):.3f}; "
            f"spread of route 2 {(max(a) - min(a)) / statistics.median(a):.3f}, of route 3 {(max(b) - min(b)) / statistics.median(b):.3f} of the median")

        # the two kernels alone: the whole grid, group by group, from and into a device picture
        dev = img.cuda()
        groups = grid.groups()
        batches = [K.image_tiles_to_f32(dev, g) for g in groups]
        canvas = torch.empty_like(dev)
        for kind, fn in (("cut   (image_tiles_to_f32)", lambda: [K.image_tiles_to_f32(dev, g) for g in groups]),
                         ("paste (image_tiles_from_f32)", lambda: [K.image_tiles_from_f32(b, canvas, g) for b, g in zip(batches, groups)])):
            fn()
            reps = 20
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(reps):
                fn()
            stop.record()
            torch.cuda.synchronize()
            ms = start.elapsed_time(stop) / reps
            moved = H * W * 3 * 5
            say(f"  {kind:30s} {ms:7.3f} ms per picture ({len(groups)} launch(es), path {K.image_tiles_last_path()}), {moved / 1e6:.0f} MB moved: "
                f"{moved / ms / 1e6:.0f} GB/s")
        assert torch.equal(canvas, dev)
        del dev, batches, canvas

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
