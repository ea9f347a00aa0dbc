"""Edge-padded tiles, measured (the record is profiles/tiled_pad.txt).

Padding trades coded area for coding calls; this probe states both sides at two sizes.  The hyperprior codec with seeded weights; the
settings are no padding (the route as it was, whose code padding leaves untouched: the baseline, run in the same process), pad_to=64
and pad_to=tile.
  (a) The picture of profiles/tiled_blend.txt -- synthetic uint8 4096 x 6144 in [H][W][C] host memory --, tiles of 512, overlap 32, at most
      as many tiles per call as scripts/tiled_blend_probe.py takes: compress_tiled + decompress_tiled(output_dtype=uint8).
  (b) 24 uint8 pictures of 24 distinct sizes between 400 and 800, none a multiple of 64, tiles of 256, pooled at max_batch 144:
      compress_tiled_items + decompress_tiled_items.
  (c) The two launches alone on a table with NO edge tile (the 144 full tiles of 24 pictures of 512 x 768), device-resident: the padded
      gather and the clipped scatter against the gather and the scatter they are instantiated from.
Every route is warmed once, then timed in alternating rounds, a host clock around work that ends in a device synchronise; medians of
the rounds with their spread.  A setting whose tiles the codec itself refuses (a host check, e.g. the transforms' LDS budget for a very
narrow edge tile) is reported as refused and left out of the timing.  The weights are seeded noise, and the bytes grow with the padded area: no rate figure here means anything.

    python scripts/tiled_pad_probe.py [--rounds 3 --reps 200] [--commit TEXT] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sizes_b(n=24):
    """n distinct (H, W) between 400 and 800, no side a multiple of 64."""
    out = []
    for k in range(n):
        h, w = 404 + 17 * k, 796 - 15 * k
        h, w = h + (h % 64 == 0), w - (w % 64 == 0)
        out.append((h, w))
    assert len(set(out)) == n and all(400 <= v <= 800 and v % 64 for s in out for v in s)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=6144)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--call-mpix", type=float, default=8.4, help="pixels per encode() / decode() call of (a), in 2^20 pixels")
    ap.add_argument("--commit", default="not stated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing here is measured on a CPU")
    from cbench_basic_amd import presets
    from cbench_basic_amd.nn import kernels as K
    from cbench_basic_amd.utils.tiling import TileGrid, pool_tiles
    from scripts.tiled_pool_probe import fmt, timed
    from scripts.tiled_probe import picture

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    codec = presets.seed_synthetic_weights(presets.hyperprior_codec(), seed=0).eval().cuda()
    codec.update_state()
    say(f"commit: {args.commit}")
    say(f"hyperprior codec, seeded weights; {torch.cuda.get_device_name(0)}; ms, median (min .. max) over {args.rounds} alternating rounds")

    def area(grids):
        return sum(ph * pw for g in grids for ph, pw in (g.coded_size(k) for k in range(len(g)))) / sum(g.H * g.W for g in grids)

    def measure(title, settings, run, grids_of):
        """settings: [(name, pad_to or None)]; run(pad) -> (containers, pictures, calls); grids_of(pad) -> the TileGrids."""
        state, refused = {}, {}
        for name, pad in settings:      # warm every shape the timed windows use
            try:
                state[name] = timed(lambda: run(pad))[1]
            except ValueError as e:     # a tile shape the codec itself refuses (a host check: nothing ran)
                refused[name] = str(e)
        say()
        say(title)
        for name, why in refused.items():
            say(f"   {name:12s} REFUSED by the codec for one of its {len(pool_tiles(grids_of(dict(settings)[name])))} tile sizes: {why}")
        settings = [(name, pad) for name, pad in settings if name in state]
        times = {name: [] for name, _ in settings}
        for _ in range(args.rounds):
            for name, pad in settings:
                times[name].append(timed(lambda: run(pad))[0])
        ref = statistics.median(times[settings[0][0]])
        for name, pad in settings:
            data, _, calls = state[name]
            grids = grids_of(pad)
            m = statistics.median(times[name])
            say(f"   {name:12s} {calls[0]:3d} + {calls[1]:3d} calls, {len(pool_tiles(grids)):2d} tile size(s), coded area {area(grids):.3f} of the pictures, "
                f"containers {sum(len(d) for d in data):9d} bytes ({data[0][:4].decode()})   {fmt(times[name])}   {m / ref:.3f} of {settings[0][0]}")

    # ---- (a)
    H, W, T, O = args.height, args.width, 512, 32
    img = picture(H, W)
    per_call = max(1, int(args.call_mpix * 2 ** 20) // (T * T))

    def run_a(pad):
        kw = {} if pad is None else dict(pad_to=pad)
        data = codec.compress_tiled(img, tile=T, overlap=O, max_batch=per_call, **kw)
        enc = codec.last_items_calls
        back = codec.decompress_tiled(data, output_dtype=torch.uint8, max_batch=per_call)
        return [data], [back], (enc, codec.last_items_calls)
    measure(f"(a) one uint8 {H} x {W} picture, [H][W][C] host memory, tiles of {T}, overlap {O}, at most {per_call} tiles per call: compress_tiled + "
            f"decompress_tiled", [("no padding", None), ("pad_to=64", 64), (f"pad_to={T}", T)], run_a,
            lambda pad: [TileGrid(H, W, T, T, overlap=O, pad_to=pad or 1)])

    # ---- (b)
    T = 256
    sizes = sizes_b()
    pictures = []
    for k, (h, w) in enumerate(sizes):
        p = torch.roll(picture(h, w), shifts=(7 * k, 13 * k), dims=(2, 3))
        pictures.append(p.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))

    def run_b(pad):
        kw = {} if pad is None else dict(pad_to=pad)
        data = codec.compress_tiled_items(pictures, tile=T, max_batch=144, **kw)
        enc = codec.last_items_calls
        back = codec.decompress_tiled_items(data, output_dtype=torch.uint8, max_batch=144)
        return data, back, (enc, codec.last_items_calls)
    measure(f"(b) {len(sizes)} uint8 pictures of {len(set(sizes))} sizes from {sizes[0]} to {sizes[-1]}, {sum(h * w for h, w in sizes) / 1e6:.1f} Mpix, tiles of {T}, "
            f"pooled at max_batch 144: compress_tiled_items + decompress_tiled_items", [("no padding", None), ("pad_to=64", 64), (f"pad_to={T}", T)], run_b,
            lambda pad: [TileGrid(h, w, T, T, pad_to=pad or 1) for h, w in sizes])

    # ---- (c)
    full = [(768, 512) if k % 4 == 3 else (512, 768) for k in range(24)]
    dev = [torch.roll(picture(h, w), shifts=(7 * k, 13 * k), dims=(2, 3)).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).cuda()
           for k, (h, w) in enumerate(full)]
    chunk, = pool_tiles([TileGrid(h, w, T, T) for h, w in full])
    n = len(chunk.tiles)
    batch = K.image_tiles_gather(dev, chunk.tiles, T, T)
    assert torch.equal(batch, K.image_tiles_gather(dev, chunk.tiles, T, T, pad=True))
    paths = [K.image_tiles_last_path()]
    canv_a, canv_b = [torch.zeros_like(p) for p in dev], [torch.zeros_like(p) for p in dev]
    K.image_tiles_scatter(batch, canv_a, chunk.tiles, T, T)
    K.image_tiles_scatter(batch, canv_b, chunk.tiles, T, T, clip=True)
    paths.append(K.image_tiles_last_path())
    assert all(torch.equal(a, b) and torch.equal(a, p) for a, b, p in zip(canv_a, canv_b, dev))
    work = {
        "gather": lambda: K.image_tiles_gather(dev, chunk.tiles, T, T),
        "gather, pad=True": lambda: K.image_tiles_gather(dev, chunk.tiles, T, T, pad=True),
        "scatter": lambda: K.image_tiles_scatter(batch, canv_a, chunk.tiles, T, T),
        "scatter, clip=True": lambda: K.image_tiles_scatter(batch, canv_b, chunk.tiles, T, T, clip=True),
    }
    micro = {name: [] for name in work}
    for _ in range(args.rounds):
        for name, fn in work.items():
            def window(fn=fn):
                for _ in range(args.reps):
                    fn()
            micro[name].append(timed(window)[0] / args.reps)
    moved = 5 * 3 * T * T * n      # one byte and one float per sample
    say()
    say(f"(c) the launches alone on a table with no edge tile: {n} tiles of {T} x {T} of 24 pictures, device-resident, outputs equal; microseconds per "
        f"call (table staging included), host clock over {args.reps} repetitions, median over {args.rounds} rounds")
    for name in work:
        m = statistics.median(micro[name])
        say(f"   {name:20s} {fmt(micro[name], 1e6)}   {moved / m / 1e9:7.0f} GB/s of {moved / 1e6:.0f} MB")
    say(f"   paths: gather {paths[0]}, scatter {paths[1]} (1 = wide)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
