"""Overlapped tiles of one large picture, measured (the record is profiles/tiled_blend.txt).

The picture and codec of scripts/tiled_probe.py -- a synthetic uint8 4096 x 6144 picture in [H][W][C] host memory, the hyperprior codec
with seeded weights --, tiles of 512, overlaps 0 / 32 / 64, at most as many tiles per encode() / decode() call as tiled_probe.py takes:
  1. compress_tiled + decompress_tiled(output_dtype=uint8), and decompress_tiled alone, per overlap: every route warmed once, then
     timed in alternating rounds (overlap 0, 32, 64, 0, 32, 64, ...), a host clock around work that ends in a device synchronise;
  2. the blend launch alone (basic_image_tiles_blend_dev through ctypes, the table already on the device), device events around 20
     launches, against the bytes it moves: four per source float read -- one, two or four floats per sample, from the geometry --
     and one per uint8 sample written; and nn.kernels.image_tiles_blend, which also builds and uploads the table, on the host clock.
The three comparisons the record states are computed here: (a) the launch against the HBM rate, (b) overlap 0 against the parent's
time for the same route in profiles/tiled_coding.txt, (c) overlap o against overlap 0 scaled by the coded area.

    python scripts/tiled_blend_probe.py [--height 4096 --width 6144 --tile 512 --overlaps 0 32 64 --rounds 3] [--out FILE]
"""
import argparse
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 6300.0      # what a float4 copy achieves on this part (8000 GB/s on paper)


def parent_time_ms(tile):
    """The median of route 2 (compress_tiled + decompress_tiled) for this tile size in profiles/tiled_coding.txt, or None."""
    try:
        text = open(os.path.join(ROOT, "profiles", "tiled_coding.txt")).read()
    except OSError:
        return None
    m = re.search(rf"tiles of {tile} x {tile}:.*\n\s+2\. compress_tiled \+ decompress_tiled\s+median\s+([0-9.]+) ms", text)
    return float(m.group(1)) if m else None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=6144)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlaps", type=int, nargs="+", default=[0, 32, 64])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--call-mpix", type=float, default=8.4, help="pixels per encode() / decode() call, in 2^20 pixels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: nothing here is measured on a CPU")
    from cbench_basic_amd import _lib, presets
    from cbench_basic_amd.nn import kernels as K
    from cbench_basic_amd.utils.tiling import TileGrid, unpack_tiled_any
    from scripts.tiled_probe import picture, timed

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    H, W, T = args.height, args.width, args.tile
    mpix = H * W / 1e6
    codec = presets.seed_synthetic_weights(presets.hyperprior_codec(), seed=0).eval().cuda()
    codec.update_state()
    img = picture(H, W)
    per_call = max(1, int(args.call_mpix * 2 ** 20) // (T * T))
    say(f"picture: uint8 {H} x {W} x 3, [H][W][C] host memory, {mpix:.1f} Mpix; hyperprior codec, seeded weights; tiles of {T} x {T}, at most "
        f"{per_call} per call; {torch.cuda.get_device_name(0)}")

    state = {}

    def both(o):
        state[o] = codec.compress_tiled(img, tile=(T, T), max_batch=per_call, overlap=o)
        state["enc_calls", o] = codec.last_items_calls
        return codec.decompress_tiled(state[o], output_dtype=torch.uint8, max_batch=per_call)

    def decode(o):
        out = codec.decompress_tiled(state[o], output_dtype=torch.uint8, max_batch=per_call)
        state["dec_calls", o] = codec.last_items_calls
        return out

    for o in args.overlaps:      # warm every shape the timed window uses
        timed(lambda: both(o))
        timed(lambda: decode(o))
    t_both, t_dec = {o: [] for o in args.overlaps}, {o: [] for o in args.overlaps}
    for _ in range(args.rounds):
        for o in args.overlaps:
            t_both[o].append(timed(lambda: both(o))[0])
            t_dec[o].append(timed(lambda: decode(o))[0])

    say()
    say("1. end to end, ms per picture, medians (min .. max) over %d alternating rounds" % args.rounds)
    area = {}
    for o in args.overlaps:
        grid = TileGrid(H, W, T, T, overlap=o)
        area[o] = sum(h * w for _, _, h, w in (grid.tile_rect(k) for k in range(len(grid)))) / (H * W)
        a, b = t_both[o], t_dec[o]
        say(f"  overlap {o:3d}: {grid.rows} x {grid.cols} = {len(grid):3d} tiles, {state['enc_calls', o]} + {state['dec_calls', o]} calls, coded area "
            f"{area[o]:.3f} of the picture, container {len(state[o])} bytes ({unpack_tiled_any(state[o])[5]}, {state[o][:4].decode()})")
        say(f"      compress_tiled + decompress_tiled  {statistics.median(a) * 1e3:8.1f} ({min(a) * 1e3:.1f} .. {max(a) * 1e3:.1f})"
            f"      decompress_tiled alone  {statistics.median(b) * 1e3:8.1f} ({min(b) * 1e3:.1f} .. {max(b) * 1e3:.1f})")

    say()
    say("2. the blend alone, every tile's reconstruction resident, uint8 [H][W][C] output")
    blend_ms = {}
    for o in [o for o in args.overlaps if o]:
        grid = TileGrid(H, W, T, T, overlap=o)
        strings = unpack_tiled_any(state[o])[6]
        outs = codec.decompress_items(strings, max_batch=per_call)      # [1, C, sh, sw] views of the chunks' batches
        recs = [(r, [k]) for k, r in enumerate(outs)]
        out = torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda").permute(0, 3, 1, 2)
        K.image_tiles_blend(recs, grid, out)
        path = K.image_tiles_last_path()
        assert torch.equal(out, decode(o))
        resident = sum(r.numel() * 4 for r, _ in recs)
        table = np.zeros(len(grid), dtype=np.dtype([("src", "<u8"), ("sh", "<i4"), ("sw", "<i4")]))
        for r, indices in recs:
            n, C, sh, sw = r.shape
            for t, k in enumerate(indices):
                table[k] = (r.data_ptr() + 4 * t * C * sh * sw, sh, sw)
        d_table = torch.from_numpy(table.view(np.uint8)).cuda()
        L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream

        def launch():
            _lib.check(L.basic_image_tiles_blend_dev(d_table.data_ptr(), H, W, T, T, o, o, 3, 0, 0, H, W, out.data_ptr(), _lib.PIXEL_U8, _lib.IMAGE_HWC, st))
        launch()
        reps = 20
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            launch()
        stop.record()
        torch.cuda.synchronize()
        ms = blend_ms[o] = start.elapsed_time(stop) / reps
        floats = 3 * (H + (grid.rows - 1) * o) * (W + (grid.cols - 1) * o)      # one per covering tile and sample
        moved = 4 * floats + 3 * H * W
        wrapper = statistics.median(timed(lambda: K.image_tiles_blend(recs, grid, out))[0] for _ in range(5)) * 1e3
        say(f"  overlap {o:3d}: launch {ms:7.3f} ms (path {path}), {moved / 1e6:.0f} MB moved ({4 * floats / 1e6:.0f} read, {3 * H * W / 1e6:.0f} written): "
            f"{moved / ms / 1e6:.0f} GB/s; image_tiles_blend with its table upload {wrapper:.3f} ms on the host clock; "
            f"reconstructions resident {resident / 1e6:.0f} MB")
        del recs, out, d_table

    say()
    say("3. what the figures say")
    for o, ms in blend_ms.items():
        grid = TileGrid(H, W, T, T, overlap=o)
        moved = 4 * 3 * (H + (grid.rows - 1) * o) * (W + (grid.cols - 1) * o) + 3 * H * W
        say(f"  (a) overlap {o}: the blend launch moves {moved / 1e6:.0f} MB in {ms:.3f} ms = {moved / ms / 1e6:.0f} GB/s, {100 * moved / ms / 1e6 / HBM_GBS:.0f} % of the "
            f"{HBM_GBS:.0f} GB/s a float4 copy reaches on this part")
    if 0 in args.overlaps:
        base, base_dec = statistics.median(t_both[0]) * 1e3, statistics.median(t_dec[0]) * 1e3
        parent = parent_time_ms(T)
        spread = (max(t_both[0]) - min(t_both[0])) / statistics.median(t_both[0])
        if parent is not None:
            say(f"  (b) overlap 0, compress_tiled + decompress_tiled: {base:.1f} ms against {parent:.1f} ms in profiles/tiled_coding.txt (the parent commit, the same "
                f"route and code path): {base / parent:.3f} of it; this run's spread {spread:.3f} of the median")
        for o in blend_ms:
            t, d = statistics.median(t_both[o]) * 1e3, statistics.median(t_dec[o]) * 1e3
            say(f"  (c) overlap {o}: {t:.1f} ms against {base:.1f} ms x {area[o]:.3f} (coded area) = {base * area[o]:.1f} ms: a remainder of {t - base * area[o]:+.1f} ms; "
                f"decompress_tiled alone {d:.1f} against {base_dec:.1f} x {area[o]:.3f} = {base_dec * area[o]:.1f} ms: {d - base_dec * area[o]:+.1f} ms, of which the "
                f"blend launch is {blend_ms[o]:.3f} ms")

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
