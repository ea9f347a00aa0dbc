#!/usr/bin/env python3
"""Run the codec benchmark on one MI355X and write metrics.csv / metrics_2d.csv (the artefacts of the reference's
tools/run_benchmark.py for the testing half of a benchmark config).

  python tools/run_benchmark.py --codec hyperprior --images /data/kodak --out runs/hp_kodak
  python tools/run_benchmark.py --codec meanscale --synthetic 8 --qsteps 1 2 4 --out runs/ms_q
  python tools/run_benchmark.py --codec basic --synthetic 8 --size 256 --complexity-levels 0 1 2 3 4 5 6 7 --out runs/basic
  python tools/run_benchmark.py --codec topogroup --method checkerboard --synthetic 4 --out runs/ckbd

Weights: --checkpoint takes a state_dict saved from the reference (keys as in INTEGRATION.md); without it the
seeded synthetic weights of cbench_basic_amd.presets are used (plumbing / throughput runs).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def save_reconstructions(codec, batches, directory):
    """Decompresses every batch as 8-bit pictures (``output_dtype=torch.uint8``: converted on the GPU, one byte per sample
    downloaded) and writes one PNG per image, ``00000.png`` ... in dataset order.  -> the files written."""
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    files = []
    for b in batches:
        pictures = codec.decompress(codec.compress(b), output_dtype=torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        for a in pictures:
            files.append(os.path.join(directory, f"{len(files):05d}.png"))
            Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a).save(files[-1])
    return files


class ReconstructionWriter:
    """The harness' ``on_reconstruction`` callback: writes the picture the metric saw for every image of every tested level as
    ``directory/<level prefix>/NNNNN.png`` (no folder level without a level prefix), NNNNN = the image's place in the dataset."""

    def __init__(self, directory, batches):
        self.directory, self.files = directory, []
        self.first_image = [0]   # of every dataset item
        for b in batches:
            self.first_image.append(self.first_image[-1] + int(b.shape[0]))

    def __call__(self, level_prefix, item_index, picture_u8):
        from PIL import Image
        folder = os.path.join(self.directory, level_prefix) if level_prefix else self.directory
        os.makedirs(folder, exist_ok=True)
        for j, a in enumerate(picture_u8.permute(0, 2, 3, 1).cpu().numpy()):
            self.files.append(os.path.join(folder, f"{self.first_image[item_index] + j:05d}.png"))
            Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a).save(self.files[-1])


STEP_CODECS = ("hyperprior", "meanscale")   # the codecs whose y coder takes a quantiser step (--qsteps, --target-bpp, --tile-*)


def parse_args(argv=None):
    """The command line, parsed and checked (argparse's error exit, status 2, for a refused combination).  Host code: nothing here
    touches the GPU."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--codec", choices=["hyperprior", "meanscale", "topogroup", "basic"], default="hyperprior",
                    help="hyperprior: the scale hyperprior; meanscale: the mean-scale hyperprior (presets.mean_scale_hyperprior_codec)")
    ap.add_argument("--method", default="checkerboard", help="topo-group pattern of --codec topogroup")
    ap.add_argument("--checkpoint", default=None, help="state_dict (.pt) of the entropy coder or of the whole codec")
    ap.add_argument("--images", default=None, help="folder of PNG/JPEG images")
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic images (torch.manual_seed(i); rand)")
    ap.add_argument("--size", type=int, default=256, help="height = width of the synthetic images")
    ap.add_argument("--height", type=int, default=None, help="synthetic image height (default --size)")
    ap.add_argument("--width", type=int, default=None, help="synthetic image width (default --size)")
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--complexity-levels", type=int, nargs="*", default=[])
    ap.add_argument("--rate-levels", type=int, nargs="*", default=[])
    ap.add_argument("--forward-pass", action="store_true", help="also record the forward-pass rate estimate")
    ap.add_argument("--complexity-search", action="store_true",
                    help="--codec basic: find the complexity levels with the greedy search over the test images "
                         "(post_training_process) instead of the fixed ladder")
    ap.add_argument("--warmup", action="store_true",
                    help="code the first batch once before the timed run (plan building, table upload, graph capture are "
                         "one-time costs; the reference's harness has no such step)")
    ap.add_argument("--workers", type=int, default=0,
                    help="num_testing_workers: concurrent stream workers on the GPU, each with its own replica of the codec; dataset "
                         "items are coded concurrently (the reference's multiprocessing pool, basic_benchmark.py:829-858, GPU-native)")
    ap.add_argument("--coalesce", type=int, default=0,
                    help="testing_coalesce_items: code the batch-1 items of the dataset in calls of up to this many items of one shape; "
                         "every item keeps the bytes of its own batch-1 call (needs --batch-size 1)")
    ap.add_argument("--tile", type=int, nargs="+", default=None, metavar=("TH", "TW"),
                    help="testing_tile: code every picture as independent TH x TW tiles (TW = TH when omitted) through compress_tiled / "
                         "decompress_tiled; compressed_length is the container's, the distortion the whole picture's (needs "
                         "--batch-size 1, does not combine with --coalesce above 1)")
    ap.add_argument("--tile-overlap", type=int, nargs="+", default=None, metavar=("OY", "OX"),
                    help="testing_tile_overlap: neighbouring tiles share OY rows and OX columns (OX = OY when omitted; at most half a tile) and "
                         "decompress_tiled cross-fades the seams (needs --tile)")
    ap.add_argument("--tile-pad", type=int, nargs="+", default=None, metavar=("PY", "PX"),
                    help="testing_tile_pad: code the edge tiles at their size rounded up to multiples of PY x PX (PX = PY when omitted; must "
                         "divide the tile), the picture's last row and column replicated; decompress_tiled crops (needs --tile)")
    ap.add_argument("--tile-pool", type=int, default=0, metavar="N",
                    help="testing_tile_pool: code up to N consecutive pictures, of any sizes, per call, the tiles of all of them pooled "
                         "into shared coding calls (compress_tiled_items / decompress_tiled_items); every picture keeps its own container "
                         "(needs --tile, does not combine with --workers above 1)")
    ap.add_argument("--stream-lanes", type=int, default=1,
                    help="lane streams per image of the y-coder, any codec (a format the reference does not read)")
    ap.add_argument("--stream-rows", action="store_true",
                    help="--codec basic: one stream per latent row of the scan-line y-coder (a format the reference does not read)")
    ap.add_argument("--scanline-decode-schedule", choices=["auto", "raster", "wavefront", "band"], default="auto",
                    help="--stream-rows: how the scan-line y-coder's persistent decode launch walks the row streams (wavefront: one "
                         "decoder wavefront per row, batch * H <= 64; band: any batch and height; both raise where the call does not fit)")
    ap.add_argument("--metrics", nargs="+", choices=["psnr", "ms-ssim"], default=["psnr"],
                    help="distortion metrics of the reconstruction (ms-ssim needs images with both sides above 160)")
    ap.add_argument("--uint8", action="store_true",
                    help="the datasets yield 8-bit images (an image file's own bytes; synthetic: torch.randint): uploaded as bytes and "
                         "converted on the GPU; original_length, compression_ratio and speed_* then count one byte per sample")
    ap.add_argument("--save-reconstructions", default=None, metavar="DIR",
                    help="after the run, decompress every item as an 8-bit picture and write one PNG per image into DIR "
                         "(with --metrics-on-uint8: the pictures the run measured, DIR/<level prefix>/NNNNN.png for every tested level)")
    ap.add_argument("--metrics-on-uint8", action="store_true",
                    help="measure the 8-bit picture: decompress(output_dtype=torch.uint8) inside the timed region, the distortion from "
                         "exact integers against the 8-bit item (a float item: quantised once)")
    ap.add_argument("--qsteps", type=float, nargs="+", default=[], metavar="Q",
                    help="testing_qsteps, --codec hyperprior or meanscale: one pass per quantiser step of the y coder through compress_q / decompress_q "
                         "(level prefix q<step>; 1 is the codec as trained, above 1 fewer bits); every step in [0.0625, 64].  Composes with "
                         "--uint8, --metrics-on-uint8, --workers and --stream-lanes; not with --coalesce, --tile* or --complexity-levels")
    ap.add_argument("--target-bpp", type=float, nargs="+", default=[], metavar="R",
                    help="testing_target_bpps, --codec hyperprior or meanscale: one pass per rate target through compress_to_rate / decompress_q (level "
                         "prefix bpp<target>): every item's step is chosen on the GPU so that its payload fits floor(R * H * W / 8) bytes.  "
                         "Composes and refuses as --qsteps does, and does not combine with it")
    ap.add_argument("--tile-qsteps", type=float, nargs="+", default=[], metavar="Q",
                    help="testing_tile_qsteps, --codec hyperprior or meanscale with --tile: one pass per quantiser step through compress_tiled_q / "
                         "decompress_tiled (level prefix tq<step>; the BTQ1 container carries the step); every step in [0.0625, 64].  "
                         "Composes with --tile-overlap, --tile-pad, --tile-pool, --uint8 and --metrics-on-uint8; not with --qsteps, "
                         "--target-bpp, --coalesce, --complexity-levels, --rate-levels or --forward-pass")
    ap.add_argument("--tile-target-bpp", type=float, nargs="+", default=[], metavar="R",
                    help="testing_tile_target_bpps, --codec hyperprior or meanscale with --tile: one pass per rate target through compress_tiled_to_rate "
                         "(level prefix tbpp<target>): ONE step per picture is chosen on the GPU so that the whole container, framing "
                         "included, fits floor(R * H * W / 8) bytes.  Composes and refuses as --tile-qsteps does, and does not combine with it")
    ap.add_argument("--skip-rows", type=int, nargs="+", default=[], metavar="R",
                    help="testing_skip_rows, --codec hyperprior or meanscale: one pass per value through compress_skip / decompress_skip (level "
                         "prefix skip<R>): y elements whose scale-table row is below R are not coded and decode as 0 (the mean); R in "
                         "[0, 64], 0 skips nothing.  Composes with --uint8, --metrics-on-uint8, --workers and --stream-lanes; not with "
                         "--qsteps, --target-bpp, --coalesce, --tile*, --complexity-levels, --rate-levels or --forward-pass")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    if args.skip_rows:
        from cbench_basic_amd.utils.skip import check_skip_rows
        if args.codec not in STEP_CODECS:
            ap.error("--skip-rows is skip coding of the hyperprior y coder: it needs --codec hyperprior or --codec meanscale")
        for name, on in (("--qsteps", bool(args.qsteps)), ("--target-bpp", bool(args.target_bpp)), ("--tile-qsteps", bool(args.tile_qsteps)),
                         ("--tile-target-bpp", bool(args.tile_target_bpp)), ("--coalesce", args.coalesce > 1), ("--tile", args.tile is not None),
                         ("--tile-overlap", args.tile_overlap is not None), ("--tile-pad", args.tile_pad is not None),
                         ("--tile-pool", args.tile_pool > 0), ("--complexity-levels", bool(args.complexity_levels)),
                         ("--rate-levels", bool(args.rate_levels)), ("--forward-pass", args.forward_pass)):
            if on:
                ap.error(f"--skip-rows does not combine with {name}: the rows are a knob of compress_skip / decompress_skip alone")
        try:
            for r in args.skip_rows:
                check_skip_rows(r)
        except ValueError as e:
            ap.error(f"--skip-rows: {e}")
    for flag, values, other in (("--tile-qsteps", args.tile_qsteps, ("--tile-target-bpp", bool(args.tile_target_bpp))),
                                ("--tile-target-bpp", args.tile_target_bpp, ("--tile-qsteps", bool(args.tile_qsteps)))):
        if not values:
            continue
        import math
        if args.codec not in STEP_CODECS:
            ap.error(f"{flag} is a knob of the hyperprior y coder's quantiser step: it needs --codec hyperprior or --codec meanscale")
        if args.tile is None:
            ap.error(f"{flag} needs --tile: the untiled knobs are --qsteps and --target-bpp")
        for name, on in (other, ("--qsteps", bool(args.qsteps)), ("--target-bpp", bool(args.target_bpp)), ("--coalesce", args.coalesce > 1),
                         ("--complexity-levels", bool(args.complexity_levels)), ("--rate-levels", bool(args.rate_levels)),
                         ("--forward-pass", args.forward_pass)):
            if on:
                ap.error(f"{flag} does not combine with {name}: it is a knob of the tiled calls alone")
        if flag == "--tile-qsteps":
            from cbench_basic_amd.utils.qstep import check_qsteps
            try:
                for q in values:
                    check_qsteps(q)
            except ValueError as e:
                ap.error(f"--tile-qsteps: {e}")
        else:
            for r in values:
                if not (math.isfinite(r) and r > 0):
                    ap.error(f"--tile-target-bpp: every target must be positive and finite, got {r}")
    if args.target_bpp:
        import math
        if args.codec not in STEP_CODECS:
            ap.error("--target-bpp chooses the hyperprior y coder's quantiser step: it needs --codec hyperprior or --codec meanscale")
        for name, on in (("--qsteps", bool(args.qsteps)), ("--coalesce", args.coalesce > 1), ("--tile", args.tile is not None),
                         ("--tile-overlap", args.tile_overlap is not None), ("--tile-pad", args.tile_pad is not None),
                         ("--tile-pool", args.tile_pool > 0), ("--complexity-levels", bool(args.complexity_levels)),
                         ("--rate-levels", bool(args.rate_levels)), ("--forward-pass", args.forward_pass)):
            if on:
                ap.error(f"--target-bpp does not combine with {name}: the target is a knob of compress_to_rate alone")
        for r in args.target_bpp:
            if not (math.isfinite(r) and r > 0):
                ap.error(f"--target-bpp: every target must be positive and finite, got {r}")
    if args.qsteps:
        from cbench_basic_amd.utils.qstep import check_qsteps
        if args.codec not in STEP_CODECS:
            ap.error("--qsteps is the hyperprior y coder's quantiser step: it needs --codec hyperprior or --codec meanscale (the PGM coders' "
                     "knob is quantizer_params)")
        for name, on in (("--coalesce", args.coalesce > 1), ("--tile", args.tile is not None), ("--tile-overlap", args.tile_overlap is not None),
                         ("--tile-pad", args.tile_pad is not None), ("--tile-pool", args.tile_pool > 0),
                         ("--complexity-levels", bool(args.complexity_levels)), ("--rate-levels", bool(args.rate_levels)),
                         ("--forward-pass", args.forward_pass)):
            if on:
                ap.error(f"--qsteps does not combine with {name}: the step is a knob of compress_q / decompress_q alone")
        try:
            for q in args.qsteps:
                check_qsteps(q)
        except ValueError as e:
            ap.error(f"--qsteps: {e}")
    if args.stream_rows and args.codec != "basic":
        ap.error("--stream-rows needs --codec basic")
    if args.scanline_decode_schedule != "auto" and not args.stream_rows:
        ap.error("--scanline-decode-schedule needs --stream-rows: only row streams have a decode schedule")
    if not 1 <= args.stream_lanes <= 256:
        ap.error("--stream-lanes must be in [1, 256]")
    if args.coalesce and args.batch_size != 1:
        ap.error("--coalesce codes batch-1 items: it does not combine with --batch-size other than 1")
    if args.coalesce < 0:
        ap.error("--coalesce must be >= 0")
    if args.tile is not None:
        if len(args.tile) > 2 or min(args.tile) < 1:
            ap.error("--tile takes TH [TW], positive")
        if args.coalesce > 1 or args.batch_size != 1:
            ap.error("--tile codes one picture per call: it does not combine with --coalesce above 1 or --batch-size other than 1")
        args.tile = (args.tile[0], args.tile[-1])
    if args.tile_overlap is not None:
        if args.tile is None:
            ap.error("--tile-overlap needs --tile")
        if len(args.tile_overlap) > 2 or min(args.tile_overlap) < 0:
            ap.error("--tile-overlap takes OY [OX], not negative")
        args.tile_overlap = (args.tile_overlap[0], args.tile_overlap[-1])
        if 2 * args.tile_overlap[0] > args.tile[0] or 2 * args.tile_overlap[1] > args.tile[1]:
            ap.error("--tile-overlap is at most half a tile")
    else:
        args.tile_overlap = (0, 0)
    if args.tile_pad is not None:
        if args.tile is None:
            ap.error("--tile-pad needs --tile")
        if len(args.tile_pad) > 2 or min(args.tile_pad) < 1:
            ap.error("--tile-pad takes PY [PX], positive")
        args.tile_pad = (args.tile_pad[0], args.tile_pad[-1])
        if args.tile[0] % args.tile_pad[0] or args.tile[1] % args.tile_pad[1]:
            ap.error("--tile-pad must divide the tile")
    if args.tile_pool < 0:
        ap.error("--tile-pool must be >= 0")
    if args.tile_pool:
        if args.tile is None:
            ap.error("--tile-pool needs --tile")
        if args.workers > 1:
            ap.error("--tile-pool runs on the calling thread: it does not combine with --workers above 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    pad = {} if args.tile_pad is None else dict(pad_to=args.tile_pad)
    if args.workers > 1:   # before HIP initialises: one hardware queue per worker stream
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
        os.environ.setdefault("BASIC_RANS_WPB", "8")
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: the codec has no CPU path")

    from cbench_basic_amd import presets
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion
    from cbench_basic_amd.data import ImageFolderDataset, RandomImageDataset, batched
    dtype = torch.uint8 if args.uint8 else torch.float32
    if args.images:
        ds = ImageFolderDataset(args.images, dtype=dtype)
    else:
        ds = RandomImageDataset(num=args.synthetic or 8, size=(3, args.height or args.size, args.width or args.size), dtype=dtype)
    batches = list(batched(ds, args.batch_size))
    builders = dict(hyperprior=lambda: presets.hyperprior_codec(stream_lanes=args.stream_lanes),
                    meanscale=lambda: presets.mean_scale_hyperprior_codec(stream_lanes=args.stream_lanes), basic=lambda **kw: presets.basic_codec(stream_lanes=args.stream_lanes, stream_rows=args.stream_rows,
                                                              scanline_decode_schedule=args.scanline_decode_schedule, **kw),
                    topogroup=lambda: presets.topogroup_ar_codec(method=args.method, stream_lanes=args.stream_lanes))
    codec = builders["basic"](search_dataset=batches) if (args.codec == "basic" and args.complexity_search) else builders[args.codec]()
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu")
        sd = sd.get("state_dict", sd)
        missing = codec.load_state_dict(sd, strict=False) if any(k.startswith("entropy_coder.") for k in sd) \
            else codec.entropy_coder.load_state_dict(sd, strict=False)
        print("checkpoint loaded; missing keys:", len(missing.missing_keys), "unexpected:", len(missing.unexpected_keys))
    else:
        presets.seed_synthetic_weights(codec, seed=0)
    codec = codec.eval().to("cuda")

    def warm(c):   # one item through the route the pass takes
        if args.tile_target_bpp:   # the tiled rate route: the module path's plans, the cost table, the group select
            c.decompress_tiled(c.compress_tiled_to_rate(batches[0].to("cuda"), target_bpp=args.tile_target_bpp[0], tile=args.tile,
                                                        overlap=args.tile_overlap, **pad))
        elif args.tile_qsteps:
            c.decompress_tiled(c.compress_tiled_q(batches[0].to("cuda"), args.tile_qsteps[0], tile=args.tile, overlap=args.tile_overlap, **pad))
        elif args.tile_pool > 1:   # the first pooled call: the batch shapes the pass will meet
            c.decompress_tiled_items(c.compress_tiled_items(batches[:args.tile_pool], tile=args.tile, overlap=args.tile_overlap, **pad))
        elif args.tile is not None:
            c.decompress_tiled(c.compress_tiled(batches[0].to("cuda"), tile=args.tile, overlap=args.tile_overlap, **pad))
        elif args.target_bpp:   # the rate kernels' route: the cost table's upload, the session's rate buffers
            c.decompress_q(c.compress_to_rate(batches[0].to("cuda"), target_bpp=args.target_bpp[0]))
        elif args.qsteps:   # the step kernels' route, and the session's step buffers
            c.decompress_q(c.compress_q(batches[0].to("cuda"), args.qsteps[0]))
        elif args.skip_rows:   # the compaction's route, and the session's compact buffers
            c.decompress_skip(c.compress_skip(batches[0].to("cuda"), args.skip_rows[0]))
        else:
            c.decompress(c.compress(batches[0].to("cuda")))
    warm_chunks = []
    if args.coalesce > 1:
        from cbench_basic_amd.utils.item_framing import coalesce_chunks
        seen = set()
        for chunk in coalesce_chunks([tuple(b.shape) for b in batches], args.coalesce):
            if len(chunk) > 1 and (tuple(batches[chunk[0]].shape), len(chunk)) not in seen:
                seen.add((tuple(batches[chunk[0]].shape), len(chunk)))
                warm_chunks.append([batches[i] for i in chunk])
    if args.warmup:
        codec.update_state()
        for lvl in (args.complexity_levels or [None]):
            if lvl is not None:
                codec.set_complex_level(lvl)
            warm(codec)
            for chunk in warm_chunks:   # the coalesced calls' one-time costs: one chunk per (shape, size) the pass will make
                codec.decompress_items(codec.compress_items(chunk))
    writer = ReconstructionWriter(args.save_reconstructions, batches) if args.save_reconstructions and args.metrics_on_uint8 else None
    bench = BasicLosslessCompressionBenchmark(codec, batches, metrics_on_uint8=args.metrics_on_uint8, on_reconstruction=writer,
                                              distortion_metric=PytorchBatchedDistortion(metrics=args.metrics),
                                              nn_codec_use_forward_pass=args.forward_pass,
                                              testing_complexity_levels=args.complexity_levels,
                                              testing_variable_rate_levels=args.rate_levels, output_dir=args.out,
                                              num_testing_workers=args.workers, testing_coalesce_items=args.coalesce, testing_tile=args.tile, testing_tile_overlap=args.tile_overlap,
                                              testing_tile_pool=args.tile_pool, testing_tile_pad=args.tile_pad, testing_qsteps=args.qsteps,
                                              testing_target_bpps=args.target_bpp, testing_tile_qsteps=args.tile_qsteps,
                                              testing_tile_target_bpps=args.tile_target_bpp, testing_skip_rows=args.skip_rows,
                                              codec_builder=(lambda: presets.seed_synthetic_weights(builders[args.codec](), seed=0)) if args.workers > 1 else None)
    if args.workers > 1 and args.warmup:   # the replicas' one-time costs too, one replica at a time (HIP-graph capture)
        pool = bench._worker_pool(batches[0], batch=max((len(c) for c in warm_chunks), default=None))
        for r, st in zip(pool.codecs, pool.streams):
            with torch.cuda.stream(st):
                for lvl in (args.complexity_levels or [None]):
                    if lvl is not None:
                        r.set_complex_level(lvl)
                    warm(r)
                    for chunk in warm_chunks:
                        r.decompress_items(r.compress_items(chunk))
            torch.cuda.synchronize()
    metrics = bench.run_benchmark(ignore_exist_metrics=True)
    bench.close()
    print(json.dumps(metrics, indent=1))
    if writer is not None:          # the pictures the run measured, every tested level
        print(f"{len(writer.files)} reconstructions written to {args.save_reconstructions}")
    elif args.save_reconstructions:   # at the complexity and rate level the run ended on
        files = save_reconstructions(codec, batches, args.save_reconstructions)
        print(f"{len(files)} reconstructions written to {args.save_reconstructions}")
    return metrics


if __name__ == "__main__":
    main()
