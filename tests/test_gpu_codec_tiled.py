"""Tiled pictures through the codecs: ``compress_tiled`` writes, for every tile, EXACTLY the bytes ``compress`` writes for that crop at
batch 1 -- whatever the picture's memory, device, dtype and the chunking --, and ``decompress_tiled`` returns the picture at its own
size, equal to every tile's own ``decompress``, cropped and pasted; a region decodes only the tiles it touches; the harness logs the
container's length and the whole picture's distortion.  The yardstick is the codec itself on the crop, one call per tile."""
import functools

import pytest
import torch

from cbench_basic_amd.utils.tiling import TileGrid, unpack_tiled

pytestmark = pytest.mark.gpu

# (codec, H, W, tile), 3 x 4 tiles each.  160 x 224 in tiles of 64: the edge tiles 32 high and wide; 150 x 200: edge tiles 22 high and 8
# wide, which decode larger than they are and are cropped.  The two AR codecs (topo-group checkerboard, BaSIC scan-line) refuse a crop
# whose sides are no multiples of 64 in compress() itself ("Input and prior shape not aligned": the y coder is built with
# force_input_prior_shape_aligned, and h_s returns the next multiple of 4 latent rows and columns), so the yardstick does not exist for
# 32-wide crops; they get the nearest shape they accept with the same grid: 320 x 448 in tiles of 128, the edge tiles 64 high and wide.
CASES = [("hyperprior-fused", 160, 224, 64), ("hyperprior-modules", 160, 224, 64), ("checkerboard", 320, 448, 128), ("basic-l0", 320, 448, 128),
         ("hyperprior-fused", 150, 200, 64)]
IDS = [f"{k}-{h}x{w}" for k, h, w, _ in CASES]


@functools.lru_cache(maxsize=None)
def _codec(kind):
    from cbench_basic_amd.presets import basic_codec, hyperprior_codec, seed_synthetic_weights, topogroup_ar_codec
    if kind.startswith("hyperprior"):
        codec = hyperprior_codec()
    elif kind == "checkerboard":
        codec = topogroup_ar_codec("checkerboard")
    else:
        codec = basic_codec()
    codec = seed_synthetic_weights(codec, seed=0).eval().cuda()
    codec.update_state()
    if kind == "hyperprior-modules":
        codec.entropy_coder.use_fused_session = False
    if kind == "basic-l0":
        codec.set_complex_level(0)
    return codec


def _picture(H, W):
    """A smooth picture with some noise, uint8 [1, 3, H, W] on the host: tiles differ from one another and code to different lengths."""
    g = torch.Generator().manual_seed(H * 1000 + W)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([(yy / H + xx / W) / 2, (torch.sin(yy / 9) * torch.cos(xx / 13) + 1) / 2, (xx * yy) / (H * W)])
    return (base + 0.1 * torch.rand(3, H, W, generator=g)).clamp(0, 1).mul(255).round().to(torch.uint8)[None]


@functools.lru_cache(maxsize=None)
def _reference(kind, H, W, TILE):
    """Computed once per case and left unchanged: (picture, grid, [compress(crop_k)], the float canvas of the tiles' own
    decompress(), cropped and pasted)."""
    codec = _codec(kind)
    img = _picture(H, W)
    grid = TileGrid(H, W, TILE, TILE)
    strings, canvas = [], torch.full((1, 3, H, W), float("nan"), device="cuda")
    for k in range(len(grid)):
        y, x, h, w = grid.tile_rect(k)
        s = codec.compress(img[:, :, y:y + h, x:x + w])
        rec = codec.decompress(s)
        assert rec.shape[0] == 1 and rec.shape[1] == 3 and rec.shape[2] >= h and rec.shape[3] >= w, (kind, k, tuple(rec.shape))
        canvas[:, :, y:y + h, x:x + w] = rec[:, :, :h, :w]
        strings.append(s)
    assert not bool(torch.isnan(canvas).any())
    return img, grid, strings, canvas


# encode() / decode() calls of a pass over 3 x 4 tiles: the groups are 2 x 3, 2 x 1, 1 x 3 and 1 x 1 tiles; in chunks of at most five the
# first needs two calls
CALLS = {None: 4, 1: 12, 5: 5}


@pytest.mark.parametrize("kind,H,W,TILE", CASES, ids=IDS)
def test_tiles_keep_the_bytes_of_their_own_batch1_call(kind, H, W, TILE):
    codec = _codec(kind)
    img, grid, want, _ = _reference(kind, H, W, TILE)
    assert len(grid) == 12 and len(grid.groups()) == 4 and len(set(want)) > 1
    if kind == "hyperprior-fused":
        assert codec.entropy_coder._fused_session({}, None) is not None
    hwc = img.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    pictures = {"host chw": img, "device chw": img.cuda(), "host hwc": hwc, "device hwc": hwc.cuda(), "float host": img.float().div(255),
                "float device": img.cuda().float().div(255)}
    from cbench_basic_amd.nn.kernels import image_layout_of
    assert image_layout_of(hwc) == "hwc" and image_layout_of(hwc.cuda()) == "hwc"
    for name, pic in pictures.items():
        for max_batch in (None, 1, 5):
            data = codec.compress_tiled(pic, tile=(TILE, TILE), max_batch=max_batch)
            calls = codec.last_items_calls
            C, h, w, th, tw, got = unpack_tiled(data)
            assert (C, h, w, th, tw) == (3, H, W, TILE, TILE), (kind, name)
            assert [len(s) for s in got] == [len(s) for s in want], (kind, name, max_batch)
            assert got == want, (kind, name, max_batch)                  # every tile: byte for byte its own compress(crop)
            assert calls == CALLS[max_batch], (kind, name, max_batch, calls)
    assert codec.compress_tiled(img, tile=TILE) == codec.compress_tiled(img, tile=(TILE, TILE))
    # a tile as large as the picture: one tile, one call, the picture's own string
    one = codec.compress_tiled(img[:, :, :64, :128], tile=(64, 128))
    assert unpack_tiled(one)[5] == [codec.compress(img[:, :, :64, :128])] and codec.last_items_calls == 1
    with pytest.raises(ValueError):
        codec.compress_tiled(torch.cat([img, img]), tile=TILE)
    with pytest.raises(TypeError):
        codec.compress_tiled(img.double(), tile=TILE)
    with pytest.raises(ValueError):
        codec.compress_tiled(img, tile=0)


@pytest.mark.parametrize("kind,H,W,TILE", CASES, ids=IDS)
def test_picture_equals_the_tiles_own_reconstructions_pasted(kind, H, W, TILE):
    from cbench_basic_amd.nn import kernels as K
    from cbench_basic_amd.utils.tiling import pack_tiled
    codec = _codec(kind)
    img, grid, strings, canvas = _reference(kind, H, W, TILE)
    data = pack_tiled(3, H, W, TILE, TILE, strings)
    want_u8 = K.image_f32_to_u8(canvas)
    T = TILE
    for max_batch in (None, 1, 5):
        for dtype in (None, torch.float32):
            pic = codec.decompress_tiled(data, output_dtype=dtype, max_batch=max_batch)
            assert pic.dtype == torch.float32 and tuple(pic.shape) == (1, 3, H, W)      # the picture's own size
            assert torch.equal(pic, canvas), (kind, max_batch)
            assert codec.last_items_calls == CALLS[max_batch] and codec.last_tiles_decoded == 12
        pic = codec.decompress_tiled(data, max_batch=max_batch)      # the default: the 8-bit picture
        assert pic.dtype == torch.uint8 and tuple(pic.shape) == (1, 3, H, W) and K.image_layout_of(pic) == "chw"
        assert torch.equal(pic, want_u8), (kind, max_batch)
        assert codec.last_items_calls == CALLS[max_batch] and codec.last_tiles_decoded == 12
    for dtype, want in ((torch.uint8, want_u8), (torch.float32, canvas)):
        pic = codec.decompress_tiled(data, output_dtype=dtype, layout="hwc")
        assert tuple(pic.shape) == (1, 3, H, W) and K.image_layout_of(pic) == "hwc" and torch.equal(pic, want), (kind, dtype)
    # regions: through four interior tiles; through the four tiles of the last corner (edge tiles); inside one tile; the whole picture
    for region, tiles in (((T - 4, T - 4, T + 6, T + 6), 4), ((H - T // 2 - 8, W - T // 2 - 38, H, W), 4), ((3, T + 6, 9, T + 11), 1), ((0, 0, H, W), 12), ((0, 0, 1, W), 4)):
        y0, x0, y1, x1 = region
        for dtype, want in ((torch.uint8, want_u8), (None, canvas)):
            part = codec.decompress_tiled(data, output_dtype=dtype, region=region)
            assert tuple(part.shape) == (1, 3, y1 - y0, x1 - x0)
            assert torch.equal(part, want[:, :, y0:y1, x0:x1]), (kind, region, dtype)
            assert codec.last_tiles_decoded == tiles, (kind, region, codec.last_tiles_decoded)
    part = codec.decompress_tiled(data, region=(T - 4, T - 4, T + 6, T + 6), layout="hwc", max_batch=1)
    assert torch.equal(part, want_u8[:, :, T - 4:T + 6, T - 4:T + 6]) and codec.last_items_calls == 4
    for region in ((0, 0, H + 1, W), (0, 0, H, W + 1), (5, 5, 5, 9), (9, 5, 5, 9), (-1, 0, 5, 5), (H, 0, H + 1, 5)):
        with pytest.raises(ValueError):
            codec.decompress_tiled(data, region=region)
    with pytest.raises(ValueError):
        codec.decompress_tiled(data[:-1])
    with pytest.raises(ValueError):
        codec.decompress_tiled(data, layout="nhwc")
    with pytest.raises(TypeError):
        codec.decompress_tiled(data, output_dtype=torch.float16)
    # the round trip from the picture itself
    assert torch.equal(codec.decompress_tiled(codec.compress_tiled(img.cuda(), tile=TILE)), want_u8)


TILE = 64


def test_grouped_codec_passes_tiled_calls_to_its_active_member():
    from cbench_basic_amd.codecs.grouped import GroupedVariableRateCodec
    codec = _codec("hyperprior-fused")
    img, grid, strings, canvas = _reference("hyperprior-fused", 150, 200, TILE)
    group = GroupedVariableRateCodec([codec])
    data = group.compress_tiled(img, tile=TILE)
    assert unpack_tiled(data)[5] == strings and group.last_items_calls == 4
    assert torch.equal(group.decompress_tiled(data, output_dtype=None, region=(60, 60, 70, 70)), canvas[:, :, 60:70, 60:70])
    assert group.last_tiles_decoded == 4


@pytest.mark.parametrize("on_uint8", [False, True], ids=["float-metrics", "uint8-metrics"])
def test_harness_codes_tiled_pictures(on_uint8, tmp_path):
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion
    from cbench_basic_amd.nn import kernels as K
    codec = _codec("hyperprior-fused")
    img, grid, strings, canvas = _reference("hyperprior-fused", 150, 200, TILE)
    data = codec.compress_tiled(img, tile=(TILE, TILE))
    bench = BasicLosslessCompressionBenchmark(codec, [img], distortion_metric=PytorchBatchedDistortion(metrics="psnr"), output_dir=str(tmp_path),
                                              testing_tile=(TILE, TILE), metrics_on_uint8=on_uint8)
    got = bench.run_benchmark(ignore_exist_metrics=True)
    bench.close()
    length = [v for k, v in got.items() if k.endswith("compressed_length")]
    psnr = [v for k, v in got.items() if k.endswith("psnr")]
    assert len(length) == 1 and len(psnr) == 1
    assert length[0] == len(data)                                   # the container's length
    assert [v for k, v in got.items() if k.endswith("original_length")] == [3 * 150 * 200]
    # the distortion of the whole pasted picture, from the metric the harness uses
    if on_uint8:
        want = PytorchBatchedDistortion(metrics="psnr")(K.image_f32_to_u8(canvas), img.cuda())["psnr"]
    else:
        want = PytorchBatchedDistortion(metrics="psnr")(canvas, K.image_u8_to_f32(img.cuda()))["psnr"]
    print("psnr", psnr[0], "want", float(want))
    assert abs(psnr[0] - float(want)) <= 1e-9 * max(1.0, abs(float(want))), (psnr[0], float(want))
    with pytest.raises(ValueError):          # tiles and coalesced items do not combine
        BasicLosslessCompressionBenchmark(codec, [img], testing_tile=(TILE, TILE), testing_coalesce_items=4)
    with pytest.raises(ValueError):          # a tiled item is one picture
        BasicLosslessCompressionBenchmark(codec, [torch.cat([img, img])], testing_tile=TILE, output_dir=str(tmp_path / "b")).run_benchmark(
            ignore_exist_metrics=True)


def test_harness_tiled_pass_with_stream_workers(tmp_path):
    """Two pictures coded by two stream workers, each through its own replica's compress_tiled: the sizes and the distortion of the
    sequential tiled pass."""
    from cbench_basic_amd import presets
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion
    codec = _codec("hyperprior-fused")
    items = [_picture(150, 200), _picture(150, 200).flip(3).contiguous()]
    res = {}
    for tag, workers in (("seq", 0), ("workers", 2)):
        bench = BasicLosslessCompressionBenchmark(codec, items, distortion_metric=PytorchBatchedDistortion(metrics="psnr"),
                                                  output_dir=str(tmp_path / tag), testing_tile=TILE, metrics_on_uint8=True, num_testing_workers=workers,
                                                  codec_builder=(lambda: presets.seed_synthetic_weights(presets.hyperprior_codec(), seed=0)) if workers else None)
        res[tag] = bench.run_benchmark(ignore_exist_metrics=True)
        bench.close()
    want = sum(len(codec.compress_tiled(x, tile=TILE)) for x in items) / 2
    for k in res["seq"]:
        if k.endswith(("compressed_length", "psnr", "original_length")):
            assert res["seq"][k] == res["workers"][k], (k, res["seq"][k], res["workers"][k])
        if k.endswith("compressed_length"):
            assert res["seq"][k] == want
