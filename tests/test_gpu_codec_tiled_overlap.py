"""Overlapped tiles through the codecs: ``compress_tiled(..., overlap=)`` writes, for every tile, EXACTLY the bytes ``compress`` writes for
that overlapped crop at batch 1, and ``decompress_tiled`` returns the tiles' own ``decompress()`` cross-faded as include/basic_hip.h
section 8c defines -- bit for bit as float32, exactly as uint8 -- whatever the chunking, the layout and the region.  The yardstick is
the codec itself on each crop, one call per tile, blended by the numpy reference of tests/tile_blend_exact.py."""
import functools

import numpy as np
import pytest
import torch

import tile_blend_exact as E
from test_gpu_codec_tiled import _codec, _picture
from cbench_basic_amd.utils.tiling import TileGrid, pack_tiled, unpack_tiled, unpack_tiled_any

pytestmark = pytest.mark.gpu

# (codec, H, W, tile, overlap), 3 x 4 tiles each.  150 x 200 in tiles of 64 that share 16: steps of 48, the edge tiles 54 high and 56
# wide, four groups.  The two AR codecs take only crops whose sides are multiples of 64 (tests/test_gpu_codec_tiled.py), so they get
# 256 x 320 in tiles of 128 that share 64, the maximum: 3 x 4 full tiles in one group.
CASES = [("hyperprior-fused", 150, 200, 64, 16), ("hyperprior-modules", 150, 200, 64, 16), ("checkerboard", 256, 320, 128, 64),
         ("basic-l0", 256, 320, 128, 64)]
IDS = [f"{k}-{h}x{w}" for k, h, w, _, _ in CASES]
# encode() / decode() calls of a pass: four groups of 2 x 3, 2 x 1, 1 x 3 and 1 x 1 tiles, or one group of 3 x 4
CALLS = {1: {None: 1, 1: 12, 5: 3}, 4: {None: 4, 1: 12, 5: 5}}


@functools.lru_cache(maxsize=None)
def _reference(kind, H, W, TILE, OVER):
    """Computed once per case and left unchanged: (picture, grid, [compress(crop_k)], the reference blend of the tiles' own
    decompress() as a float32 tensor on the device, that quantised)."""
    codec = _codec(kind)
    img = _picture(H, W)
    grid = TileGrid(H, W, TILE, TILE, overlap=OVER)
    strings, tiles = [], {}
    for k in range(len(grid)):
        y, x, h, w = grid.tile_rect(k)
        s = codec.compress(img[:, :, y:y + h, x:x + w])
        rec = codec.decompress(s)
        assert rec.shape[0] == 1 and rec.shape[1] == 3 and rec.shape[2] >= h and rec.shape[3] >= w, (kind, k, tuple(rec.shape))
        tiles[k] = rec[0].cpu().numpy()
        strings.append(s)
    full = E.blend(grid, tiles)
    assert not np.isnan(full).any()
    return img, grid, strings, torch.from_numpy(full)[None].cuda(), torch.from_numpy(E.quantise(full))[None].cuda()


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("kind,H,W,TILE,OVER", CASES, ids=IDS)
def test_tiles_keep_the_bytes_of_their_own_batch1_call(kind, H, W, TILE, OVER):
    codec = _codec(kind)
    img, grid, want, _, _ = _reference(kind, H, W, TILE, OVER)
    groups = grid.groups()
    assert (grid.rows, grid.cols) == (3, 4) and len(groups) == (4 if H == 150 else 1) and len(set(want)) > 1
    if H == 150:
        assert sorted((g.ny, g.nx, g.h, g.w) for g in groups) == [(1, 1, 54, 56), (1, 3, 54, 64), (2, 1, 64, 56), (2, 3, 64, 64)]
    hwc = img.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    # the float picture is divided on the host and then moved: a division by a scalar on the device multiplies by the rounded
    # reciprocal, which is another picture by an ulp here and there (and, for basic-l0, another string for one tile)
    pictures = {"host chw": img, "device chw": img.cuda(), "host hwc": hwc, "device hwc": hwc.cuda(), "float host": img.float().div(255),
                "float device": img.float().div(255).cuda()}
    for name, pic in pictures.items():
        for max_batch in (None, 1, 5):
            data = codec.compress_tiled(pic, tile=(TILE, TILE), max_batch=max_batch, overlap=OVER)
            calls = codec.last_items_calls
            assert data[:4] == b"BTL2"
            C, h, w, th, tw, overlap, got = unpack_tiled_any(data)
            assert (C, h, w, th, tw, overlap) == (3, H, W, TILE, TILE, (OVER, OVER)), (kind, name)
            assert [len(s) for s in got] == [len(s) for s in want], (kind, name, max_batch)
            assert got == want, (kind, name, max_batch)                  # every tile: byte for byte its own compress(crop)
            assert calls == CALLS[len(groups)][max_batch], (kind, name, max_batch, calls)
    assert codec.compress_tiled(img, tile=TILE, overlap=(OVER, OVER)) == pack_tiled(3, H, W, TILE, TILE, want, overlap=OVER)
    # an overlap along one axis only
    one = unpack_tiled_any(codec.compress_tiled(img.cuda(), tile=TILE, overlap=(0, OVER)))
    g1 = TileGrid(H, W, TILE, TILE, overlap=(0, OVER))
    assert one[5] == (0, OVER) and len(one[6]) == len(g1)
    y, x, h, w = g1.tile_rect(len(g1) - 1)
    assert one[6][-1] == codec.compress(img[:, :, y:y + h, x:x + w])


@pytest.mark.parametrize("kind,H,W,TILE,OVER", CASES, ids=IDS)
def test_picture_is_the_reference_blend_of_the_tiles_own_reconstructions(kind, H, W, TILE, OVER):
    from cbench_basic_amd.nn import kernels as K
    codec = _codec(kind)
    img, grid, strings, want_f, want_u8 = _reference(kind, H, W, TILE, OVER)
    data = pack_tiled(3, H, W, TILE, TILE, strings, overlap=OVER)
    calls = CALLS[len(grid.groups())]
    for max_batch in (None, 1, 5):
        for dtype in (None, torch.float32):
            pic = codec.decompress_tiled(data, output_dtype=dtype, max_batch=max_batch)
            assert tuple(pic.shape) == (1, 3, H, W) and _same_bits(pic, want_f), (kind, max_batch)      # bit for bit
            assert codec.last_items_calls == calls[max_batch] and codec.last_tiles_decoded == 12
        pic = codec.decompress_tiled(data, max_batch=max_batch)      # the default: the 8-bit picture
        assert pic.dtype == torch.uint8 and tuple(pic.shape) == (1, 3, H, W) and K.image_layout_of(pic) == "chw"
        assert torch.equal(pic, want_u8), (kind, max_batch)
        assert codec.last_items_calls == calls[max_batch] and codec.last_tiles_decoded == 12
    for dtype, want in ((torch.uint8, want_u8), (torch.float32, want_f)):
        pic = codec.decompress_tiled(data, output_dtype=dtype, layout="hwc")
        assert tuple(pic.shape) == (1, 3, H, W) and K.image_layout_of(pic) == "hwc" and torch.equal(pic, want), (kind, dtype)
    # regions: inside tile 0's own area; across a band of columns; through a four-tile corner; the whole picture
    s = TILE - OVER
    for region, tiles in (((3, 5, 9, 20), 1), ((3, s - 4, 9, s + 6), 2), ((s + 2, s + 3, s + 7, s + 9), 4), ((0, 0, H, W), 12)):
        y0, x0, y1, x1 = region
        covering = [k for k in range(12) for y, x, h, w in [grid.tile_rect(k)] if y < y1 and y + h > y0 and x < x1 and x + w > x0]
        assert len(covering) == tiles, (region, covering)                # as the geometry predicts
        for dtype, want in ((torch.uint8, want_u8), (None, want_f)):
            for layout in ("chw", "hwc"):
                part = codec.decompress_tiled(data, output_dtype=dtype, region=region, layout=layout)
                assert tuple(part.shape) == (1, 3, y1 - y0, x1 - x0) and K.image_layout_of(part) in (layout, "chw")
                assert torch.equal(part, want[:, :, y0:y1, x0:x1]), (kind, region, dtype, layout)
                assert codec.last_tiles_decoded == tiles, (kind, region, codec.last_tiles_decoded)
    part = codec.decompress_tiled(data, region=(s + 2, s + 3, s + 7, s + 9), max_batch=1)
    assert torch.equal(part, want_u8[:, :, s + 2:s + 7, s + 3:s + 9]) and codec.last_items_calls == 4
    for region in ((0, 0, H + 1, W), (5, 5, 5, 9), (-1, 0, 5, 5)):
        with pytest.raises(ValueError):
            codec.decompress_tiled(data, region=region)
    # the round trip from the picture itself
    assert torch.equal(codec.decompress_tiled(codec.compress_tiled(img.cuda(), tile=TILE, overlap=OVER)), want_u8)


def test_overlap_zero_is_the_container_and_the_picture_as_they_were():
    codec = _codec("hyperprior-fused")
    img = _picture(150, 200)
    plain = codec.compress_tiled(img, tile=64)
    assert plain[:4] == b"BTL1"
    for zero in (0, (0, 0)):
        assert codec.compress_tiled(img, tile=64, overlap=zero) == plain
        assert codec.compress_tiled(img.cuda(), tile=(64, 64), max_batch=5, overlap=zero) == plain
    assert unpack_tiled_any(plain) == unpack_tiled(plain)[:5] + ((0, 0), unpack_tiled(plain)[5])
    # the picture: every tile's own decompress(), cropped and pasted
    grid = TileGrid(150, 200, 64, 64)
    want = torch.empty((1, 3, 150, 200), device="cuda")
    for k, s in enumerate(unpack_tiled(plain)[5]):
        y, x, h, w = grid.tile_rect(k)
        want[:, :, y:y + h, x:x + w] = codec.decompress(s)[:, :, :h, :w]
    assert _same_bits(codec.decompress_tiled(plain, output_dtype=None), want)
    assert _same_bits(codec.decompress_tiled(codec.compress_tiled(img, tile=64, overlap=0), output_dtype=torch.float32), want)


def test_overlaps_and_containers_that_are_refused():
    codec = _codec("hyperprior-fused")
    img = _picture(150, 200)
    for bad in (33, (33, 0), (0, 40), -1, (-1, 0), (0, -16), (1, 2, 3), 1.5):
        with pytest.raises(ValueError):
            codec.compress_tiled(img, tile=64, overlap=bad)
    assert codec.compress_tiled(img[:, :, :64, :96], tile=64, overlap=32)[:4] == b"BTL2"      # exactly half a tile is allowed
    data = codec.compress_tiled(img, tile=64, overlap=16)
    for cut in (data[:-1], data[:40], data[:4], data + b"\x00", b"BTL1" + data[4:]):
        with pytest.raises(ValueError):
            codec.decompress_tiled(cut)


def test_grouped_codec_passes_the_overlap_to_its_active_member():
    from cbench_basic_amd.codecs.grouped import GroupedVariableRateCodec
    codec = _codec("hyperprior-fused")
    img, grid, strings, want_f, want_u8 = _reference("hyperprior-fused", 150, 200, 64, 16)
    group = GroupedVariableRateCodec([codec])
    data = group.compress_tiled(img, tile=64, overlap=16)
    assert unpack_tiled_any(data)[5:] == ((16, 16), strings) and group.last_items_calls == 4
    assert _same_bits(group.decompress_tiled(data, output_dtype=None, region=(50, 50, 60, 60)), want_f[:, :, 50:60, 50:60].contiguous())
    assert group.last_tiles_decoded == 4
    assert torch.equal(group.decompress_tiled(data), want_u8)


@pytest.mark.parametrize("on_uint8", [False, True], ids=["float-metrics", "uint8-metrics"])
def test_harness_codes_overlapped_tiles(on_uint8, tmp_path):
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion
    from cbench_basic_amd.nn import kernels as K
    codec = _codec("hyperprior-fused")
    img, grid, strings, want_f, want_u8 = _reference("hyperprior-fused", 150, 200, 64, 16)
    data = pack_tiled(3, 150, 200, 64, 64, strings, overlap=16)
    bench = BasicLosslessCompressionBenchmark(codec, [img], distortion_metric=PytorchBatchedDistortion(metrics="psnr"), output_dir=str(tmp_path),
                                              testing_tile=(64, 64), testing_tile_overlap=16, metrics_on_uint8=on_uint8)
    got = bench.run_benchmark(ignore_exist_metrics=True)
    bench.close()
    length = [v for k, v in got.items() if k.endswith("compressed_length")]
    psnr = [v for k, v in got.items() if k.endswith("psnr")]
    assert len(length) == 1 and len(psnr) == 1
    assert length[0] == len(data)                                   # the BTL2 container's length
    assert [v for k, v in got.items() if k.endswith("original_length")] == [3 * 150 * 200]
    # the distortion of the whole blended picture, from the metric the harness uses
    if on_uint8:
        want = PytorchBatchedDistortion(metrics="psnr")(want_u8, img.cuda())["psnr"]
    else:
        want = PytorchBatchedDistortion(metrics="psnr")(want_f, K.image_u8_to_f32(img.cuda()))["psnr"]
    print("psnr", psnr[0], "want", float(want))
    assert abs(psnr[0] - float(want)) <= 1e-9 * max(1.0, abs(float(want))), (psnr[0], float(want))
    for bad in (dict(testing_tile_overlap=16), dict(testing_tile=64, testing_tile_overlap=33), dict(testing_tile=64, testing_tile_overlap=(0, -1))):
        with pytest.raises(ValueError):          # an overlap needs tiles, and at most half of one
            BasicLosslessCompressionBenchmark(codec, [img], **bad)
