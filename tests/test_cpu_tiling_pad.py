"""Edge-padded tiles on the host (cbench_basic_amd/utils/tiling.py, ``pad_to``): the coded sizes, the refusals, the BTL3 container, the
planner's counts, and that ``pad_to=(1, 1)`` changes nothing.  No device."""
import itertools
import struct

import pytest

from cbench_basic_amd.utils import tiling
from cbench_basic_amd.utils.tiling import TileGrid, pack_tiled, pool_tiles, unpack_tiled, unpack_tiled_any, unpack_tiled_full

import tile_pad_exact as E

SWEEP = [(H, W, t, o, p) for (H, W), (t, o), p in itertools.product(
    [(1, 1), (7, 5), (16, 24), (17, 23), (70, 100), (64, 64), (130, 50), (33, 97)],
    [((16, 16), 0), ((16, 24), (4, 8)), ((64, 64), 0), ((64, 64), 16), ((8, 12), (0, 6))],
    [1, 2, (4, 4), (8, 4), (16, 1)]) if t[0] % (p if isinstance(p, int) else p[0]) == 0 and t[1] % (p if isinstance(p, int) else p[1]) == 0]


def test_coded_size_is_the_valid_size_rounded_up_and_the_geometry_does_not_move():
    assert len(SWEEP) > 100
    for H, W, (th, tw), overlap, pad in SWEEP:
        py, px = (pad, pad) if isinstance(pad, int) else pad
        plain, grid = TileGrid(H, W, th, tw, overlap=overlap), TileGrid(H, W, th, tw, overlap=overlap, pad_to=pad)
        assert grid.pad_to == (py, px) and (grid.py, grid.px) == (py, px)
        assert (grid.rows, grid.cols, len(grid)) == (plain.rows, plain.cols, len(plain))
        assert grid.groups() == plain.groups()
        assert grid.tiles_of_region(0, 0, H, W) == plain.tiles_of_region(0, 0, H, W)
        assert grid.tiles_of_region(H - 1, W - 1, H, W) == plain.tiles_of_region(H - 1, W - 1, H, W)
        for k in range(len(grid)):
            y, x, h, w = grid.tile_rect(k)
            assert (y, x, h, w) == plain.tile_rect(k)
            ph, pw = grid.coded_size(k)
            assert (ph, pw) == E.coded_size(h, w, py, px)
            assert h <= ph <= th and w <= pw <= tw and ph % py == 0 and pw % px == 0 and ph - h < py and pw - w < px
            assert plain.coded_size(k) == (h, w)
        with pytest.raises(IndexError):
            grid.coded_size(len(grid))
    full = TileGrid(70, 100, 64, 64, pad_to=64)
    assert {full.coded_size(k) for k in range(len(full))} == {(64, 64)}


@pytest.mark.parametrize("pad", [0, -1, (0, 4), (4, 0), (4,), (4, 4, 4), 2.0, (4, 2.0), True, None, "4", 3, (16, 5), (32, 16), 128])
def test_refusals(pad):
    with pytest.raises(ValueError):
        TileGrid(70, 100, 16, 16, pad_to=pad)
    with pytest.raises(ValueError):
        pack_tiled(3, 70, 100, 16, 16, [b""] * 35, pad_to=pad)


def test_pad_to_one_changes_nothing():
    for H, W, th, tw, overlap in [(70, 100, 64, 64, 0), (70, 100, 32, 48, (8, 16)), (64, 64, 64, 64, 0), (130, 50, 64, 64, 32)]:
        a, b, c = TileGrid(H, W, th, tw, overlap), TileGrid(H, W, th, tw, overlap, pad_to=1), TileGrid(H, W, th, tw, overlap, pad_to=(1, 1))
        assert a.pad_to == b.pad_to == c.pad_to == (1, 1)
        assert a.groups() == b.groups() == c.groups()
        strings = [bytes([k]) * (k + 1) for k in range(len(a))]
        want = pack_tiled(3, H, W, th, tw, strings, overlap=overlap)
        assert want[:4] in (b"BTL1", b"BTL2")
        assert pack_tiled(3, H, W, th, tw, strings, overlap=overlap, pad_to=1) == want
        assert pack_tiled(3, H, W, th, tw, strings, overlap=overlap, pad_to=(1, 1)) == want
        full = unpack_tiled_full(want)
        assert tuple(full) == (3, H, W, th, tw, a.overlap, (1, 1), strings)
        assert unpack_tiled_any(want) == (3, H, W, th, tw, a.overlap, strings)
    grids = [TileGrid(H, W, 64, 64) for H, W in PICTURES]
    same = [TileGrid(H, W, 64, 64, pad_to=(1, 1)) for H, W in PICTURES]
    for max_batch in (None, 1, 3):
        assert pool_tiles(grids, max_batch) == pool_tiles(same, max_batch)


def test_btl3_round_trip():
    for H, W, th, tw, overlap, pad in [(70, 100, 64, 64, 0, 64), (70, 100, 64, 64, 16, (32, 64)), (500, 750, 256, 128, (0, 64), (64, 64)),
                                       (5, 5, 8, 8, 0, (2, 4))]:
        grid = TileGrid(H, W, th, tw, overlap, pad)
        strings = [bytes([k % 251]) * (3 * k % 17) for k in range(len(grid))]
        data = pack_tiled(4, H, W, th, tw, strings, overlap=overlap, pad_to=pad)
        assert data[:4] == b"BTL3"
        head = struct.unpack_from("<4sBIIIIIIIII", data)
        assert struct.calcsize("<4sBIIIIIIIII") == 41
        assert head == (b"BTL3", 4, H, W, th, tw, grid.oy, grid.ox, grid.py, grid.px, len(grid))
        assert data[41:41 + 4 * len(grid)] == struct.pack("<%dI" % len(grid), *[len(s) for s in strings])
        assert data[41 + 4 * len(grid):] == b"".join(strings)
        full = unpack_tiled_full(data)
        assert isinstance(full, tuple) and full.pad_to == grid.pad_to and full.overlap == grid.overlap
        assert (full.channels, full.H, full.W, full.th, full.tw, full.strings) == (4, H, W, th, tw, strings)
        assert unpack_tiled_full(bytearray(data)) == full and unpack_tiled_full(memoryview(data)) == full
        for reader in (unpack_tiled_any, unpack_tiled):          # the readers of BTL1 / BTL2 keep refusing anything else
            with pytest.raises(ValueError, match="wrong magic"):
                reader(data)


def _head3(channels=3, H=70, W=100, th=64, tw=64, oy=0, ox=0, py=64, px=64, n=4, magic=b"BTL3"):
    return struct.pack("<4sBIIIIIIIII", magic, channels, H, W, th, tw, oy, ox, py, px, n)


def test_unpack_tiled_full_refuses_what_is_not_exactly_a_container():
    body = struct.pack("<4I", 1, 2, 0, 3) + b"a" + b"bb" + b"ccc"
    good = _head3() + body
    assert unpack_tiled_full(good).strings == [b"a", b"bb", b"", b"ccc"]
    bad = {
        "magic": _head3(magic=b"BTL4") + body, "empty": b"", "short magic": b"BTL",
        "head cut short": good[:40], "channels 0": _head3(channels=0) + body, "H 0": _head3(H=0) + body, "W 0": _head3(W=0) + body,
        "th 0": _head3(th=0) + body, "tw 0": _head3(tw=0) + body,
        "overlap": _head3(oy=33) + body, "overlap x": _head3(ox=40) + body,
        "py 0": _head3(py=0) + body, "px 0": _head3(px=0) + body, "py does not divide": _head3(py=48) + body, "px does not divide": _head3(px=128) + body,
        "tile count": _head3(n=5) + body, "lengths cut short": good[:41 + 15], "payload cut short": good[:-1], "bytes after": good + b"x",
    }
    for name, data in bad.items():
        with pytest.raises(ValueError):
            unpack_tiled_full(data)
            pytest.fail(name)
    # the refusals of the older containers hold through the new reader
    old = pack_tiled(3, 70, 100, 64, 64, [b"a", b"bb", b"", b"ccc"])
    for data in (old[:-1], old + b"x", old[:20], b"BTL0" + old[4:]):
        with pytest.raises(ValueError):
            unpack_tiled_full(data)


PICTURES = [(70, 100), (64, 64), (130, 50)]


def test_planner_counts():
    def plan(pad, max_batch=None):
        grids = [TileGrid(H, W, 64, 64) if pad is None else TileGrid(H, W, 64, 64, pad_to=pad) for H, W in PICTURES]
        chunks = pool_tiles(grids, max_batch)
        tiles = sorted((t.picture, t.index) for c in chunks for t in c.tiles)
        assert tiles == [(p, k) for p, g in enumerate(grids) for k in range(len(g))]      # every tile once
        for c in chunks:
            for t in c.tiles:
                assert grids[t.picture].coded_size(t.index) == (c.h, c.w) and grids[t.picture].tile_rect(t.index)[:2] == (t.y0, t.x0)
        return chunks
    none = plan(None)
    assert len(none) == 6 and len({(c.h, c.w) for c in none}) == 6 and sum(len(c.tiles) for c in none) == 8
    assert [(c.h, c.w) for c in none] == [(64, 64), (64, 36), (6, 64), (6, 36), (64, 50), (2, 50)]
    half = plan((32, 32))
    assert [(c.h, c.w, len(c.tiles)) for c in half] == [(64, 64, 5), (32, 64, 3)]
    assert [(t.picture, t.index) for t in half[0].tiles] == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)]
    assert [(t.picture, t.index) for t in half[1].tiles] == [(0, 2), (0, 3), (2, 2)]
    full = plan((64, 64))
    assert [(c.h, c.w, len(c.tiles)) for c in full] == [(64, 64, 8)]
    assert [(c.h, c.w, len(c.tiles)) for c in plan(64, 3)] == [(64, 64, 3), (64, 64, 3), (64, 64, 2)]
    assert [(c.h, c.w, len(c.tiles)) for c in plan(32, 2)] == [(64, 64, 2), (64, 64, 2), (64, 64, 1), (32, 64, 2), (32, 64, 1)]


def test_restated_padded_tile_and_clipped_paste():
    """The numpy restatement the GPU tests lean on, against a plain loop over the formula."""
    import numpy as np
    rng = np.random.default_rng(5)
    pic = rng.integers(0, 256, (3, 12, 18), dtype=np.uint8)
    for y, x, ph, pw in [(0, 0, 16, 16), (8, 16, 16, 16), (11, 17, 4, 8), (0, 0, 12, 18), (3, 5, 7, 9)]:
        got = E.padded_tile(pic, y, x, ph, pw)
        assert got.dtype == np.float32 and got.shape == (3, ph, pw)
        for c, r, q in itertools.product(range(3), range(ph), range(pw)):
            assert got[c, r, q] == np.float32(pic[c, min(y + r, 11), min(x + q, 17)]) / np.float32(255)
        src = (rng.random((3, ph + 2, pw + 3), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)
        src[0, 0, 0], src[1, 0, 1], src[2, 1, 0] = np.nan, np.inf, -np.inf
        canvas = np.full((3, 12, 18), 0xAB, dtype=np.uint8)
        E.clipped_paste(canvas, src, y, x, ph, pw)
        for c, r, q in itertools.product(range(3), range(12), range(18)):
            inside = y <= r < y + ph and x <= q < x + pw
            v = src[c, r - y, q - x] if inside else None
            want = 0xAB if not inside else 0 if np.isnan(v) else int(np.rint(np.float32(min(max(v, np.float32(0)), np.float32(1))) * np.float32(255)))
            assert canvas[c, r, q] == want
    assert tiling.MAGIC3 == b"BTL3"


@pytest.mark.parametrize("argv,word", [(["--tile-pad", "64"], "needs --tile"), (["--tile", "64", "--tile-pad", "48"], "divide the tile"),
                                       (["--tile", "64", "32", "--tile-pad", "32", "64"], "divide the tile"),
                                       (["--tile", "64", "--tile-pad", "0"], "positive"),
                                       (["--tile", "64", "--tile-pad", "1", "2", "4"], "PY [PX]")])
def test_tool_refuses_a_padding_without_tiles_or_one_that_does_not_divide_the_tile(argv, word, monkeypatch, capsys):
    import importlib.util
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "run_benchmark.py")
    spec = importlib.util.spec_from_file_location("run_benchmark_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["run_benchmark.py", "--out", "unused"] + argv)
    with pytest.raises(SystemExit) as e:
        tool.main()
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--tile-pad" in err and word in err, err


def test_harness_refuses_a_padding_without_tiles_or_one_that_does_not_divide_the_tile():
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark
    for kw in (dict(testing_tile_pad=64), dict(testing_tile=64, testing_tile_pad=48), dict(testing_tile=(64, 32), testing_tile_pad=(32, 64)),
               dict(testing_tile=64, testing_tile_pad=0), dict(testing_tile=64, testing_tile_pad=(32, 32, 32))):
        with pytest.raises(ValueError, match="testing_tile_pad"):
            BasicLosslessCompressionBenchmark(None, [], **kw)
    assert BasicLosslessCompressionBenchmark(None, [], testing_tile=(64, 32), testing_tile_pad=(32, 16)).testing_tile_pad == (32, 16)
    assert BasicLosslessCompressionBenchmark(None, [], testing_tile=64, testing_tile_pad=32, testing_tile_overlap=16).testing_tile_pad == (32, 32)
    assert BasicLosslessCompressionBenchmark(None, [], testing_tile=64).testing_tile_pad is None
