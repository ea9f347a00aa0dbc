"""Overlapped tiles on the host (cbench_basic_amd/utils/tiling.py): the geometry by brute force over small sizes, overlap 0 against the
grid as it was, region queries, the BTL2 container, and the numpy reference of the blend (tests/tile_blend_exact.py) against its own
defining properties.  No device, no torch."""
import struct

import numpy as np
import pytest

import tile_blend_exact as E
from cbench_basic_amd.utils.tiling import MAGIC, MAGIC2, TileGrid, pack_tiled, split_group, unpack_tiled, unpack_tiled_any


def _tiles_of(group):
    return [(group.indices[i * group.nx + j], group.y0 + i * group.step_y, group.x0 + j * group.step_x, group.h, group.w)
            for i in range(group.ny) for j in range(group.nx)]


def test_one_axis_by_brute_force_for_every_small_size():
    """Every t < 40, o <= t / 2, L < 200: all samples covered, none more than twice, the doubly covered ones exactly the bands
    [(i + 1) * s, (i + 1) * s + o), the last tile longer than the overlap."""
    for t in range(1, 40):
        for o in range(0, t // 2 + 1):
            s = t - o
            for L in range(1, 200):
                grid = TileGrid(L, 1, t, 1, overlap=(o, 0))
                n = grid.rows
                assert n == max(1, -(-(L - o) // s)) and grid.cols == 1 and grid.sy == s
                cover = np.zeros(L, dtype=np.int32)
                for i in range(n):
                    y, x, h, w = grid.tile_rect(i)
                    assert (y, x, w) == (i * s, 0, 1) and h == min(t, L - y) and h >= 1
                    cover[y:y + h] += 1
                assert cover.min() >= 1 and cover.max() <= 2, (t, o, L)
                want = np.ones(L, dtype=np.int32)
                for i in range(n - 1):
                    want[(i + 1) * s:(i + 1) * s + o] += 1
                    assert (i + 1) * s + o <= L                          # a band lies inside the picture
                assert np.array_equal(cover, want), (t, o, L)
                if L > o:
                    assert grid.tile_rect(n - 1)[2] > o, (t, o, L)       # a last tile is longer than the overlap
                # the same numbers on the other axis
                other = TileGrid(1, L, 1, t, overlap=(0, o))
                assert (other.cols, other.sx) == (n, s) and [other.tile_rect(i)[1::2] for i in range(n)] == [grid.tile_rect(i)[0::2] for i in range(n)]


@pytest.mark.parametrize("th,tw,oy,ox", [(8, 16, 3, 8), (5, 4, 2, 0), (16, 3, 0, 1), (6, 6, 3, 3)])
def test_groups_are_at_most_four_and_hold_every_tile_once(th, tw, oy, ox):
    for H in range(1, 41):
        for W in range(1, 41):
            grid = TileGrid(H, W, th, tw, overlap=(oy, ox))
            groups = grid.groups()
            assert 1 <= len(groups) <= 4 and len({(g.h, g.w) for g in groups}) == len(groups)
            seen = {}
            for g in groups:
                assert (g.step_y, g.step_x) == (th - oy, tw - ox) and len(g.indices) == g.ny * g.nx
                for k, y, x, h, w in _tiles_of(g):
                    assert k not in seen
                    seen[k] = (y, x, h, w)
                for sub in split_group(g, 3):                            # chunks are regular grids of the same steps
                    assert (sub.step_y, sub.step_x, sub.h, sub.w) == (g.step_y, g.step_x, g.h, g.w)
                assert sorted(t for sub in split_group(g, 3) for t in _tiles_of(sub)) == sorted(_tiles_of(g))
            assert sorted(seen) == list(range(len(grid)))
            assert all(seen[k] == grid.tile_rect(k) for k in seen)


def test_overlap_zero_is_the_grid_as_it_was():
    for th, tw in [(1, 1), (3, 5), (8, 16), (16, 1)]:
        for H in range(1, 41):
            for W in range(1, 41, 3):
                old, new = TileGrid(H, W, th, tw), TileGrid(H, W, th, tw, overlap=(0, 0))
                assert (new.rows, new.cols, new.sy, new.sx, new.overlap) == (-(-H // th), -(-W // tw), th, tw, (0, 0))
                assert old.groups() == new.groups() == TileGrid(H, W, th, tw, overlap=0).groups()
                assert [old.tile_rect(k) for k in range(len(old))] == [(k // old.cols * th, k % old.cols * tw, min(th, H - k // old.cols * th),
                                                                        min(tw, W - k % old.cols * tw)) for k in range(len(old))]
                assert old.tiles_of_region(H // 2, W // 3, H, W) == list(old._groups(H // 2 // th, old.rows, W // 3 // tw, old.cols))


@pytest.mark.parametrize("th,tw,oy,ox", [(8, 16, 3, 8), (5, 4, 2, 0), (16, 3, 0, 1), (6, 6, 3, 3), (8, 8, 0, 0)])
def test_tiles_of_region_finds_every_tile_that_covers_a_sample(th, tw, oy, ox):
    rng = np.random.default_rng(th * 100 + tw)
    for H in range(1, 41, 2):
        for W in range(1, 41):
            grid = TileGrid(H, W, th, tw, overlap=(oy, ox))
            regions = [(0, 0, H, W), (H - 1, W - 1, H, W), (0, 0, 1, 1)]
            for _ in range(4):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                regions.append((y0, x0, int(rng.integers(y0 + 1, H + 1)), int(rng.integers(x0 + 1, W + 1))))
            for (y0, x0, y1, x1) in regions:
                want = {k for k in range(len(grid)) for y, x, h, w in [grid.tile_rect(k)] if y < y1 and y + h > y0 and x < x1 and x + w > x0}
                got = [k for g in grid.tiles_of_region(y0, x0, y1, x1) for k, *rect in _tiles_of(g) if tuple(rect) == grid.tile_rect(k)]
                assert len(got) == len(set(got)) and set(got) == want, (H, W, th, tw, oy, ox, (y0, x0, y1, x1))
    with pytest.raises(ValueError):
        TileGrid(20, 30, 8, 8, overlap=(2, 2)).tiles_of_region(0, 0, 21, 30)


def test_overlaps_that_are_refused():
    for bad in [(5, 0), (0, 5), (-1, 0), (0, -1), (1.0, 0), (True, 0), (1, 2, 3)]:
        with pytest.raises(ValueError):
            TileGrid(20, 30, 8, 8, overlap=bad)
    with pytest.raises(ValueError):
        TileGrid(20, 30, 8, 8, overlap=-1)
    with pytest.raises(ValueError):
        TileGrid(20, 30, 9, 9, overlap=5)
    assert TileGrid(20, 30, 8, 8, overlap=4).overlap == (4, 4)           # exactly half is allowed
    with pytest.raises(ValueError):
        pack_tiled(3, 20, 30, 8, 8, [b""] * 100, overlap=(5, 0))


def test_btl2_round_trip_and_overlap_zero_is_btl1_byte_for_byte():
    rng = np.random.default_rng(1)
    grid = TileGrid(70, 100, 32, 32, overlap=(8, 5))
    assert (grid.rows, grid.cols) == (3, 4)
    strings = [b"", b"\x00", rng.bytes(70000)] + [rng.bytes(int(rng.integers(0, 300))) for _ in range(len(grid) - 3)]
    data = pack_tiled(3, 70, 100, 32, 32, strings, overlap=(8, 5))
    assert data[:4] == MAGIC2 == b"BTL2"
    assert len(data) == 4 + 1 + 7 * 4 + 4 * len(grid) + sum(len(s) for s in strings)
    assert struct.unpack_from("<BIIIIIII", data, 4) == (3, 70, 100, 32, 32, 8, 5, len(grid))
    assert struct.unpack_from("<%dI" % len(grid), data, 33) == tuple(len(s) for s in strings)
    assert unpack_tiled_any(data) == (3, 70, 100, 32, 32, (8, 5), strings) == unpack_tiled_any(bytearray(data))
    with pytest.raises(ValueError):
        unpack_tiled(data)                                               # the BTL1 reader keeps refusing every other magic
    with pytest.raises(ValueError):
        pack_tiled(3, 70, 100, 32, 32, strings[:-1], overlap=(8, 5))
    # overlap 0, however it is spelt, is the container as it was
    plain = TileGrid(70, 100, 32, 32)
    old = pack_tiled(3, 70, 100, 32, 32, strings[:len(plain)])
    assert old[:4] == MAGIC == b"BTL1" and len(old) == 25 + 4 * len(plain) + sum(len(s) for s in strings[:len(plain)])
    assert old == pack_tiled(3, 70, 100, 32, 32, strings[:len(plain)], overlap=(0, 0)) == pack_tiled(3, 70, 100, 32, 32, strings[:len(plain)], overlap=0)
    assert unpack_tiled_any(old) == (3, 70, 100, 32, 32, (0, 0), strings[:len(plain)])
    assert unpack_tiled(old) == (3, 70, 100, 32, 32, strings[:len(plain)])


def test_malformed_btl2_containers_are_refused():
    strings = [b"abc", b"", b"defgh", b"i", b"jk", b"l"]
    good = pack_tiled(3, 10, 14, 8, 8, strings, overlap=(2, 3))      # rows = ceil(8 / 6) = 2, cols = ceil(11 / 5) = 3
    head = 33
    assert unpack_tiled_any(good)[5:] == ((2, 3), strings)

    def field(offset, value, fmt="<I"):
        return good[:offset] + struct.pack(fmt, value) + good[offset + struct.calcsize(fmt):]
    bad = {
        "empty": b"",
        "wrong magic": b"BTL3" + good[4:],
        "BTL1 magic on a BTL2 body": b"BTL1" + good[4:],
        "magic only": good[:4],
        "truncated head": good[:head - 1],
        "truncated table": good[:head + 4 * 6 - 1],
        "head only": good[:head],
        "truncated payload": good[:-1],
        "table only": good[:head + 24],
        "trailing bytes": good + b"\x00",
        "n too small": field(29, 5),
        "n too large": field(29, 7),
        "n huge": field(29, 0xFFFFFFFF),
        "zero channels": field(4, 0, "<B"),
        "zero H": field(5, 0),
        "zero W": field(9, 0),
        "zero th": field(13, 0),
        "zero tw": field(17, 0),
        "other grid": field(25, 0),                   # ox = 0: 2 x 2 tiles expected, 6 stated
        "oy above half a tile": field(21, 5),
        "ox above half a tile": field(25, 5),
        "oy huge": field(21, 0xFFFFFFFF),
        "length too long": field(head, 4),
        "length too short": field(head, 2),
    }
    for name, data in bad.items():
        with pytest.raises(ValueError):
            unpack_tiled_any(data)
            pytest.fail(name)


def test_the_ramp_rises_strictly_inside_zero_and_one():
    for o in range(1, 300):
        r = E.ramp(o)
        assert r.dtype == np.float32 and r.shape == (o,) and 0 < r[0] and r[-1] < 1 and bool((np.diff(r) > 0).all())
        assert r[0] == np.float32(1 / (2.0 * o))
    assert E.ramp(0).shape == (0,)
    assert np.array_equal(E.ramp(2), np.array([0.25, 0.75], dtype=np.float32))


GRIDS = [(70, 100, 32, 32, 8, 8), (71, 102, 32, 32, 5, 5), (70, 100, 32, 32, 16, 16), (70, 100, 32, 32, 0, 8), (70, 100, 32, 32, 8, 0),
         (20, 100, 32, 32, 8, 8), (70, 20, 32, 32, 8, 8)]


@pytest.mark.parametrize("H,W,th,tw,oy,ox", GRIDS)
def test_reference_agreeing_tiles_give_that_value_exactly(H, W, th, tw, oy, ox):
    grid = TileGrid(H, W, th, tw, overlap=(oy, ox))
    rng = np.random.default_rng(H + W + oy)
    pic = (rng.random((3, H, W), dtype=np.float32) * np.float32(3) - np.float32(1)).astype(np.float32)
    pic[0, ::3, ::5] = E.TIES[np.arange(pic[0, ::3, ::5].size) % 255].reshape(pic[0, ::3, ::5].shape)
    tiles = {}
    for k in range(len(grid)):
        y, x, h, w = grid.tile_rect(k)
        tiles[k] = np.pad(pic[:, y:y + h, x:x + w], ((0, 0), (0, k % 3), (0, k % 2)), constant_values=np.nan)      # padding is never read
    assert np.array_equal(E.blend(grid, tiles).view(np.int32), pic.view(np.int32))
    # and where they differ, a band sample lies between its two tiles (one axis, finite values)
    if oy == 0 and ox:
        tiles2 = {k: np.full_like(t, float(k % grid.cols)) for k, t in tiles.items()}
        out = E.blend(grid, tiles2)
        for j in range(1, grid.cols):
            band = out[:, :, j * grid.sx:j * grid.sx + ox]
            assert bool((band > j - 1).all()) and bool((band < j).all()) and bool((np.diff(band, axis=2) > 0).all())
            assert np.array_equal(band[0, 0], np.float32(j - 1) + E.ramp(ox))


@pytest.mark.parametrize("H,W,th,tw", [(70, 100, 32, 32), (71, 102, 32, 32), (5, 7, 8, 8)])
def test_reference_overlap_zero_is_the_plain_paste(H, W, th, tw):
    grid = TileGrid(H, W, th, tw)
    _, tiles = E.sources(grid, 3)
    a, b = E.blend(grid, tiles), E.paste(grid, tiles)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int32), b[~np.isnan(b)].view(np.int32))
    assert np.array_equal(E.quantise(a), E.quantise(b))


def test_reference_two_axes_go_x_first_and_the_sources_carry_ties_through_bands():
    grid = TileGrid(70, 100, 32, 32, overlap=(8, 8))
    batches, tiles = E.sources(grid, 3)
    assert len(batches) == 4 and len({b.shape[2:] for b, _ in batches}) == 4 and sorted(k for _, ks in batches for k in ks) == list(range(12))
    out = E.blend(grid, tiles)
    # one corner sample, operation by operation: tiles 0, 1 (top) and 4, 5 (bottom) around (24 + 3, 24 + 5)
    y, x, dy, dx = 27, 29, 3, 5
    wx, wy = np.float32((2 * dx + 1) / 16.0), np.float32((2 * dy + 1) / 16.0)
    for c in range(3):
        r00, r01, r10, r11 = tiles[0][c, y, x], tiles[1][c, y, dx], tiles[4][c, dy, x], tiles[5][c, dy, dx]
        top = np.float32(r00 + np.float32(wx * np.float32(r01 - r00)))
        bottom = np.float32(r10 + np.float32(wx * np.float32(r11 - r10)))
        want = np.float32(top + np.float32(wy * np.float32(bottom - top)))
        assert (np.isnan(want) and np.isnan(out[c, y, x])) or want == out[c, y, x]
    assert E.ties_in_bands(grid, out) >= 200
    kept = out[:, E.band_mask(grid)]
    assert bool(np.isnan(kept).any()) and bool((kept < 0).any()) and bool((kept > 1).any())
    assert np.array_equal(E.quantise(np.array([np.nan, np.inf, -np.inf, -1.0, 2.0, 0.5], dtype=np.float32)), np.array([0, 255, 0, 0, 255, 128], dtype=np.uint8))


@pytest.mark.parametrize("argv,word", [(["--tile-overlap", "16"], "needs --tile"), (["--tile", "64", "--tile-overlap", "33"], "half a tile"),
                                       (["--tile", "64", "32", "--tile-overlap", "8", "17"], "half a tile"),
                                       (["--tile", "64", "--tile-overlap", "-1"], "not negative"),
                                       (["--tile", "64", "--tile-overlap", "1", "2", "3"], "OY [OX]")])
def test_tool_refuses_an_overlap_without_tiles_or_above_half_a_tile(argv, word, monkeypatch, capsys):
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
    assert e.value.code == 2 and "--tile-overlap" in err and word in err, err


def test_harness_refuses_an_overlap_without_tiles():
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark
    for bad in (dict(testing_tile_overlap=16), dict(testing_tile=64, testing_tile_overlap=33), dict(testing_tile=(64, 32), testing_tile_overlap=(8, 17)),
                dict(testing_tile=64, testing_tile_overlap=(0, -1)), dict(testing_tile=64, testing_tile_overlap=(1, 2, 3))):
        with pytest.raises(ValueError):
            BasicLosslessCompressionBenchmark(object(), [], force_testing_device=None, **bad)
    bench = BasicLosslessCompressionBenchmark(object(), [], force_testing_device=None, testing_tile=64, testing_tile_overlap=32)
    assert bench.testing_tile_overlap == (32, 32) and BasicLosslessCompressionBenchmark(object(), [], force_testing_device=None).testing_tile_overlap == (0, 0)
