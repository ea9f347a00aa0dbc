"""Tiled pictures on the host (cbench_basic_amd/utils/tiling.py): the grid's groups cover every pixel exactly once in row-major tile
order, region queries find exactly the intersecting tiles, chunks of a group are regular grids again, and the container round-trips
and refuses everything that is not exactly one container.  No device, no torch."""
import itertools
import struct

import numpy as np
import pytest

from cbench_basic_amd.utils.tiling import MAGIC, TileGrid, pack_tiled, split_group, unpack_tiled

SIZES = range(1, 41)
TILES = list(itertools.product([1, 3, 8, 16], [1, 5, 16]))


def _tiles_of(group):
    """[(index, y, x, h, w)] of a group, in its own order."""
    return [(group.indices[i * group.nx + j], group.y0 + i * group.step_y, group.x0 + j * group.step_x, group.h, group.w)
            for i in range(group.ny) for j in range(group.nx)]


@pytest.mark.parametrize("th,tw", TILES)
def test_groups_cover_every_pixel_once_in_row_major_order(th, tw):
    for H in SIZES:
        for W in SIZES:
            grid = TileGrid(H, W, th, tw)
            assert (grid.rows, grid.cols) == (-(-H // th), -(-W // tw)) and len(grid) == grid.rows * grid.cols
            groups = grid.groups()
            assert 1 <= len(groups) <= 4
            cover = np.zeros((H, W), dtype=np.int32)
            seen = {}
            for g in groups:
                assert g.step_y >= g.h >= 1 and g.step_x >= g.w >= 1 and len(g.indices) == g.ny * g.nx
                for k, y, x, h, w in _tiles_of(g):
                    assert y + h <= H and x + w <= W
                    cover[y:y + h, x:x + w] += 1
                    assert k not in seen
                    seen[k] = (y, x, h, w)
            assert (cover == 1).all(), (H, W, th, tw)
            # tile k is the k-th tile in row-major order, as high and wide as the picture leaves it
            assert sorted(seen) == list(range(len(grid)))
            for k, rect in seen.items():
                i, j = divmod(k, grid.cols)
                assert rect == (i * th, j * tw, min(th, H - i * th), min(tw, W - j * tw)) == grid.tile_rect(k)
            assert len({(g.h, g.w) for g in groups}) == len(groups)     # one group per tile size


@pytest.mark.parametrize("th,tw", TILES)
def test_tiles_of_region_finds_exactly_the_intersecting_tiles(th, tw):
    rng = np.random.default_rng(th * 100 + tw)
    for H in SIZES:
        for W in SIZES:
            grid = TileGrid(H, W, th, tw)
            regions = [(0, 0, H, W), (H - 1, W - 1, H, W), (0, 0, 1, 1)]
            for _ in range(3):
                y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                regions.append((y0, x0, int(rng.integers(y0 + 1, H + 1)), int(rng.integers(x0 + 1, W + 1))))
            for (y0, x0, y1, x1) in regions:
                want = set()
                for k in range(len(grid)):
                    y, x, h, w = grid.tile_rect(k)
                    if y < y1 and y + h > y0 and x < x1 and x + w > x0:
                        want.add(k)
                got = []
                for g in grid.tiles_of_region(y0, x0, y1, x1):
                    for k, y, x, h, w in _tiles_of(g):
                        assert (y, x, h, w) == grid.tile_rect(k)
                        got.append(k)
                assert len(got) == len(set(got)) and set(got) == want, (H, W, th, tw, (y0, x0, y1, x1))


def test_region_outside_the_picture_or_empty_is_refused():
    grid = TileGrid(20, 30, 8, 8)
    for region in [(0, 0, 21, 30), (0, 0, 20, 31), (-1, 0, 5, 5), (0, -1, 5, 5), (5, 5, 5, 9), (5, 5, 9, 5), (9, 5, 5, 9), (20, 0, 21, 5)]:
        with pytest.raises(ValueError):
            grid.tiles_of_region(*region)
    for bad in [(0, 5, 1, 1), (5, 5, 0, 1), (5, 5, 1, -1), (5.0, 5, 1, 1)]:
        with pytest.raises(ValueError):
            TileGrid(*bad)


def test_split_group_gives_as_few_regular_sub_grids_as_any_shape_allows():
    for H, W, th, tw in [(40, 40, 8, 5), (37, 23, 8, 5), (16, 16, 16, 16), (33, 7, 3, 1), (64, 96, 8, 8)]:
        for g in TileGrid(H, W, th, tw).groups():
            assert split_group(g, None) == [g] and split_group(g, 0) == [g] and split_group(g, g.ny * g.nx) == [g]
            for m in [1, 2, 3, 5, 7, 33, 100]:
                subs = split_group(g, m)
                assert all(1 <= s.ny * s.nx <= m and len(s.indices) == s.ny * s.nx for s in subs)
                assert all((s.step_y, s.step_x, s.h, s.w) == (g.step_y, g.step_x, g.h, g.w) for s in subs)
                assert sorted(t for s in subs for t in _tiles_of(s)) == sorted(_tiles_of(g))      # the same tiles at the same places, once
                fewest = min(-(-g.ny // a) * -(-g.nx // b) for a in range(1, g.ny + 1) for b in range(1, g.nx + 1) if a * b <= m)
                assert len(subs) == fewest, (H, W, th, tw, m, len(subs), fewest)
    eight_by_twelve = TileGrid(64, 96, 8, 8).groups()[0]
    assert [(s.ny, s.nx) for s in split_group(eight_by_twelve, 33)] == [(8, 4)] * 3       # not four chunks of two whole rows
    assert [(s.ny, s.nx) for s in split_group(eight_by_twelve, 24)] == [(2, 12)] * 4      # whole rows where that is no worse
    with pytest.raises(ValueError):
        split_group(TileGrid(8, 8, 4, 4).groups()[0], -1)


def test_container_round_trip():
    rng = np.random.default_rng(0)
    grid = TileGrid(70, 100, 32, 32)
    strings = [b"", b"\x00", rng.bytes(100000)] + [rng.bytes(int(rng.integers(0, 300))) for _ in range(len(grid) - 3)]
    data = pack_tiled(3, 70, 100, 32, 32, strings)
    assert data[:4] == MAGIC == b"BTL1"
    assert len(data) == 4 + 1 + 5 * 4 + 4 * len(grid) + sum(len(s) for s in strings)
    assert struct.unpack_from("<BIIIII", data, 4) == (3, 70, 100, 32, 32, len(grid))
    assert struct.unpack_from("<%dI" % len(grid), data, 25) == tuple(len(s) for s in strings)
    assert unpack_tiled(data) == (3, 70, 100, 32, 32, strings)
    assert unpack_tiled(bytearray(data)) == (3, 70, 100, 32, 32, strings)
    assert unpack_tiled(pack_tiled(1, 1, 1, 7, 9, [b""])) == (1, 1, 1, 7, 9, [b""])
    with pytest.raises(ValueError):
        pack_tiled(3, 70, 100, 32, 32, strings[:-1])
    with pytest.raises(ValueError):
        pack_tiled(0, 70, 100, 32, 32, strings)


def test_malformed_containers_are_refused():
    strings = [b"abc", b"", b"defgh", b"i"]
    good = pack_tiled(3, 10, 12, 8, 8, strings)      # 2 x 2 tiles
    head = 25
    assert unpack_tiled(good)[5] == strings

    def field(offset, value, fmt="<I"):
        return good[:offset] + struct.pack(fmt, value) + good[offset + struct.calcsize(fmt):]
    bad = {
        "empty": b"",
        "wrong magic": b"BTL2" + good[4:],
        "magic only": good[:4],
        "truncated head": good[:head - 1],
        "truncated table": good[:head + 4 * 4 - 1],
        "head only": good[:head],
        "truncated payload": good[:-1],
        "table only": good[:head + 16],
        "trailing bytes": good + b"\x00",
        "n too small": field(21, 3),
        "n too large": field(21, 5),
        "n huge": field(21, 0xFFFFFFFF),
        "zero channels": field(4, 0, "<B"),
        "zero H": field(5, 0),
        "zero W": field(9, 0),
        "zero th": field(13, 0),
        "zero tw": field(17, 0),
        "other grid": field(13, 4),                   # th = 4: 3 x 2 tiles expected, 4 stated
        "length too long": field(head, 4),
        "length too short": field(head, 2),
    }
    for name, data in bad.items():
        with pytest.raises(ValueError):
            unpack_tiled(data)
            pytest.fail(name)
