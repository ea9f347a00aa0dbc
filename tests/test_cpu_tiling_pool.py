"""The planner of pooled tiles (utils.tiling.pool_tiles) and the refusals of the harness and tool switches that are raised before
anything touches a GPU.  The planner's contract: every tile of every picture exactly once; sizes in the order of their first
appearance, picture-major and tile-major within a size; chunks of at most max_batch; sum over the sizes of ceil(count / max_batch)
chunks."""
import os
import subprocess
import sys

import pytest

from cbench_basic_amd.utils.tiling import TileGrid, pool_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 150 x 200 and 160 x 224 in tiles of 64 are 3 x 4 tiles each, 96 x 64 is 2 x 1; with an overlap of 16 the steps are 48
SIZES = [(150, 200), (160, 224), (96, 64)]


def _grids(overlap):
    return [TileGrid(H, W, 64, 64, overlap) for H, W in SIZES]


def _expected(grids, max_batch):
    """The contract restated without the planner: (h, w) -> the (picture, tile, y0, x0) rows in picture- and tile-major order."""
    by_size = {}
    for p, g in enumerate(grids):
        for k in range(len(g)):
            y, x, h, w = g.tile_rect(k)
            by_size.setdefault((h, w), []).append((p, k, y, x))
    chunks = []
    for size, rows in by_size.items():
        step = max_batch or len(rows)
        chunks += [(size, rows[i:i + step]) for i in range(0, len(rows), step)]
    return by_size, chunks


@pytest.mark.parametrize("overlap", [0, 16, (16, 0)], ids=["abutting", "overlap16", "overlap16x0"])
@pytest.mark.parametrize("max_batch", [None, 0, 1, 5, 7, 1000])
def test_every_tile_once_in_the_stated_order(overlap, max_batch):
    grids = _grids(overlap)
    chunks = pool_tiles(grids, max_batch)
    by_size, want = _expected(grids, max_batch)
    # every tile of every picture exactly once, at its own origin and size
    seen = [(t.picture, t.index) for c in chunks for t in c.tiles]
    assert sorted(seen) == [(p, k) for p, g in enumerate(grids) for k in range(len(g))] and len(set(seen)) == len(seen)
    for c in chunks:
        assert c.tiles and (not max_batch or len(c.tiles) <= max_batch)
        for t in c.tiles:
            assert grids[t.picture].tile_rect(t.index) == (t.y0, t.x0, c.h, c.w)
    # the order and the number of chunks
    assert [((c.h, c.w), [tuple(t) for t in c.tiles]) for c in chunks] == want
    assert len(chunks) == sum(-(-len(rows) // (max_batch or len(rows))) for rows in by_size.values())
    first_seen = list(dict.fromkeys((c.h, c.w) for c in chunks))
    assert first_seen == list(by_size)                       # a size's chunks are consecutive, sizes by first appearance


def test_counts_of_the_three_pictures():
    # abutting: 150 x 200 -> 64x64 x6, 64x8 x2, 22x64 x3, 22x8; 160 x 224 -> 64x64 x6, 64x32 x2, 32x64 x3, 32x32; 96 x 64 -> 64x64, 32x64
    chunks = pool_tiles(_grids(0))
    assert [(c.h, c.w, len(c.tiles)) for c in chunks] == [(64, 64, 13), (64, 8, 2), (22, 64, 3), (22, 8, 1), (64, 32, 2), (32, 64, 4), (32, 32, 1)]
    assert len(pool_tiles(_grids(0), 5)) == 3 + 1 + 1 + 1 + 1 + 1 + 1
    assert len(pool_tiles(_grids(0), 1)) == 26


def test_single_picture_and_single_tile():
    g = TileGrid(150, 200, 64, 64)
    chunks = pool_tiles([g])
    assert [len(c.tiles) for c in chunks] == [len(grp.indices) for grp in g.groups()]        # one picture: its groups
    assert [[t.index for t in c.tiles] for c in chunks] == [list(grp.indices) for grp in g.groups()]
    one = pool_tiles([TileGrid(40, 50, 64, 64)], 3)
    assert len(one) == 1 and (one[0].h, one[0].w) == (40, 50) and [tuple(t) for t in one[0].tiles] == [(0, 0, 0, 0)]
    assert pool_tiles([]) == []
    for bad in (-1, 2.5, True, "3"):
        with pytest.raises(ValueError):
            pool_tiles([g], bad)


class _NoCodec:
    """Stands where a codec would: the refusals below are raised before a codec is asked for anything."""


def test_harness_refuses_the_pool_without_its_conditions():
    import torch
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark as B
    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="needs testing_tile"):
        B(_NoCodec(), [img], testing_tile_pool=3)
    with pytest.raises(ValueError):                                  # as today: tiles and coalesced items
        B(_NoCodec(), [img], testing_tile=64, testing_coalesce_items=4)
    with pytest.raises(ValueError):
        B(_NoCodec(), [img], testing_tile=64, testing_coalesce_items=4, testing_tile_pool=3)
    with pytest.raises(ValueError, match="testing_coalesce_items"):
        B(_NoCodec(), [img], testing_tile=64, testing_coalesce_items=2, testing_tile_pool=3)
    assert B(_NoCodec(), [img], testing_tile=64, testing_coalesce_items=1, testing_tile_pool=3).testing_tile_pool == 3   # 1: no coalescing
    with pytest.raises(ValueError):
        B(_NoCodec(), [img], testing_tile=64, testing_tile_pool=-1)
    with pytest.raises(ValueError, match="num_testing_workers"):      # the pooled pass runs on the calling thread
        B(_NoCodec(), [img], testing_tile=64, testing_tile_pool=2, num_testing_workers=2, codec_builder=_NoCodec)
    # items that are not [1, C, H, W]: refused when the pass reads the dataset, before any call of the codec
    for item in (torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(3, 8, 8, dtype=torch.uint8)):
        bench = B(_NoCodec(), [img, item], testing_tile=64, testing_tile_pool=2, force_testing_device=None)
        with pytest.raises(ValueError, match=r"\[1, C, H, W\]"):
            bench._run_dataset()
    assert B(_NoCodec(), [img], testing_tile=64, testing_tile_pool=3).testing_tile_pool == 3
    assert B(_NoCodec(), [img], testing_tile=64).testing_tile_pool == 0


def _tool(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_benchmark.py"), "--out", os.devnull, *argv],
                          capture_output=True, text=True, cwd=ROOT)


@pytest.mark.parametrize("argv,needle", [
    (["--tile-pool", "4"], "--tile-pool needs --tile"),
    (["--tile", "64", "--tile-pool", "-1"], "--tile-pool must be >= 0"),
    (["--tile", "64", "--tile-pool", "4", "--workers", "2"], "--workers"),
    (["--tile", "64", "--tile-pool", "4", "--coalesce", "4"], "--coalesce"),             # the existing refusal of --tile, unchanged
    (["--tile", "64", "--tile-pool", "4", "--batch-size", "2"], "--batch-size"),
], ids=["no-tile", "negative", "workers", "coalesce", "batch"])
def test_tool_refuses(argv, needle):
    r = _tool(*argv)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr)
