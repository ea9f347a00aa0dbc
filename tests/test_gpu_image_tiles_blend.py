"""The blend of overlapped tiles and their cut (csrc/image.hip, include/basic_hip.h section 8c) through the raw C ABI, against the numpy
reference of tests/tile_blend_exact.py: the float picture bit for bit (NaN where the reference has NaN), the 8-bit picture exactly,
for both layouts, both output kinds and both paths (wide / sample by sample; which one a call took is asserted), with guard bands of
a sentinel around every output and the sources left as they were.  The source tiles carry uniform values beyond [0, 1], every
rounding tie, NaN and +-inf, differ in sh x sw inside one table, and agree over patches so that ties pass bands unchanged."""
import functools

import numpy as np
import pytest
import torch

import tile_blend_exact as E
from cbench_basic_amd.utils.tiling import TileGrid

pytestmark = pytest.mark.gpu

LAYOUTS = ["chw", "hwc"]
CHANNELS = [1, 2, 3, 4]
KINDS = ["u8", "f32"]
GUARD = 64            # elements of sentinel on either side of an output; a multiple of 4, so an offset of 0 keeps the wide path
SENTINEL_U, SENTINEL_F = 0xA5, -7.5
ENTRY = np.dtype([("src", "<u8"), ("sh", "<i4"), ("sw", "<i4")])      # basic_tile_source

# (H, W, tile, oy, ox)
MAIN = (70, 100, 32, 8, 8)          # tiles 32 / 32 / 22 by 32 / 32 / 32 / 28, all four groups; every width a multiple of 4: wide
ODD = (71, 102, 32, 5, 5)           # nothing a multiple of 4: sample by sample
HALF = (70, 100, 32, 16, 16)        # the maximum: every sample off the picture's rim in a band
GRIDS = [MAIN, ODD, HALF, (70, 100, 32, 0, 8), (70, 100, 32, 8, 0), (20, 100, 32, 8, 8), (70, 20, 32, 8, 8)]


def _grid(spec):
    H, W, t, oy, ox = spec
    return TileGrid(H, W, t, t, overlap=(oy, ox))


@functools.lru_cache(maxsize=None)
def _case(spec, C):
    """Computed once per grid and channel count and left unchanged: (grid, host batches, device batches, the reference picture)."""
    grid = _grid(spec)
    batches, tiles = E.sources(grid, C)
    full = E.blend(grid, tiles)
    full.setflags(write=False)
    dev = [torch.from_numpy(b).cuda() for b, _ in batches]
    return grid, batches, dev, full


def _table(grid, batches, dev, null=()):
    """The device table of a grid's sources, the entries of `null` (and of tiles no batch holds) zero."""
    table = np.zeros(len(grid), dtype=ENTRY)
    for (b, indices), d in zip(batches, dev):
        n, C, sh, sw = b.shape
        for t, k in enumerate(indices):
            if k not in null:
                table[k] = (d.data_ptr() + 4 * t * C * sh * sw, sh, sw)
    return torch.from_numpy(table.view(np.uint8)).cuda()


def _expect_wide(grid, C, layout, off, rx0, rw):
    """The rule of section 8c; `off` in elements of the output: a uint8 base must be 4-byte, a float32 base 16-byte aligned."""
    ok = off % 4 == 0 and rw % 4 == 0 and rx0 % 4 == 0 and grid.sx % 4 == 0 and grid.ox % 4 == 0
    return int(ok and (layout == "chw" or C in (1, 3, 4)))


def _blend_raw(L, table_ptr, grid, C, region, out_ptr, kind, layout):
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    y0, x0, y1, x1 = region
    return L.basic_image_tiles_blend_dev(table_ptr, grid.H, grid.W, grid.th, grid.tw, grid.oy, grid.ox, C, y0, x0, y1 - y0, x1 - x0, out_ptr,
                                         {"u8": _lib.PIXEL_U8, "f32": _lib.PIXEL_F32}.get(kind, kind),
                                         K.IMAGE_LAYOUTS[layout] if isinstance(layout, str) else layout, torch.cuda.current_stream().cuda_stream)


def _needs(grid, region, null):
    """[rh, rw] bool: the samples of the region that a tile of `null` covers."""
    y0, x0, y1, x1 = region
    m = np.zeros((grid.H, grid.W), dtype=bool)
    for k in null:
        y, x, h, w = grid.tile_rect(k)
        m[y:y + h, x:x + w] = True
    return m[y0:y1, x0:x1]


def _check_blend(spec, C, layout, kind, region=None, off=0, null=(), only_needed=False, want_path=None):
    """One launch into a guarded buffer whose picture starts `off` elements in; -> the picture written, [C, rh, rw]."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    L = _lib.lib()
    grid, batches, dev, full = _case(spec, C)
    region = (0, 0, grid.H, grid.W) if region is None else region
    y0, x0, y1, x1 = region
    rh, rw = y1 - y0, x1 - x0
    needed = {k for g in grid.tiles_of_region(*region) for k in g.indices}
    absent = set(null) | (set(range(len(grid))) - needed if only_needed else set())
    table = _table(grid, batches, dev, absent)
    n = C * rh * rw
    torch_dtype, sentinel = (torch.uint8, SENTINEL_U) if kind == "u8" else (torch.float32, SENTINEL_F)
    big = torch.full((GUARD + off + n + GUARD,), sentinel, dtype=torch_dtype, device="cuda")
    _lib.check(_blend_raw(L, table.data_ptr(), grid, C, region, big[GUARD + off:].data_ptr(), kind, layout))
    path = K.image_tiles_last_path()
    assert path == _expect_wide(grid, C, layout, off, x0, rw), (spec, C, layout, kind, region, off, path)
    if want_path is not None:
        assert path == want_path, (spec, C, layout, kind, region, off)
    got = big.cpu().numpy()
    assert (got[:GUARD + off] == sentinel).all() and (got[GUARD + off + n:] == sentinel).all(), "guard bands"
    flat = got[GUARD + off:GUARD + off + n]
    pic = flat.reshape(C, rh, rw) if layout == "chw" else flat.reshape(rh, rw, C).transpose(2, 0, 1)
    want = full[:, y0:y1, x0:x1]
    keep = np.broadcast_to(_needs(grid, region, set(null) & needed), pic.shape)      # these keep the sentinel
    assert (pic[keep] == sentinel).all(), (spec, C, layout, kind, region, off, "a sample that needs a missing tile was written")
    if kind == "u8":
        assert np.array_equal(pic[~keep], E.quantise(want)[~keep]), (spec, C, layout, kind, region, off)
    else:
        a, b = pic[~keep], want[~keep]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (spec, C, layout, kind, region, off, "NaN positions")
        assert np.array_equal(a[~np.isnan(a)].view(np.int32), b[~np.isnan(b)].view(np.int32)), (spec, C, layout, kind, region, off)      # bit for bit
    for (b, _), d in zip(batches, dev):      # the sources are only read
        assert np.array_equal(d.cpu().numpy().view(np.int32), b.view(np.int32))
    return pic


def test_the_cases_reach_what_they_are_meant_to():
    grid, batches, _, full = _case(MAIN, 3)
    assert (grid.rows, grid.cols) == (3, 4) and len(grid.groups()) == 4
    assert [grid.tile_rect(k)[2] for k in (0, 4, 8)] == [32, 32, 22] and [grid.tile_rect(k)[3] for k in range(4)] == [32, 32, 32, 28]
    assert len({b.shape[2:] for b, _ in batches}) == 4                       # sh x sw differs inside one table
    assert any(b.shape[2:] == (g.h, g.w) for (b, _), g in zip(batches, grid.groups()))      # one group without padding
    for spec in (MAIN, ODD, HALF):
        for C in CHANNELS:
            g, _, _, pic = _case(spec, C)
            assert E.ties_in_bands(g, pic) >= 200, (spec, C)                 # ties reach the quantiser inside bands
            kept = pic[:, E.band_mask(g)]
            assert np.isnan(kept).any() and (kept < 0).any() and (kept > 1).any()
    half = _grid(HALF)
    assert E.band_mask(half)[16:, 16:96].all() and E.band_mask(half)[16:64, 16:].all()      # every sample in a band, but for the picture's rim
    assert (_grid(GRIDS[5]).rows, _grid(GRIDS[6]).cols) == (1, 1)             # a single row, a single column of tiles


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_blend_whole_picture_every_grid(C, layout, kind):
    can_go_wide = int(layout == "chw" or C != 2)
    for spec in GRIDS:
        want_path = 0 if spec == ODD else can_go_wide
        _check_blend(spec, C, layout, kind, want_path=want_path)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_wide_and_scalar_agree_and_a_moved_base_goes_scalar(C, layout, kind):
    can_go_wide = int(layout == "chw" or C != 2)
    for spec in (MAIN, HALF):
        wide = _check_blend(spec, C, layout, kind, off=0, want_path=can_go_wide)
        for off in (1, 2, 3):      # uint8: 1-3 bytes; float32: 1-3 floats, no longer 16-byte aligned
            scalar = _check_blend(spec, C, layout, kind, off=off, want_path=0)
            assert np.array_equal(wide.view(np.uint8 if kind == "u8" else np.int32), scalar.view(np.uint8 if kind == "u8" else np.int32))
        assert np.array_equal(_check_blend(spec, C, layout, kind, off=4, want_path=can_go_wide).view(np.uint8 if kind == "u8" else np.int32),
                              wide.view(np.uint8 if kind == "u8" else np.int32))


# rectangles of MAIN (bands of rows 24..31 and 48..55, of columns 24..31, 48..55 and 72..79)
REGIONS = [(3, 5, 20, 22),         # inside tile 0's own area
           (3, 33, 20, 47),        # inside tile 1's own area: one tile, and not the first
           (10, 20, 21, 37),       # across one band of columns
           (20, 26, 60, 30),       # inside a band of columns, across two bands of rows
           (25, 27, 29, 30),       # inside a four-tile corner
           (21, 19, 35, 59),       # through two corners
           (69, 99, 70, 100),      # the last sample
           (0, 0, 1, 100), (0, 0, 70, 1),
           (8, 24, 56, 64),        # every multiple of 4: wide
           (31, 4, 33, 100),       # two rows, aligned columns: wide
           (1, 2, 70, 98)]         # rw a multiple of 4, rx0 not: sample by sample


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", [1, 3])
def test_rectangles_off_every_alignment_with_only_their_tiles_in_the_table(C, layout, kind):
    grid = _grid(MAIN)
    counts = []
    for region in REGIONS:
        counts.append(sum(len(g.indices) for g in grid.tiles_of_region(*region)))
        _check_blend(MAIN, C, layout, kind, region=region, only_needed=True)
    assert counts == [1, 1, 2, 6, 4, 6, 1, 4, 3, 9, 8, 12]
    assert _check_blend(MAIN, C, layout, kind, region=REGIONS[9], only_needed=True, want_path=1).shape == (C, 48, 40)
    for region in [(2, 3, 69, 101), (0, 1, 71, 99)]:
        _check_blend(ODD, C, layout, kind, region=region, only_needed=True, want_path=0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_needed_tile_that_is_null_leaves_its_samples_alone(layout, kind):
    # tile 5 (rows 24..55, columns 24..55) missing: its samples, bands with the eight neighbours included, keep the sentinel; every
    # other sample is written, nothing else changes.  Both paths; and two missing tiles in the odd grid.
    for off, path in ((0, 1), (1, 0)):
        pic = _check_blend(MAIN, 3, layout, kind, null=(5,), off=off, want_path=path)
        sentinel = SENTINEL_U if kind == "u8" else SENTINEL_F
        assert (pic[:, 24:56, 24:56] == sentinel).all() and int((pic == sentinel).sum()) >= 3 * 32 * 32
    _check_blend(ODD, 4, layout, kind, null=(0, 11), want_path=0)
    _check_blend(MAIN, 3, layout, kind, region=(20, 20, 60, 60), null=(5, 6), want_path=1)


def _cut_raw(L, fn, img_ptr, layout, C, H, W, g, dst_ptr):
    from cbench_basic_amd.nn import kernels as K
    return fn(img_ptr, K.IMAGE_LAYOUTS[layout], C, H, W, g.y0, g.x0, g.step_y, g.step_x, g.ny, g.nx, g.h, g.w, dst_ptr,
              torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_overlapped_cut_is_the_crop_divided_by_255(C, layout):
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    L = _lib.lib()
    for spec in (MAIN, ODD):
        grid = _grid(spec)
        H, W = grid.H, grid.W
        u = torch.randint(0, 256, (C, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(C * 1000 + H + W))
        flat = (u if layout == "chw" else u.permute(1, 2, 0)).contiguous().reshape(-1)
        big = torch.full((GUARD + flat.numel() + GUARD,), SENTINEL_U, dtype=torch.uint8)
        big[GUARD:GUARD + flat.numel()] = flat
        big = big.cuda()
        for g in grid.groups():
            m = g.ny * g.nx * C * g.h * g.w
            dst = torch.full((16 + m + 16,), SENTINEL_F, dtype=torch.float32, device="cuda")
            _lib.check(_cut_raw(L, L.basic_image_tiles_overlap_u8_to_f32_dev, big[GUARD:].data_ptr(), layout, C, H, W, g, dst[16:].data_ptr()))
            wide = W % 4 == 0 and g.x0 % 4 == 0 and g.step_x % 4 == 0 and g.w % 4 == 0 and (layout == "chw" or C in (1, 3, 4))
            assert K.image_tiles_last_path() == int(wide) == (0 if spec == ODD else int(layout == "chw" or C != 2)), (spec, C, layout, g[:8])
            got = dst.cpu()
            want = torch.stack([u[:, y:y + g.h, x:x + g.w].float().div(255) for y, x in
                                [(g.y0 + i * g.step_y, g.x0 + j * g.step_x) for i in range(g.ny) for j in range(g.nx)]])
            assert torch.equal(got[16:16 + m].view(want.shape).view(torch.int32), want.view(torch.int32)), (spec, C, layout, g[:8])      # bit for bit
            assert bool((got[:16] == SENTINEL_F).all()) and bool((got[16 + m:] == SENTINEL_F).all())
        assert torch.equal(big.cpu()[GUARD:GUARD + flat.numel()], flat)      # the picture is only read
    # the new entry keeps every other refusal of the cut
    g = _grid(MAIN).groups()[0]
    img, dst = torch.zeros(3 * 70 * 100, dtype=torch.uint8, device="cuda"), torch.zeros(6 * 3 * 32 * 32, device="cuda")
    for bad in (g._replace(step_x=0), g._replace(step_y=-24), g._replace(ny=3), g._replace(x0=28), g._replace(h=0)):
        assert _cut_raw(L, L.basic_image_tiles_overlap_u8_to_f32_dev, img.data_ptr(), "chw", 3, 70, 100, bad, dst.data_ptr()) == _lib.ERR_INVALID
        assert _lib.last_error()


def test_python_front_ends():
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    grid, batches, dev, full = _case(MAIN, 3)
    sources = [(d, idx) for d, (_, idx) in zip(dev, batches)]
    for layout in LAYOUTS:
        for dtype in (torch.uint8, torch.float32):
            out = torch.empty((1, 70, 100, 3) if layout == "hwc" else (1, 3, 70, 100), dtype=dtype, device="cuda")
            out = out.permute(0, 3, 1, 2) if layout == "hwc" else out
            assert K.image_tiles_blend(sources, grid, out) is out
            got = out.cpu().numpy()[0]
            if dtype == torch.uint8:
                assert np.array_equal(got, E.quantise(full)), layout
            else:
                assert np.array_equal(np.isnan(got), np.isnan(full)) and np.array_equal(got[~np.isnan(got)].view(np.int32), full[~np.isnan(full)].view(np.int32))
    # a region from the sources of its own tiles only, batch by batch or as single tiles
    region = (21, 19, 35, 59)
    need = {k for g in grid.tiles_of_region(*region) for k in g.indices}
    singles = [(d[t:t + 1], [k]) for d, (_, idx) in zip(dev, batches) for t, k in enumerate(idx) if k in need]
    out = torch.empty((1, 3, 14, 40), device="cuda")
    K.image_tiles_blend(singles, grid, out, region=region)
    got, want = out.cpu().numpy()[0], full[:, 21:35, 19:59]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)].view(np.int32), want[~np.isnan(want)].view(np.int32))
    with pytest.raises(ValueError, match="needs tiles"):
        K.image_tiles_blend(singles[1:], grid, out, region=region)           # a tile nobody supplied
    with pytest.raises(ValueError):
        K.image_tiles_blend(sources, grid, out, region=(21, 19, 35, 60))     # an output of another size
    with pytest.raises(ValueError):
        K.image_tiles_blend(sources, grid, out, region=(60, 19, 74, 59))     # leaves the picture
    with pytest.raises(ValueError):
        K.image_tiles_blend([(dev[0][:, :, :31], batches[0][1])] + sources[1:], grid, torch.empty((1, 3, 70, 100), device="cuda"))      # sh < th
    with pytest.raises(ValueError):
        K.image_tiles_blend([(dev[0][:-1], batches[0][1])], grid, out, region=region)      # a tile short
    with pytest.raises(TypeError):
        K.image_tiles_blend(sources, grid, torch.empty((1, 3, 70, 100), device="cuda", dtype=torch.float16))
    with pytest.raises(_lib.BasicHipError):
        K.image_tiles_blend(sources, grid, torch.empty((1, 3, 70, 100)))     # a host output: no CPU path
    # the cut through the wrapper: a group of overlapped tiles goes to the new entry
    u = torch.randint(0, 256, (1, 3, 70, 100), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    for pic in (u.cuda(), u.cuda().contiguous(memory_format=torch.channels_last)):
        for g in grid.groups():
            tiles = K.image_tiles_to_f32(pic, g)
            want = torch.stack([u[0, :, y:y + g.h, x:x + g.w].float().div(255) for y, x in
                                [(g.y0 + i * g.step_y, g.x0 + j * g.step_x) for i in range(g.ny) for j in range(g.nx)]])
            assert torch.equal(tiles.cpu(), want), g[:8]


def test_bad_arguments_are_invalid_and_launch_nothing():
    from cbench_basic_amd import _lib
    L = _lib.lib()
    grid, batches, dev, _ = _case(MAIN, 3)
    table = _table(grid, batches, dev)
    out_u = torch.full((3 * 70 * 100 + 8,), SENTINEL_U, dtype=torch.uint8, device="cuda")
    out_f = torch.full((3 * 70 * 100 + 8,), SENTINEL_F, dtype=torch.float32, device="cuda")
    whole = (0, 0, 70, 100)

    def call(table_ptr=table.data_ptr(), H=70, W=100, th=32, tw=32, oy=8, ox=8, C=3, region=whole, out=out_u.data_ptr(), kind=_lib.PIXEL_U8,
             layout=_lib.IMAGE_CHW):
        y0, x0, y1, x1 = region
        return L.basic_image_tiles_blend_dev(table_ptr, H, W, th, tw, oy, ox, C, y0, x0, y1 - y0, x1 - x0, out, kind, layout,
                                             torch.cuda.current_stream().cuda_stream)
    bad = {
        "null table": dict(table_ptr=None), "null output": dict(out=None), "layout 2": dict(layout=2), "layout -1": dict(layout=-1),
        "kind 2": dict(kind=2), "kind -1": dict(kind=-1), "no channels": dict(C=0), "H = 0": dict(H=0), "W < 0": dict(W=-100),
        "th = 0": dict(th=0), "tw < 0": dict(tw=-32), "oy < 0": dict(oy=-1), "ox < 0": dict(ox=-8),
        "oy above half a tile": dict(oy=17), "ox above half a tile": dict(ox=17), "oy = th": dict(oy=32),
        "rh = 0": dict(region=(5, 5, 5, 9)), "rw < 0": dict(region=(5, 9, 9, 5)), "ry0 < 0": dict(region=(-1, 0, 5, 5)),
        "rx0 < 0": dict(region=(0, -4, 5, 4)), "a row too many": dict(region=(0, 0, 71, 100)), "a column too many": dict(region=(0, 4, 70, 104)),
        "ry0 + rh overflows an int": dict(region=(2 ** 31 - 1 - 70, 0, 2 ** 31 - 1, 100)),
        "misaligned float output": dict(out=out_f.data_ptr() + 2, kind=_lib.PIXEL_F32),
        "2^41 samples": dict(H=2 ** 20, W=2 ** 20, C=2, region=(0, 0, 2 ** 20, 2 ** 20)),
    }
    for what, kw in bad.items():
        rc = call(**kw)
        assert rc == _lib.ERR_INVALID, what
        assert _lib.last_error(), what
        with pytest.raises(ValueError):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((out_u.cpu() == SENTINEL_U).all()) and bool((out_f.cpu() == SENTINEL_F).all())      # nothing was launched
    assert call(oy=16, ox=16, H=70, W=100, region=(0, 0, 1, 1)) == 0                                # exactly half a tile is allowed
