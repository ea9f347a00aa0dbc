"""The tile kernels (csrc/image.hip, include/basic_hip.h section 8c) against torch on the CPU, exactly: a cut tile is
``img[..., y:y + h, x:x + w].float().div(255)`` bit for bit, a pasted tile is
``torch.nan_to_num(x, nan=0.0).clamp(0, 1).mul(255).round().to(torch.uint8)`` of the top-left th x tw of its source, for both layouts of
the picture, both paths (wide / sample by sample; which one a call took is asserted), and with every byte outside the tiles and in
guard bands around the picture left alone."""
import pytest
import torch

from cbench_basic_amd.utils.tiling import TileGrid, TileGroup

pytestmark = pytest.mark.gpu

LAYOUTS = ["chw", "hwc"]
CHANNELS = [1, 3, 4]
GUARD = 64            # bytes of sentinel on either side of the picture; a multiple of 4, so an offset of 0 keeps the wide path
SENTINEL_U, SENTINEL_F = 0xA5, -7.5


def _cpu_quantise(x):
    return torch.nan_to_num(x, nan=0.0).clamp(0, 1).mul(255).round().to(torch.uint8)


def _mem(chw, layout):
    """[C, H, W] values -> the flat memory image of the picture in `layout`."""
    return (chw if layout == "chw" else chw.permute(1, 2, 0)).contiguous().reshape(-1)


def _unmem(flat, C, H, W, layout):
    return flat.view(C, H, W) if layout == "chw" else flat.view(H, W, C).permute(2, 0, 1)


def _origins(g):
    return [(g.y0 + i * g.step_y, g.x0 + j * g.step_x) for i in range(g.ny) for j in range(g.nx)]


def _group(y0, x0, step_y, step_x, ny, nx, h, w):
    return TileGroup(y0, x0, step_y, step_x, ny, nx, h, w, tuple(range(ny * nx)))


def _expect_wide(C, W, layout, g, off, sw=None):
    """The rule of section 8c (the float side of these tests is always 16-byte aligned)."""
    ok = off % 4 == 0 and W % 4 == 0 and g.x0 % 4 == 0 and g.step_x % 4 == 0 and g.w % 4 == 0 and (sw is None or sw % 4 == 0)
    return int(ok and (layout == "chw" or C in (1, 3, 4)))


def _cut_raw(L, img_ptr, layout, C, H, W, g, dst_ptr):
    from cbench_basic_amd.nn import kernels as K
    return L.basic_image_tiles_u8_to_f32_dev(img_ptr, K.IMAGE_LAYOUTS[layout] if isinstance(layout, str) else layout, C, H, W, g.y0, g.x0,
                                             g.step_y, g.step_x, g.ny, g.nx, g.h, g.w, dst_ptr, torch.cuda.current_stream().cuda_stream)


def _paste_raw(L, src_ptr, sh, sw, C, g, img_ptr, layout, H, W):
    from cbench_basic_amd.nn import kernels as K
    return L.basic_image_tiles_f32_to_u8_dev(src_ptr, sh, sw, C, g.y0, g.x0, g.step_y, g.step_x, g.ny, g.nx, g.h, g.w, img_ptr,
                                             K.IMAGE_LAYOUTS[layout] if isinstance(layout, str) else layout, H, W,
                                             torch.cuda.current_stream().cuda_stream)


def _check_cut(C, H, W, layout, groups, off, want_path=None):
    """Every group cut out of a seeded C x H x W picture whose memory starts `off` bytes into a buffer; -> the tiles, per group."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    L = _lib.lib()
    u = torch.randint(0, 256, (C, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(C * 1000 + H + W))
    n = C * H * W
    big = torch.full((GUARD + off + n + GUARD,), SENTINEL_U, dtype=torch.uint8)
    big[GUARD + off:GUARD + off + n] = _mem(u, layout)
    big = big.cuda()
    img = big[GUARD + off:GUARD + off + n]
    out = []
    for g in groups:
        m = g.ny * g.nx * C * g.h * g.w
        dst = torch.full((16 + m + 16,), SENTINEL_F, dtype=torch.float32, device="cuda")
        _lib.check(_cut_raw(L, img.data_ptr(), layout, C, H, W, g, dst[16:].data_ptr()))
        path = K.image_tiles_last_path()
        assert path == _expect_wide(C, W, layout, g, off), (C, H, W, layout, g[:8], off, path)
        if want_path is not None:
            assert path == want_path, (C, H, W, layout, g[:8], off)
        got = dst.cpu()
        want = torch.stack([u[:, y:y + g.h, x:x + g.w].float().div(255) for y, x in _origins(g)])
        tiles = got[16:16 + m].view(want.shape)
        assert torch.equal(tiles.view(torch.int32), want.view(torch.int32)), (C, H, W, layout, g[:8], off)      # bit for bit
        assert bool((got[:16] == SENTINEL_F).all()) and bool((got[16 + m:] == SENTINEL_F).all())
        out.append(tiles)
    assert torch.equal(big.cpu()[GUARD + off:GUARD + off + n], _mem(u, layout))      # the picture is only read
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_cut_all_four_groups_with_edge_tiles(C, layout):
    # 70 x 100 in 32 x 32 tiles: 3 x 4 tiles, the edge tiles 6 high and 4 wide; every width here is a multiple of 4, so these calls go
    # wide wherever the layout allows.  71 x 102 (edges 7 and 6): no row of the picture starts on a dword, every call goes sample by sample
    groups = TileGrid(70, 100, 32, 32).groups()
    assert sorted((g.ny, g.nx, g.h, g.w) for g in groups) == [(1, 1, 6, 4), (1, 3, 6, 32), (2, 1, 32, 4), (2, 3, 32, 32)]
    _check_cut(C, 70, 100, layout, groups, off=0)
    groups = TileGrid(71, 102, 32, 32).groups()
    assert sorted((g.h, g.w) for g in groups) == [(7, 6), (7, 32), (32, 6), (32, 32)]
    _check_cut(C, 71, 102, layout, groups, off=0, want_path=0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
def test_cut_wide_path_and_a_base_moved_by_one_byte(C, layout):
    groups = TileGrid(64, 96, 32, 32).groups()
    assert len(groups) == 1 and (groups[0].ny, groups[0].nx) == (2, 3)
    wide = _check_cut(C, 64, 96, layout, groups, off=0, want_path=1)
    for off in (1, 2, 3):
        scalar = _check_cut(C, 64, 96, layout, groups, off=off, want_path=0)
        assert torch.equal(wide[0], scalar[0])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS + [2])
def test_cut_sub_grid_off_the_origin_with_gaps(C, layout):
    # origin (3, 8), steps (33, 40) over 20 x 24 tiles: wide where the layout allows (two interleaved channels: sample by sample);
    # origin (3, 5): sample by sample; a single row of tiles; a single tile in the picture's last corner
    _check_cut(C, 70, 100, layout, [_group(3, 8, 33, 40, 2, 2, 20, 24)], off=0, want_path=0 if (C == 2 and layout == "hwc") else 1)
    _check_cut(C, 70, 100, layout, [_group(3, 5, 33, 40, 2, 2, 20, 24), _group(69, 0, 1, 25, 1, 4, 1, 25), _group(67, 96, 3, 4, 1, 1, 3, 4)], off=0)


def _paste_source(n_tiles, C, sh, sw):
    """[n_tiles, C, sh, sw]: uniform values in [-0.25, 1.25), every rounding tie (k + 0.5) / 255, NaN, +-inf, negatives, values above 1."""
    m = n_tiles * C * sh * sw
    g = torch.Generator().manual_seed(m)
    x = torch.rand(m, generator=g) * 1.5 - 0.25
    special = torch.cat([(torch.arange(255, dtype=torch.float64) + 0.5).div(255).float(),
                         torch.tensor([float("nan"), float("inf"), float("-inf"), -1.0, -0.0, 2.0, 1.0, 1e30, -1e30])])
    k = min(special.numel(), m)
    x[torch.randperm(m, generator=g)[:k]] = special[torch.randperm(special.numel(), generator=g)[:k]]      # scattered over the tiles
    x[:k] = special[:k]                                                # and once more in the first rows of the first tile
    return x.view(n_tiles, C, sh, sw)


def _check_paste(C, H, W, layout, g, pad, off, want_path=None):
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    L = _lib.lib()
    sh, sw = g.h + pad[0], g.w + pad[1]
    x = _paste_source(g.ny * g.nx, C, sh, sw)
    n = C * H * W
    want = torch.full((C, H, W), SENTINEL_U, dtype=torch.uint8)
    for t, (y, xx) in enumerate(_origins(g)):
        want[:, y:y + g.h, xx:xx + g.w] = _cpu_quantise(x[t, :, :g.h, :g.w])
    if g.h * g.w >= 400:      # the kept corners do hold the special values
        kept = x[:, :, :g.h, :g.w]
        assert bool(torch.isnan(kept).any()) and bool(torch.isinf(kept).any()) and bool((kept < 0).any()) and bool((kept > 1).any())
        ties = (torch.arange(255, dtype=torch.float64) + 0.5).div(255).float()
        assert int(torch.isin(ties, kept).sum()) >= 200
    big = torch.full((GUARD + off + n + GUARD,), SENTINEL_U, dtype=torch.uint8, device="cuda")
    xd = x.cuda()
    _lib.check(_paste_raw(L, xd.data_ptr(), sh, sw, C, g, big[GUARD + off:].data_ptr(), layout, H, W))
    path = K.image_tiles_last_path()
    assert path == _expect_wide(C, W, layout, g, off, sw=sw), (C, H, W, layout, g[:8], pad, off, path)
    if want_path is not None:
        assert path == want_path
    got = big.cpu()
    assert bool((got[:GUARD + off] == SENTINEL_U).all()) and bool((got[GUARD + off + n:] == SENTINEL_U).all())      # guard bytes
    pic = _unmem(got[GUARD + off:GUARD + off + n], C, H, W, layout)
    assert torch.equal(pic, want), (C, H, W, layout, g[:8], pad, off)      # the tiles' bytes, and 0xA5 everywhere outside them
    return pic


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("pad", [(5, 4), (0, 0)])
def test_paste_crops_converts_and_leaves_the_rest_alone(C, layout, pad):
    # gaps between the tiles and a border around them: 0xA5 there before and after
    g = _group(3, 8, 33, 40, 2, 2, 20, 24)
    wide = _check_paste(C, 70, 100, layout, g, pad, off=0, want_path=1)
    for off in (1, 3):
        assert torch.equal(_check_paste(C, 70, 100, layout, g, pad, off=off, want_path=0), wide)
    _check_paste(C, 70, 100, layout, _group(3, 5, 33, 40, 2, 2, 20, 24), pad, off=0, want_path=0)
    _check_paste(C, 70, 100, layout, g, (pad[0], pad[1] + 1), off=0, want_path=0)      # sw no multiple of 4
    # a whole grid with edge tiles, group by group into one picture: every byte written exactly once
    for H, W in ((70, 100), (71, 102)):
        for grp in TileGrid(H, W, 32, 32).groups():
            _check_paste(C, H, W, layout, grp, pad, off=0)


def test_paste_two_interleaved_channels_goes_sample_by_sample():
    g = _group(0, 0, 32, 32, 2, 3, 32, 32)
    assert torch.equal(_check_paste(2, 64, 96, "hwc", g, (5, 4), off=0, want_path=0), _check_paste(2, 64, 96, "chw", g, (5, 4), off=0, want_path=1))


def test_python_front_ends():
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    u = torch.randint(0, 256, (1, 3, 70, 100), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    grid = TileGrid(70, 100, 32, 32)
    for name, pic in (("chw", u.cuda()), ("hwc", u.cuda().contiguous(memory_format=torch.channels_last)), ("strided", u.cuda()[:, :, :, ::2])):
        host = pic.cpu()
        H, W = host.shape[2:]
        for g in TileGrid(H, W, 32, 32).groups():
            tiles = K.image_tiles_to_f32(pic, g)
            assert tiles.dtype == torch.float32 and tuple(tiles.shape) == (g.ny * g.nx, 3, g.h, g.w) and tiles.is_contiguous()
            want = torch.stack([host[0, :, y:y + g.h, x:x + g.w].float().div(255) for y, x in _origins(g)])
            assert torch.equal(tiles.cpu(), want), (name, g[:8])
    # the way back through the wrapper: cut every group, paste it into an empty canvas of either layout -> the picture
    for layout in LAYOUTS:
        canvas = torch.zeros((1, 70, 100, 3) if layout == "hwc" else (1, 3, 70, 100), dtype=torch.uint8, device="cuda")
        canvas = canvas.permute(0, 3, 1, 2) if layout == "hwc" else canvas
        for g in grid.groups():
            assert K.image_tiles_from_f32(K.image_tiles_to_f32(u.cuda(), g), canvas, g) is canvas
        assert torch.equal(canvas.cpu(), u), layout
    g = grid.groups()[0]
    with pytest.raises(TypeError):
        K.image_tiles_to_f32(u.cuda().float(), g)
    with pytest.raises(ValueError):
        K.image_tiles_to_f32(u.cuda()[0], g)
    with pytest.raises(ValueError):
        K.image_tiles_to_f32(torch.cat([u, u]).cuda(), g)
    with pytest.raises(_lib.BasicHipError):
        K.image_tiles_to_f32(u, g)                                             # a host picture: no CPU path
    tiles = K.image_tiles_to_f32(u.cuda(), g)
    with pytest.raises(ValueError):
        K.image_tiles_from_f32(tiles[:-1], u.cuda(), g)                        # a tile short
    with pytest.raises(ValueError):
        K.image_tiles_from_f32(tiles, u.cuda()[:, :, :, ::2], g)               # a canvas that cannot be written in place
    with pytest.raises(TypeError):
        K.image_tiles_from_f32(tiles.half(), u.cuda(), g)


def test_bad_arguments_are_invalid_and_launch_nothing():
    from cbench_basic_amd import _lib
    L = _lib.lib()
    C, H, W = 3, 64, 96
    img = torch.full((C * H * W + 4,), SENTINEL_U, dtype=torch.uint8, device="cuda")
    flt = torch.full((6 * C * 40 * 40 + 4,), SENTINEL_F, dtype=torch.float32, device="cuda")
    ok = _group(0, 0, 32, 32, 2, 3, 32, 32)
    bad_groups = {
        "ny = 0": ok._replace(ny=0), "nx < 0": ok._replace(nx=-1), "th = 0": ok._replace(h=0), "tw < 0": ok._replace(w=-4),
        "step_y = 0": ok._replace(step_y=0), "step_x < 0": ok._replace(step_x=-32), "y0 < 0": ok._replace(y0=-1), "x0 < 0": ok._replace(x0=-4),
        "step_y < th": ok._replace(step_y=31), "step_x < tw": ok._replace(step_x=28, w=32),
        "last row leaves": ok._replace(y0=1), "last column leaves": ok._replace(x0=4), "a row too many": ok._replace(ny=3),
        "a column too many": ok._replace(nx=4), "one tile too high": _group(0, 0, 65, 32, 1, 1, 65, 32),
    }
    st = torch.cuda.current_stream().cuda_stream

    def refused(rc, what):
        assert rc == _lib.ERR_INVALID, what
        assert _lib.last_error(), what
        with pytest.raises(ValueError):
            _lib.check(rc)
    # cut
    for what, g in bad_groups.items():
        refused(_cut_raw(L, img.data_ptr(), "chw", C, H, W, g, flt.data_ptr()), what)
    refused(_cut_raw(L, None, "chw", C, H, W, ok, flt.data_ptr()), "null picture")
    refused(_cut_raw(L, img.data_ptr(), "hwc", C, H, W, ok, None), "null destination")
    refused(_cut_raw(L, img.data_ptr(), 2, C, H, W, ok, flt.data_ptr()), "layout 2")
    refused(_cut_raw(L, img.data_ptr(), -1, C, H, W, ok, flt.data_ptr()), "layout -1")
    refused(_cut_raw(L, img.data_ptr(), "chw", 0, H, W, ok, flt.data_ptr()), "no channels")
    refused(_cut_raw(L, img.data_ptr(), "chw", C, 0, W, ok, flt.data_ptr()), "img_h = 0")
    refused(_cut_raw(L, img.data_ptr(), "chw", C, H, -W, ok, flt.data_ptr()), "img_w < 0")
    refused(_cut_raw(L, img.data_ptr(), "chw", C, H, W, ok, flt.data_ptr() + 2), "misaligned float pointer")
    big = 2 ** 20      # 2^41 samples of one channel, in a picture that would hold them
    refused(_cut_raw(L, img.data_ptr(), "chw", 1, 2 * big, big, _group(0, 0, big, big, 2, 1, big, big), flt.data_ptr()), "2^41 samples")
    # paste
    for what, g in bad_groups.items():
        refused(_paste_raw(L, flt.data_ptr(), 40, 40, C, g, img.data_ptr(), "hwc", H, W), what)
    refused(_paste_raw(L, flt.data_ptr(), 31, 40, C, ok, img.data_ptr(), "chw", H, W), "sh < th")
    refused(_paste_raw(L, flt.data_ptr(), 40, 28, C, ok, img.data_ptr(), "chw", H, W), "sw < tw")
    refused(_paste_raw(L, flt.data_ptr(), 0, 40, C, ok, img.data_ptr(), "chw", H, W), "sh = 0")
    refused(_paste_raw(L, None, 40, 40, C, ok, img.data_ptr(), "chw", H, W), "null source")
    refused(_paste_raw(L, flt.data_ptr(), 40, 40, C, ok, None, "chw", H, W), "null picture")
    refused(_paste_raw(L, flt.data_ptr(), 40, 40, C, ok, img.data_ptr(), 7, H, W), "layout 7")
    refused(_paste_raw(L, flt.data_ptr(), 40, 40, -C, ok, img.data_ptr(), "chw", H, W), "channels < 0")
    refused(_paste_raw(L, flt.data_ptr() + 1, 40, 40, C, ok, img.data_ptr(), "chw", H, W), "misaligned float pointer")
    refused(_paste_raw(L, flt.data_ptr(), 2 * big, big, 1, _group(0, 0, big, big, 1, 1, big, big), img.data_ptr(), "chw", big, big), "2^41 samples")
    with pytest.raises(ValueError):
        _lib.check(L.basic_image_tiles_last_path(None))
    torch.cuda.synchronize()
    assert bool((img.cpu() == SENTINEL_U).all()) and bool((flt.cpu() == SENTINEL_F).all())      # nothing was launched
