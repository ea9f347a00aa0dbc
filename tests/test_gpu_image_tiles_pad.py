"""The edge-padded cut and the clipped paste of include/basic_hip.h section 8d (nn.kernels.image_tiles_gather(pad=True) /
image_tiles_scatter(clip=True)): tiles that leave their picture at the bottom and right.  Exact against the numpy restatement of
tests/tile_pad_exact.py; both paths asserted through image_tiles_last_path; the canvases of the paste are views inside larger buffers
filled with a marker, and the WHOLE buffer is compared; every refusal is returned before anything is copied or launched (arguments
only: nothing is provoked on the device).

The tables: a 12 x 20 picture under tiles of 16 x 16 at the origins (0, 16) (runs 1..3 of every row outside), (8, 0) (rows 12..23 outside),
(8, 16) (both) and (0, 0).  A 16 x 16 tile at (0, 0) of a 12-row picture still leaves it at the bottom, so the bit-for-bit comparison
with the existing gather, which needs tiles wholly inside, is made on a second table of 8 x 16 tiles."""
import functools

import numpy as np
import pytest
import torch

import tile_blend_exact as B
import tile_pad_exact as E

pytestmark = pytest.mark.gpu

MARK = 0xAB
GUARD = 64                                    # bytes of marker in front of and behind a canvas
FORMS = [(1, "chw"), (2, "chw"), (3, "chw"), (3, "hwc"), (4, "hwc")]      # planar with C = 1, 2, 3; interleaved with C = 3, 4
IDS = [f"{layout}-C{C}" for C, layout in FORMS]
ORIGINS = [(0, 16), (8, 0), (8, 16), (0, 0)]


@functools.lru_cache(maxsize=None)
def _host(C, H, W):
    """The picture uint8 [C, H, W], numpy; computed once and left unchanged."""
    return np.random.default_rng(1000 * C + 10 * H + W).integers(0, 256, (C, H, W), dtype=np.uint8)


def _views(C, H, W, layout, off=0, fill=None):
    """A [1, C, H, W] uint8 picture of the given memory order that lies ``GUARD + off`` bytes into a larger buffer, on the device and
    in numpy: (device buffer, device view, numpy buffer, numpy [C, H, W] view).  ``fill``: the byte the buffers start with."""
    n = C * H * W
    dev = torch.full((n + 2 * GUARD + 4,), MARK if fill is None else fill, dtype=torch.uint8, device="cuda")
    host = np.full(n + 2 * GUARD + 4, MARK if fill is None else fill, dtype=np.uint8)
    lo = GUARD + off
    if layout == "hwc":
        return dev, dev[lo:lo + n].view(1, H, W, C).permute(0, 3, 1, 2), host, host[lo:lo + n].reshape(H, W, C).transpose(2, 0, 1)
    return dev, dev[lo:lo + n].view(1, C, H, W), host, host[lo:lo + n].reshape(C, H, W)


def _picture(C, H, W, layout, off=0):
    """The device picture of _host(C, H, W) in that memory order and alignment."""
    _, view, _, _ = _views(C, H, W, layout, off)
    view.copy_(torch.from_numpy(_host(C, H, W))[None])
    assert view.data_ptr() % 4 == off % 4
    return view


def _wide(C, rows, specs, pw, sw=None):
    """The rule of section 8d: rows = [(picture, y, x)], specs[p] = (H, W, layout, off)."""
    ok = pw % 4 == 0 and (sw is None or sw % 4 == 0)
    for p, _, x in rows:
        _, W, layout, off = specs[p]
        ok = ok and off % 4 == 0 and W % 4 == 0 and x % 4 == 0 and (layout == "chw" or C in (1, 3, 4))
    return int(ok)


def _check_gather(C, specs, rows, ph, pw, path):
    from cbench_basic_amd.nn import kernels as K
    pictures = [_picture(C, H, W, layout, off) for H, W, layout, off in specs]
    refs = [(p, t, y, x) for t, (p, y, x) in enumerate(rows)]
    got = K.image_tiles_gather(pictures, refs, ph, pw, pad=True)
    assert K.image_tiles_last_path() == path == _wide(C, rows, specs, pw), (C, specs, rows)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(rows), C, ph, pw)
    want = np.stack([E.padded_tile(_host(C, *specs[p][:2]), y, x, ph, pw) for p, y, x in rows])
    assert np.array_equal(got.cpu().numpy(), want), (C, specs, rows)
    return pictures, refs, got


@pytest.mark.parametrize("C,layout", FORMS, ids=IDS)
def test_wide_gather_replicates_the_last_row_and_column(C, layout):
    from cbench_basic_amd.nn import kernels as K
    specs = [(12, 20, layout, 0)]
    _check_gather(C, specs, [(0, y, x) for y, x in ORIGINS], 16, 16, 1)
    for y, x in ORIGINS:                                   # each origin alone: a table of one row
        _check_gather(C, specs, [(0, y, x)], 16, 16, 1)
    # no tile leaves the picture: bit for bit the existing gather, and the existing gather refuses what the padded one takes
    inside = [(0, 0, 0), (0, 4, 4), (0, 0, 4)]
    pictures, refs, got = _check_gather(C, specs, inside, 8, 16, 1)
    assert torch.equal(got, K.image_tiles_gather(pictures, refs, 8, 16))
    with pytest.raises(ValueError, match="the tile leaves the picture"):
        K.image_tiles_gather(pictures, [(0, 0, 0, 0)], 16, 16)


@pytest.mark.parametrize("C,layout", FORMS, ids=IDS)
def test_scalar_gather_clamps_every_sample(C, layout):
    from cbench_basic_amd.nn import kernels as K
    corner = [(0, y, x) for y, x in ORIGINS]
    _check_gather(C, [(12, 18, layout, 0)], corner + [(0, 11, 17)], 16, 16, 0)          # W no multiple of 4; a valid size of 1 x 1
    _check_gather(C, [(12, 20, layout, 1)], corner + [(0, 11, 19)], 16, 16, 0)          # a base pointer off 4-byte alignment
    _check_gather(C, [(12, 20, layout, 0)], corner + [(0, 11, 19), (0, 3, 5)], 16, 16, 0)   # an origin that is no multiple of 4
    _check_gather(C, [(12, 20, layout, 0)], corner, 15, 14, 0)                          # a tile width that is no multiple of 4
    pictures, refs, got = _check_gather(C, [(12, 18, layout, 0)], [(0, 0, 0), (0, 5, 3)], 7, 15, 0)   # wholly inside
    assert torch.equal(got, K.image_tiles_gather(pictures, refs, 7, 15))


# three pictures of different sizes and layouts under one table; tiles of 8 x 8
MANY = [(0, 8, 16), (1, 4, 12), (2, 0, 8), (0, 0, 0), (1, 8, 0), (2, 6, 8), (1, 8, 12), (0, 4, 12)]


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_one_launch_over_rows_of_three_pictures(C):
    wide = [(12, 20, "chw", 0), (9, 16, "hwc", 0), (7, 12, "chw", 0)]
    _check_gather(C, wide, MANY, 8, 8, 0 if C == 2 else 1)                  # two interleaved channels: sample by sample
    _check_gather(C, [(12, 20, "hwc", 0), (9, 15, "chw", 0), (7, 12, "hwc", 0)], MANY, 8, 8, 0)
    _check_gather(C, [(12, 20, "chw", 0), (9, 16, "hwc", 0), (7, 12, "chw", 3)], MANY, 8, 8, 0)


def _check_scatter(C, specs, rows, ph, pw, sh, sw, path, seed=0):
    """Every row pastes into a canvas of its own (the rectangles of ORIGINS intersect in one picture), a view inside a marker-filled
    buffer; the whole buffers are compared."""
    from cbench_basic_amd.nn import kernels as K
    src = B._values(np.random.default_rng(seed + 100 * C + sh + sw), len(rows) * C * sh * sw).reshape(len(rows), C, sh, sw)
    assert np.isnan(src).any() and np.isposinf(src).any() and np.isneginf(src).any() and np.isin(B.TIES, src).sum() > 100
    canvases = [_views(C, *specs[p]) for p, _, _ in rows]
    refs = [(t, t, y, x) for t, (_, y, x) in enumerate(rows)]
    K.image_tiles_scatter(torch.from_numpy(src).cuda(), [c[1] for c in canvases], refs, ph, pw, clip=True)
    own = [(t, y, x) for t, (_, y, x) in enumerate(rows)]
    assert K.image_tiles_last_path() == path == _wide(C, own, [specs[p] for p, _, _ in rows], pw, sw), (C, specs, rows)
    for t, (p, y, x) in enumerate(rows):
        dev, _, host, view = canvases[t]
        E.clipped_paste(view, src[t], y, x, ph, pw)
        H, W = specs[p][:2]
        assert (host != MARK).sum() <= C * min(ph, H - y) * min(pw, W - x)           # nothing outside the valid rectangle
        assert np.array_equal(dev.cpu().numpy(), host), (C, specs, t, (y, x))
    return src


@pytest.mark.parametrize("C,layout", FORMS, ids=IDS)
def test_wide_scatter_writes_the_part_inside_and_no_other_byte(C, layout):
    rows = [(0, y, x) for y, x in ORIGINS]
    _check_scatter(C, [(12, 20, layout, 0)], rows, 16, 16, 20, 24, 1)
    _check_scatter(C, [(12, 20, layout, 0)], rows, 16, 16, 16, 16, 1, seed=1)
    _check_scatter(C, [(12, 20, layout, 0)], [(0, 0, 0), (0, 4, 4)], 8, 16, 12, 20, 1, seed=2)   # wholly inside


@pytest.mark.parametrize("C,layout", FORMS, ids=IDS)
def test_scalar_scatter_tests_every_sample(C, layout):
    rows = [(0, y, x) for y, x in ORIGINS]
    _check_scatter(C, [(12, 18, layout, 0)], rows + [(0, 11, 17)], 16, 16, 20, 24, 0)
    _check_scatter(C, [(12, 20, layout, 1)], rows + [(0, 11, 19)], 16, 16, 20, 24, 0, seed=1)
    _check_scatter(C, [(12, 20, layout, 0)], rows, 16, 16, 19, 21, 0, seed=2)           # sw no multiple of 4
    _check_scatter(C, [(12, 20, layout, 0)], rows + [(0, 3, 5)], 15, 14, 15, 14, 0, seed=3)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_one_scatter_over_canvases_of_three_sizes(C):
    _check_scatter(C, [(12, 20, "chw", 0), (9, 16, "hwc", 0), (7, 12, "chw", 0)], MANY, 8, 8, 12, 12, 1)
    _check_scatter(C, [(12, 20, "hwc", 0), (9, 15, "chw", 0), (7, 12, "hwc", 2)], MANY, 8, 8, 9, 11, 0, seed=1)


def test_a_clipped_scatter_of_tiles_inside_equals_the_plain_scatter():
    from cbench_basic_amd.nn import kernels as K
    src = torch.from_numpy(B._values(np.random.default_rng(3), 2 * 3 * 12 * 20).reshape(2, 3, 12, 20)).cuda()
    a, b = torch.full((1, 3, 12, 20), MARK, dtype=torch.uint8, device="cuda"), torch.full((1, 3, 12, 20), MARK, dtype=torch.uint8, device="cuda")
    refs = [(0, 0, 0, 0), (0, 1, 4, 4)]      # the second after the first: their rectangles intersect
    for t in range(2):
        K.image_tiles_scatter(src[t:t + 1], [a], refs[t:t + 1], 8, 16, clip=True)
        K.image_tiles_scatter(src[t:t + 1], [b], refs[t:t + 1], 8, 16)
    assert torch.equal(a, b) and bool((a != MARK).any())
    with pytest.raises(ValueError, match="the tile leaves the picture"):
        K.image_tiles_scatter(src[:1], [b], [(0, 0, 0, 8)], 8, 16)


def test_refusals_come_before_any_copy_or_launch():
    """Arguments only: every call below is refused on the host.  The batch, the picture and the table workspace keep their marker
    bytes, and the path report keeps the value of the last accepted call."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    L = _lib.lib()
    C, H, W, n = 3, 16, 24, 2
    img = torch.full((1, C, H, W), MARK, dtype=torch.uint8, device="cuda")
    ws = torch.full((n * 32 + 8,), MARK, dtype=torch.uint8, device="cuda")
    f32 = torch.full((n * C * 12 * 16 + 4,), 7.0, device="cuda")
    K.image_tiles_gather([img], [(0, 0, 12, 20)], 8, 8, pad=True)
    before = K.image_tiles_last_path()
    stream = K._stream()

    def table(**change):
        t = np.zeros(n, dtype=K._TILE_REF)
        for k in range(n):
            t[k] = (img.data_ptr(), H, W, 12 * k, 20 * k, _lib.IMAGE_CHW, 0)     # row 1 leaves the picture at the bottom and right
        for field, value in change.items():
            t[field][1] = value
        return t

    def gather(t=None, n_=n, channels=C, ph=8, pw=8, ws_=None, dst=None, null_table=False):
        t = table() if t is None else t
        return L.basic_image_tiles_gather_pad_u8_to_f32_dev(None if null_table else t.ctypes.data, n_, channels, ph, pw,
                                                            ws.data_ptr() if ws_ is None else ws_, f32.data_ptr() if dst is None else dst, stream)

    def scatter(t=None, n_=n, channels=C, ph=8, pw=8, sh=12, sw=16, ws_=None, src=None, null_table=False):
        t = table() if t is None else t
        return L.basic_image_tiles_scatter_clip_f32_to_u8_dev(f32.data_ptr() if src is None else src, sh, sw, channels, ph, pw,
                                                              None if null_table else t.ctypes.data, n_, ws.data_ptr() if ws_ is None else ws_, stream)
    BIG = 1 << 20
    cases = {
        "null table": dict(null_table=True), "null workspace": dict(ws_=0), "null batch": dict(dst=0), "null picture": dict(t=table(img=0)),
        "n = 0": dict(n_=0), "n < 0": dict(n_=-1), "channels = 0": dict(channels=0), "ph = 0": dict(ph=0), "pw < 0": dict(pw=-8),
        "img_h = 0": dict(t=table(img_h=0)), "img_w < 0": dict(t=table(img_w=-24)), "layout": dict(t=table(layout=2)),
        "y0 < 0": dict(t=table(y0=-1)), "x0 < 0": dict(t=table(x0=-4)), "origin below": dict(t=table(y0=H)), "origin right": dict(t=table(x0=W)),
        "origin far": dict(t=table(y0=1 << 30, x0=1 << 30)),
        "float alignment": dict(dst=f32.data_ptr() + 2), "workspace alignment": dict(ws_=ws.data_ptr() + 4),
        "2^40 samples": dict(ph=BIG, pw=BIG + 4),
    }
    for name, kw in cases.items():
        assert gather(**kw) == _lib.ERR_INVALID, name
        assert "image_tiles_gather_pad_u8_to_f32" in _lib.last_error(), (name, _lib.last_error())
        if name.startswith("origin"):
            assert "the tile's origin leaves the picture" in _lib.last_error(), (name, _lib.last_error())
        kw = {("src" if k == "dst" else k): v for k, v in kw.items()}
        if name == "2^40 samples":
            kw = dict(sh=BIG, sw=BIG + 4)
        assert scatter(**kw) == _lib.ERR_INVALID, name
        assert "image_tiles_scatter_clip_f32_to_u8" in _lib.last_error(), (name, _lib.last_error())
        if name.startswith("origin"):
            assert "the tile's origin leaves the picture" in _lib.last_error(), (name, _lib.last_error())
    for name, kw in {"sh < ph": dict(sh=7), "sw < pw": dict(sw=4), "sh = 0": dict(sh=0), "sw < 0": dict(sw=-16)}.items():
        assert scatter(**kw) == _lib.ERR_INVALID, name
    with pytest.raises(ValueError):          # through the front-end: a ValueError
        K.image_tiles_gather([img], [(0, 0, H, 0)], 8, 8, pad=True)
    with pytest.raises(ValueError):
        K.image_tiles_scatter(f32[:C * 64].view(1, C, 8, 8), [img], [(0, 0, 0, W)], 8, 8, clip=True)
    torch.cuda.synchronize()
    assert K.image_tiles_last_path() == before
    assert bool((img == MARK).all()) and bool((ws == MARK).all()) and bool((f32 == 7.0).all())
    assert gather() == _lib.OK and scatter() == _lib.OK                       # the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert bool((ws != MARK).any()) and bool((f32 != 7.0).any())
