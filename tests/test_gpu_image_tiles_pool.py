"""The table-driven cut and paste of include/basic_hip.h section 8d (nn.kernels.image_tiles_gather / image_tiles_scatter): tiles of
many pictures in one launch.  Exact against torch on the CPU -- ``img[..., y:y + h, x:x + w].float().div(255)`` on the way in,
image_f32_to_u8's definition on the way out -- and against the single-picture entries of section 8c; both paths asserted through
image_tiles_last_path; every refusal returned before anything is copied or launched (arguments only: nothing is provoked on the
device)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(16, 24), (13, 19)]
SENTINEL = 0xAB


@functools.lru_cache(maxsize=None)
def _pictures(C):
    """Computed once per channel count and left unchanged.  For each size, on the GPU: the picture in chw memory, in hwc memory, and in
    chw memory one byte off 4-byte alignment; and the same picture on the host."""
    g = torch.Generator().manual_seed(100 + C)
    out = []
    for H, W in SIZES:
        host = torch.randint(0, 256, (1, C, H, W), dtype=torch.uint8, generator=g)
        chw = host.cuda()
        hwc = host.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).cuda()
        buf = torch.empty(C * H * W + 1, dtype=torch.uint8, device="cuda")
        off = buf[1:].view(1, C, H, W)
        off.copy_(chw)
        assert chw.data_ptr() % 4 == 0 and hwc.data_ptr() % 4 == 0 and off.data_ptr() % 4 == 1
        out.append(dict(host=host, chw=chw, hwc=hwc, off=off))
    return out


def _device_pictures(C, kinds):
    """[picture] and, beside it, the host picture of each: kinds = [(size index, "chw" / "hwc" / "off")]."""
    P = _pictures(C)
    return [P[s][k] for s, k in kinds], [P[s]["host"] for s, _ in kinds]


def _u8_definition(x):
    return torch.nan_to_num(x, nan=0.0).clamp(0, 1).mul(255).round().to(torch.uint8)


# pictures of the tables below: 0 = 16 x 24 chw, 1 = 16 x 24 hwc, 2 = 13 x 19 chw, 3 = 13 x 19 hwc, 4 = 16 x 24 chw off alignment
KINDS = [(0, "chw"), (0, "hwc"), (1, "chw"), (1, "hwc"), (0, "off")]
# (name, (h, w), rows (picture, y0, x0), expected path).  wide: 8 x 8 tiles in the 16 x 24 pictures, x0 a multiple of 4 -- mixed layouts, a
# picture in several rows, rows that overlap (y0 3, x0 4 against the tile at the origin), tiles flush with the bottom and right edge.
GATHERS = [
    ("wide", (8, 8), [(0, 0, 0), (1, 0, 8), (0, 3, 4), (1, 8, 16), (0, 8, 16), (1, 5, 12), (0, 8, 0)], 1),
    ("wide-one-row", (8, 8), [(1, 8, 16)], 1),
    ("x0-not-multiple-of-4", (8, 8), [(0, 0, 0), (1, 8, 5)], 0),
    ("width-not-multiple-of-4", (8, 8), [(0, 0, 0), (2, 5, 8)], 0),
    ("base-off-alignment", (8, 8), [(0, 0, 0), (4, 8, 16)], 0),
    ("scalar", (5, 7), [(0, 0, 0), (3, 8, 12), (2, 8, 12), (1, 11, 17), (2, 3, 5), (3, 1, 6), (4, 2, 3), (2, 0, 0)], 0),
    ("scalar-one-row", (5, 7), [(3, 8, 12)], 0),
]
# rectangles of one scatter do not intersect in a picture (pictures 0 and 1, 0 and 4, 2 and 3 are different canvases here)
SCATTERS = [
    ("wide", (8, 8), (12, 16), [(0, 0, 0), (1, 0, 8), (0, 8, 16), (1, 8, 16), (0, 8, 0), (1, 8, 0)], 1),
    ("wide-exact", (8, 8), (8, 8), [(1, 8, 16), (0, 4, 4)], 1),
    ("wide-one-row", (8, 8), (8, 12), [(0, 8, 16)], 1),
    ("sw-not-multiple-of-4", (8, 8), (8, 10), [(0, 0, 0), (1, 8, 16)], 0),
    ("x0-not-multiple-of-4", (8, 8), (12, 16), [(0, 0, 0), (1, 8, 5)], 0),
    ("base-off-alignment", (8, 8), (12, 16), [(0, 0, 0), (4, 8, 16)], 0),
    ("scalar", (5, 7), (6, 9), [(0, 0, 0), (3, 8, 12), (2, 8, 12), (1, 11, 17), (2, 0, 3), (3, 1, 2), (4, 2, 3), (0, 6, 9)], 0),
    ("scalar-one-row", (5, 7), (5, 7), [(2, 8, 12)], 0),
]


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("name,size,rows,path", GATHERS, ids=[g[0] for g in GATHERS])
def test_gather_equals_torch_and_the_single_picture_cut(C, name, size, rows, path):
    from cbench_basic_amd.nn import kernels as K
    h, w = size
    pictures, hosts = _device_pictures(C, KINDS)
    refs = [(p, t, y, x) for t, (p, y, x) in enumerate(rows)]
    got = K.image_tiles_gather(pictures, refs, h, w)
    assert K.image_tiles_last_path() == path, (name, C)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(rows), C, h, w)
    want = torch.cat([hosts[p][..., y:y + h, x:x + w].float().div(255) for p, y, x in rows])
    assert torch.equal(got.cpu(), want), (name, C)
    for t, (p, y, x) in enumerate(rows):     # the entry of one picture and one grid, for that picture and origin
        one = K.image_tiles_to_f32(pictures[p], (y, x, h, w, 1, 1, h, w))
        assert torch.equal(got[t:t + 1], one), (name, C, t)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("name,size,src,rows,path", SCATTERS, ids=[s[0] for s in SCATTERS])
def test_scatter_equals_the_definition_and_the_single_picture_paste(C, name, size, src, rows, path):
    from cbench_basic_amd.nn import kernels as K
    h, w = size
    sh, sw = src
    like, _ = _device_pictures(C, KINDS)
    g = torch.Generator().manual_seed(7 * C + len(rows))
    batch = torch.rand(len(rows), C, sh, sw, generator=g) * 2 - 0.5            # a third of it out of range
    flat = batch.view(-1)
    flat[::11] = float("nan")
    flat[3::17] = float("inf")
    flat[5::19] = float("-inf")
    flat[7::23] = 0.5 / 255                                                      # a tie: rounds to even
    dev = batch.cuda()

    def canvases():
        out = [torch.full_like(p, SENTINEL) for p in like]                      # full_like keeps chw / hwc memory
        buf = torch.full((like[4].numel() + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
        out[4] = buf[1:].view(like[4].shape)
        assert [K.image_layout_of(c) for c in out] == [K.image_layout_of(p) for p in like] and out[4].data_ptr() % 4 == 1
        return out
    got = canvases()
    refs = [(p, t, y, x) for t, (p, y, x) in enumerate(rows)]
    K.image_tiles_scatter(dev, got, refs, h, w)
    assert K.image_tiles_last_path() == path, (name, C)
    want = [torch.full(tuple(p.shape), SENTINEL, dtype=torch.uint8) for p in like]
    for t, (p, y, x) in enumerate(rows):
        want[p][0, :, y:y + h, x:x + w] = _u8_definition(batch[t, :, :h, :w])
    for p in range(len(like)):               # the tiles, and every byte outside them still the sentinel
        assert torch.equal(got[p].cpu(), want[p]), (name, C, p)
    single = canvases()
    for t, (p, y, x) in enumerate(rows):
        K.image_tiles_from_f32(dev[t:t + 1], single[p], (y, x, h, w, 1, 1, h, w))
    for p in range(len(like)):
        assert torch.equal(got[p], single[p]), (name, C, p)


def test_wrappers_refuse_what_they_cannot_pass_on():
    from cbench_basic_amd.nn import kernels as K
    pictures, _ = _device_pictures(3, KINDS)
    with pytest.raises(ValueError):
        K.image_tiles_gather(pictures, [], 8, 8)
    with pytest.raises(ValueError):
        K.image_tiles_gather(pictures + _device_pictures(1, KINDS)[0], [(0, 0, 0, 0), (5, 0, 0, 0)], 8, 8)     # two channel counts
    with pytest.raises(TypeError):
        K.image_tiles_gather([pictures[0].float()], [(0, 0, 0, 0)], 8, 8)
    with pytest.raises(ValueError):
        K.image_tiles_scatter(torch.zeros(2, 3, 8, 8, device="cuda"), pictures, [(0, 0, 0, 0)], 8, 8)         # two tiles, one row
    with pytest.raises(ValueError):
        K.image_tiles_scatter(torch.zeros(1, 3, 8, 8, device="cuda"), [pictures[0][:, :, :, ::2]], [(0, 0, 0, 0)], 8, 4)   # a strided canvas
    # a picture with other strides is read through a contiguous copy
    odd = pictures[0][:, :, :, ::2]
    assert K.image_layout_of(odd) is None
    got = K.image_tiles_gather([odd], [(0, 0, 4, 4)], 8, 8)
    assert torch.equal(got.cpu(), odd.cpu()[..., 4:12, 4:12].float().div(255))      # the yardstick is the CPU's division


def test_refusals_come_before_any_copy_or_launch():
    """Arguments only: every call below is refused on the host.  The batch, the picture and the table workspace keep their sentinel
    bytes, and the path report keeps the value of the last accepted call."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    L = _lib.lib()
    C, H, W, n = 3, 16, 24, 2
    img = torch.full((1, C, H, W), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = torch.full((n * 32 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    f32 = torch.full((n * C * 12 * 16 + 4,), 7.0, device="cuda")
    K.image_tiles_gather([img], [(0, 0, 0, 0)], 8, 8)
    before = K.image_tiles_last_path()
    stream = K._stream()

    def table(**change):
        t = np.zeros(n, dtype=K._TILE_REF)
        for k in range(n):
            t[k] = (img.data_ptr(), H, W, 8 * k, 8 * k, _lib.IMAGE_CHW, 0)
        for field, value in change.items():
            t[field][1] = value
        return t

    def gather(t=None, n_=n, channels=C, th=8, tw=8, ws_=None, dst=None, null_table=False):
        t = table() if t is None else t
        return L.basic_image_tiles_gather_u8_to_f32_dev(None if null_table else t.ctypes.data, n_, channels, th, tw,
                                                        ws.data_ptr() if ws_ is None else ws_, f32.data_ptr() if dst is None else dst, stream)

    def scatter(t=None, n_=n, channels=C, th=8, tw=8, sh=12, sw=16, ws_=None, src=None, null_table=False):
        t = table() if t is None else t
        return L.basic_image_tiles_scatter_f32_to_u8_dev(f32.data_ptr() if src is None else src, sh, sw, channels, th, tw,
                                                         None if null_table else t.ctypes.data, n_, ws.data_ptr() if ws_ is None else ws_, stream)
    BIG = 1 << 20
    cases = {
        "null table": dict(null_table=True), "null workspace": dict(ws_=0), "null batch": dict(dst=0), "null picture": dict(t=table(img=0)),
        "n = 0": dict(n_=0), "n < 0": dict(n_=-1), "channels = 0": dict(channels=0), "th = 0": dict(th=0), "tw < 0": dict(tw=-8),
        "img_h = 0": dict(t=table(img_h=0)), "img_w < 0": dict(t=table(img_w=-24)), "layout": dict(t=table(layout=2)),
        "y0 < 0": dict(t=table(y0=-1)), "x0 < 0": dict(t=table(x0=-4)), "bottom": dict(t=table(y0=9)), "right": dict(t=table(x0=17)),
        "float alignment": dict(dst=f32.data_ptr() + 2), "workspace alignment": dict(ws_=ws.data_ptr() + 4),
        "2^40 samples": dict(th=BIG, tw=BIG + 4),
    }
    for name, kw in cases.items():
        assert gather(**kw) == _lib.ERR_INVALID, name
        assert "image_tiles_gather_u8_to_f32" in _lib.last_error(), (name, _lib.last_error())
        kw = {("src" if k == "dst" else k): v for k, v in kw.items()}
        if name == "2^40 samples":
            kw = dict(sh=BIG, sw=BIG + 4)
        assert scatter(**kw) == _lib.ERR_INVALID, name
        assert "image_tiles_scatter_f32_to_u8" in _lib.last_error(), (name, _lib.last_error())
    for name, kw in {"sh < th": dict(sh=7), "sw < tw": dict(sw=4), "sh = 0": dict(sh=0), "sw < 0": dict(sw=-16)}.items():
        assert scatter(**kw) == _lib.ERR_INVALID, name
    with pytest.raises(ValueError):          # through the front-end: a ValueError
        K.image_tiles_gather([img], [(0, 0, 9, 0)], 8, 8)
    with pytest.raises(ValueError):
        K.image_tiles_scatter(f32[:C * 64].view(1, C, 8, 8), [img], [(0, 0, 0, 17)], 8, 8)
    torch.cuda.synchronize()
    assert K.image_tiles_last_path() == before
    assert bool((img == SENTINEL).all()) and bool((ws == SENTINEL).all()) and bool((f32 == 7.0).all())
    assert gather() == _lib.OK and scatter() == _lib.OK                       # the same arguments unchanged are accepted
    torch.cuda.synchronize()
