"""The 8-bit image kernels (csrc/image.hip, include/basic_hip.h section 8b) against torch on the CPU, exactly:
uint8 -> float32 is ``u.float().div(255)`` bit for bit, float32 -> uint8 is
``torch.nan_to_num(x, nan=0.0).clamp(0, 1).mul(255).round().to(torch.uint8)``, for both layouts of the uint8 side, every path the
library takes (wide / sample by sample, by shape and by the alignment of either pointer) and with guard bands around the
destination."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, C, H, W): one pixel; one channel and an odd row; odd everything (sample by sample when HWC); four channels; h * w % 4 == 0
# with three channels (the wide HWC path, more than one image); a row that is no multiple of four
SHAPES = [(1, 3, 1, 1), (1, 1, 3, 17), (2, 3, 5, 7), (2, 4, 2, 4), (3, 3, 16, 20), (1, 3, 2, 129)]
LAYOUTS = ["chw", "hwc"]
GUARD = 64          # bytes / floats of sentinel on either side; a multiple of 16 bytes, so an offset of 0 keeps the wide path
SENTINEL_F, SENTINEL_U = -7.5, 0xA5


def _cpu_quantise(x):
    return torch.nan_to_num(x, nan=0.0).clamp(0, 1).mul(255).round().to(torch.uint8)


def _as_layout(chw, layout):
    """[B, C, H, W] values -> the flat memory image of the uint8 side in `layout`."""
    return (chw if layout == "chw" else chw.permute(0, 2, 3, 1)).contiguous().reshape(-1)


def _view(flat, shape, layout):
    """A [B, C, H, W] view of flat memory in `layout`."""
    B, C, H, W = shape
    return flat.view(B, C, H, W) if layout == "chw" else flat.view(B, H, W, C).permute(0, 3, 1, 2)


def _u8_to_f32_raw(src_view, layout, shape, dst_flat):
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    B, C, H, W = shape
    _lib.check(_lib.lib().basic_image_u8_to_f32_dev(src_view.data_ptr(), K.IMAGE_LAYOUTS[layout], B, C, H, W, dst_flat.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream))


def _f32_to_u8_raw(src, shape, layout, dst_flat):
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    B, C, H, W = shape
    _lib.check(_lib.lib().basic_image_f32_to_u8_dev(src.data_ptr(), B, C, H, W, K.IMAGE_LAYOUTS[layout], dst_flat.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream))


def test_all_256_values_and_the_round_trip():
    from cbench_basic_amd.nn import kernels as K
    u = torch.arange(256, dtype=torch.uint8)
    want = u.float().div(255)
    for shape in ((1, 1, 1, 256), (1, 1, 256, 1), (256, 1, 1, 1), (1, 4, 8, 8)):
        f = K.image_u8_to_f32(u.view(shape).cuda())
        assert f.dtype == torch.float32 and tuple(f.shape) == shape
        assert torch.equal(f.cpu().view(-1).view(torch.int32), want.view(torch.int32)), shape     # bit for bit
        for layout in LAYOUTS:
            back = K.image_f32_to_u8(f, layout=layout)
            assert back.dtype == torch.uint8 and tuple(back.shape) == shape and K.image_layout_of(back) in (layout, "chw")
            assert torch.equal(back.cpu(), u.view(shape)), (shape, layout)
    # sample by sample (the source three bytes off a dword) gives the same 256 floats
    big = torch.zeros(256 + 8, dtype=torch.uint8)
    big[3:259] = u
    f = K.image_u8_to_f32(big.cuda()[3:259].view(1, 1, 1, 256))
    assert torch.equal(f.cpu().view(-1).view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_u8_to_f32_layouts_shapes_offsets_and_guards(shape, layout):
    from cbench_basic_amd.nn import kernels as K
    B, C, H, W = shape
    n = B * C * H * W
    g = torch.Generator().manual_seed(n)
    u = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    want = u.float().div(255)
    mem = _as_layout(u, layout)
    results = []
    for off in (0, 1, 2, 3):                      # the source as a view into a larger buffer: 0 keeps the wide path where the shape allows
        big = torch.full((n + 16,), 0x5A, dtype=torch.uint8)
        big[off:off + n] = mem
        src = _view(big.cuda()[off:off + n], shape, layout)
        assert K.image_layout_of(src) in (layout, "chw")
        out = K.image_u8_to_f32(src)
        assert tuple(out.shape) == shape and out.is_contiguous()
        assert torch.equal(out.cpu(), want), (shape, layout, off)
        results.append(out)
        # the same call with guard bands around the destination; dst_off 1: the float side off its 16 bytes (sample by sample)
        for dst_off in (0, 1):
            dst = torch.full((GUARD + n + GUARD + 1,), SENTINEL_F, dtype=torch.float32, device="cuda")
            _u8_to_f32_raw(src, layout, shape, dst[GUARD + dst_off:])
            got = dst.cpu()
            assert torch.equal(got[GUARD + dst_off:GUARD + dst_off + n].view(shape), want), (shape, layout, off, dst_off)
            assert bool((got[:GUARD + dst_off] == SENTINEL_F).all()) and bool((got[GUARD + dst_off + n:] == SENTINEL_F).all())
    assert all(torch.equal(results[0], r) for r in results[1:])       # aligned and unaligned paths agree


def _special_floats():
    """[every float32 whose low 16 bits are zero | the neighbourhoods of the 255 rounding ties | 2^20 uniform values]"""
    hi = (torch.arange(65536, dtype=torch.int64) << 16)
    hi = torch.where(hi >= 2 ** 31, hi - 2 ** 32, hi).to(torch.int32).view(torch.float32)
    k = torch.arange(255, dtype=torch.float64)
    tie = ((k + 0.5) / 255).to(torch.float32)                       # the fp32 nearest (k + 0.5) / 255
    ties = (tie.view(torch.int32)[:, None] + torch.arange(-2, 3, dtype=torch.int32)[None, :]).reshape(-1).view(torch.float32)
    g = torch.Generator().manual_seed(7)
    uni = torch.rand(2 ** 20, generator=g) * 1.5 - 0.25
    return hi, ties, uni


def test_f32_to_u8_special_values():
    from cbench_basic_amd.nn import kernels as K
    hi, ties, uni = _special_floats()
    assert hi.numel() == 65536 and bool(torch.isnan(hi).any()) and bool(torch.isinf(hi).any()) and ties.numel() == 255 * 5
    assert int((hi.abs() < 1.1754944e-38).sum()) > 200              # denormals and both zeros
    for name, x in (("patterns", hi), ("ties", ties), ("uniform", uni)):
        want = _cpu_quantise(x)
        for shape in ((1, 1, 1, x.numel()), (1, 1, x.numel(), 1)):
            got = K.image_f32_to_u8(x.view(shape).cuda())
            assert got.dtype == torch.uint8
            bad = (got.cpu().view(-1) != want).nonzero().view(-1)
            assert bad.numel() == 0, (name, x[bad[:4]].tolist(), got.cpu().view(-1)[bad[:4]].tolist(), want[bad[:4]].tolist())
    q = _cpu_quantise(ties).view(255, 5).int()
    assert bool(((q[:, 4] - q[:, 0]) == 1).all())                   # every neighbourhood does straddle its rounding boundary
    # three interleaved channels of the same values, wide (h * w % 4 == 0) and sample by sample (one row short)
    for hgt in (2 ** 12, 2 ** 12 - 1):
        x = uni[:3 * 85 * hgt].view(1, 3, hgt, 85)
        got = K.image_f32_to_u8(x.cuda(), layout="hwc")
        assert K.image_layout_of(got) == "hwc" and torch.equal(got.cpu(), _cpu_quantise(x)), hgt


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_f32_to_u8_layouts_shapes_offsets_and_guards(shape, layout):
    from cbench_basic_amd.nn import kernels as K
    B, C, H, W = shape
    n = B * C * H * W
    g = torch.Generator().manual_seed(1000 + n)
    x = torch.rand(shape, generator=g) * 1.5 - 0.25
    x.view(-1)[::5] = (torch.randint(0, 255, (len(x.view(-1)[::5]),), generator=g).float() + 0.5) / 255    # ties among them
    x.view(-1)[0] = float("nan")
    want = _cpu_quantise(x)
    out = K.image_f32_to_u8(x.cuda(), layout=layout)
    assert tuple(out.shape) == shape and K.image_layout_of(out) in (layout, "chw")
    assert torch.equal(out.cpu(), want), (shape, layout)
    mem = _as_layout(want, layout)
    xs = torch.full((n + 8,), 0.5, dtype=torch.float32, device="cuda")
    for src_off in (0, 1):                        # 1: the float side off its 16 bytes
        src = xs[src_off:src_off + n]
        src.copy_(x.view(-1))
        for off in (0, 1, 2, 3):
            dst = torch.full((GUARD + n + GUARD + 3,), SENTINEL_U, dtype=torch.uint8, device="cuda")
            _f32_to_u8_raw(src, shape, layout, dst[GUARD + off:])
            got = dst.cpu()
            assert torch.equal(got[GUARD + off:GUARD + off + n], mem), (shape, layout, src_off, off)
            assert bool((got[:GUARD + off] == SENTINEL_U).all()) and bool((got[GUARD + off + n:] == SENTINEL_U).all())


def test_offsets_past_two_to_the_31():
    """More than 2^31 samples in one call (element offsets are 64-bit): flat wide, sample by sample, and the wide HWC path.  The
    inputs are made on the device; windows at the start, across 2^31 and at the end of every plane are compared on the CPU."""
    from cbench_basic_amd.nn import kernels as K
    if torch.cuda.get_device_properties(0).total_memory < 32 * 2 ** 30:
        pytest.skip("needs 18 GiB of device memory beside what the other tests hold")
    win = 4096

    def windows(n):
        return [(0, win), (2 ** 31 - win, 2 ** 31 + win), (n - win, n)] if n > 2 ** 31 + win else [(0, win), (n // 2 - win, n // 2 + win), (n - win, n)]
    # flat: [1, 1, 2^16 + 1, 2^15], from an aligned and from a byte-shifted source
    shape = (1, 1, 2 ** 16 + 1, 2 ** 15)
    n = shape[2] * shape[3]
    big = torch.randint(0, 256, (n + 4,), dtype=torch.uint8, device="cuda")
    for off in (0, 1):
        src = big[off:off + n]
        f = K.image_u8_to_f32(src.view(shape)).view(-1)
        for a, b in windows(n):
            assert torch.equal(f[a:b].cpu(), src[a:b].cpu().float().div(255)), (off, a)
        if off == 0:
            back = K.image_f32_to_u8(f.view(shape)).view(-1)
            for a, b in windows(n):
                assert torch.equal(back[a:b].cpu(), src[a:b].cpu()), a
            del back
        del f
    del big
    # three interleaved channels: [1, 3, 2^15, 2^15] over [H][W][C] memory, 3 x 2^30 samples
    H = W = 2 ** 15
    P = H * W
    hwc = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device="cuda")
    f = K.image_u8_to_f32(hwc.permute(0, 3, 1, 2))
    flat_f, flat_u = f.view(3, P), hwc.view(P, 3)
    for a, b in windows(P):
        assert torch.equal(flat_f[:, a:b].cpu(), flat_u[a:b].cpu().t().float().div(255)), a
    back = K.image_f32_to_u8(f, layout="hwc")
    assert K.image_layout_of(back) == "hwc"
    flat_b = back.permute(0, 2, 3, 1).reshape(P, 3)
    for a, b in windows(P):
        assert torch.equal(flat_b[a:b].cpu(), flat_u[a:b].cpu()), a


def test_python_front_ends_take_any_dense_or_strided_tensor():
    from cbench_basic_amd.nn import kernels as K
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 256, (2, 3, 8, 12), dtype=torch.uint8, generator=g)
    want = u.float().div(255)
    assert torch.equal(K.image_u8_to_f32(u.cuda().contiguous(memory_format=torch.channels_last)).cpu(), want)
    assert torch.equal(K.image_u8_to_f32(u.cuda()[:, :, :, ::2]).cpu(), want[:, :, :, ::2])      # no layout: made contiguous
    with pytest.raises(TypeError):
        K.image_u8_to_f32(u.cuda().float())
    with pytest.raises(TypeError):
        K.image_f32_to_u8(u.cuda())
    with pytest.raises(ValueError):
        K.image_f32_to_u8(want.cuda(), layout="nhwc")
    from cbench_basic_amd import _lib
    with pytest.raises(_lib.BasicHipError):
        K.image_u8_to_f32(u)                                                                      # a host tensor: no CPU path


def test_bad_arguments_are_invalid_and_launch_nothing():
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.full((64,), SENTINEL_F, dtype=torch.float32, device="cuda")
    for args in ((src.data_ptr(), 0, 0, 3, 4, 4, dst.data_ptr()), (src.data_ptr(), 0, 1, 3, 0, 4, dst.data_ptr()),
                 (src.data_ptr(), 0, 1, -3, 4, 4, dst.data_ptr()), (src.data_ptr(), 0, 1, 3, 4, -4, dst.data_ptr()),
                 (src.data_ptr(), 2, 1, 3, 4, 4, dst.data_ptr()), (None, 0, 1, 3, 4, 4, dst.data_ptr()),
                 (src.data_ptr(), 1, 1, 3, 4, 4, None)):
        assert L.basic_image_u8_to_f32_dev(*args, st) == _lib.ERR_INVALID, args
        assert _lib.last_error()
        with pytest.raises(ValueError):
            _lib.check(L.basic_image_u8_to_f32_dev(*args, st))
    assert bool((dst.cpu() == SENTINEL_F).all())
    fsrc = torch.zeros(64, dtype=torch.float32, device="cuda")
    bdst = torch.full((64,), SENTINEL_U, dtype=torch.uint8, device="cuda")
    for args in ((fsrc.data_ptr(), 0, 3, 4, 4, 0, bdst.data_ptr()), (fsrc.data_ptr(), 1, 3, 4, 4, 5, bdst.data_ptr()),
                 (None, 1, 3, 4, 4, 0, bdst.data_ptr()), (fsrc.data_ptr(), 1, 3, 4, 4, 1, None)):
        assert L.basic_image_f32_to_u8_dev(*args, st) == _lib.ERR_INVALID, args
    assert bool((bdst.cpu() == SENTINEL_U).all())
    with pytest.raises(ValueError):
        K.image_u8_to_f32(torch.zeros(1, 3, 0, 4, dtype=torch.uint8, device="cuda"))
