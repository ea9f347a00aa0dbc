"""The distortion of 8-bit pictures on the GPU: basic_image_sse_u8_dev (csrc/image.hip, include/basic_hip.h section 8b) against numpy's
int64 sum, EQUAL in every layout combination, path and alignment; what it leaves around its output; its refusals; ms_ssim_per_image_u8
against its definition; the exact PSNR against the float kernel's within that kernel's own error bound; and the harness and the tool
measuring, handing out and writing the very picture they decoded."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, C, H, W): smallest; sample by sample, odd everything; CHW planes of 9 bytes (dwords straddle channels and images); the wide paths;
# HWC with four channels; a channel count without a wide HWC variant
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (2, 3, 3, 3), (3, 3, 16, 20), (1, 4, 8, 8), (2, 2, 4, 6)]
LAYOUTS = ["chw", "hwc"]
COMBOS = [(la, lb) for la in LAYOUTS for lb in LAYOUTS]
POISON = 0x5A5A5A5A5A5A5A5A
GUARD = 8


def _K():
    from cbench_basic_amd.nn import kernels as K
    return K


def _np_sse(a, b):
    return ((a.numpy().astype(np.int64) - b.numpy().astype(np.int64)) ** 2).sum((2, 3))


def _pair(shape, seed=None):
    """Two uint8 batches whose images (and channels) all differ in content and in error."""
    g = torch.Generator().manual_seed(sum(shape) if seed is None else seed)
    a = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    b = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    return a, b


def _on_device(chw, layout, off=0):
    """The [B, C, H, W] values on the GPU with memory in `layout`, the first sample `off` bytes into a larger buffer."""
    B, C, H, W = chw.shape
    mem = (chw if layout == "chw" else chw.permute(0, 2, 3, 1)).contiguous().reshape(-1)
    big = torch.full((mem.numel() + 16,), 0xC3, dtype=torch.uint8)
    big[off:off + mem.numel()] = mem
    flat = big.cuda()[off:off + mem.numel()]
    assert flat.data_ptr() % 4 == off % 4
    return flat.view(B, C, H, W) if layout == "chw" else flat.view(B, H, W, C).permute(0, 3, 1, 2)


def _raw(a, la, b, lb, shape, out_ptr):
    from cbench_basic_amd import _lib
    K = _K()
    B, C, H, W = shape
    return _lib.lib().basic_image_sse_u8_dev(a.data_ptr(), K.IMAGE_LAYOUTS[la], b.data_ptr(), K.IMAGE_LAYOUTS[lb], B, C, H, W, out_ptr,
                                             torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- the kernel against numpy, exactly
@pytest.mark.parametrize("la,lb", COMBOS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sse_equals_numpy_in_every_layout_and_alignment(shape, la, lb):
    K = _K()
    a, b = _pair(shape)
    want = _np_sse(a, b)
    if shape[0] * shape[1] > 1 and shape[2] * shape[3] > 1:
        assert len(set(want.reshape(-1).tolist())) == want.size            # no two sums alike: a swapped destination shows
    # (0, 0): the wide path where the shape has one; then each pointer 1, 2 and 3 bytes off a dword, and both
    for off_a, off_b in [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 2)]:
        da, db = _on_device(a, la, off_a), _on_device(b, lb, off_b)
        assert K.image_layout_of(da) in (la, "chw") and K.image_layout_of(db) in (lb, "chw")
        got = K.image_sse_u8(da, db)
        assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == shape[:2]
        assert np.array_equal(got.cpu().numpy(), want), (shape, la, lb, off_a, off_b, got.cpu().tolist(), want.tolist())


@pytest.mark.parametrize("la,lb", COMBOS)
@pytest.mark.parametrize("shape", [(1, 1, 272, 256), (2, 3, 160, 176), (1, 3, 272, 256)])
def test_saturated_sums_pass_32_bits(shape, la, lb):
    """All-255 against all-0: every square is 65,025.  1x1x272x256 is 69,632 samples, 4,527,820,800 > 2^32 in one sum; 2x3x160x176
    crosses 2^32 within an image (84,480 samples of three channels), 1x3x272x256 within every channel of an interleaved image."""
    K = _K()
    a, b = torch.full(shape, 255, dtype=torch.uint8), torch.zeros(shape, dtype=torch.uint8)
    per_channel = 65025 * shape[2] * shape[3]
    if shape[1] == 1:
        assert per_channel == 4527820800 and per_channel > 2 ** 32
    assert per_channel * shape[1] > 2 ** 32
    for x, y in ((a, b), (b, a)):
        got = K.image_sse_u8(_on_device(x, la), _on_device(y, lb)).cpu().numpy()
        assert got.shape == shape[:2] and bool((got == per_channel).all()), (shape, la, lb, got.tolist(), per_channel)
    got = K.image_sse_u8(_on_device(a, la, 1), _on_device(b, lb, 2)).cpu().numpy()       # sample by sample: the same integers
    assert bool((got == per_channel).all())


def test_sse_grid_stride_and_every_path_agree():
    """A batch large enough that workgroups share planes and images (more than one workgroup per destination, more than one pass of a
    lane): all layout combinations and the sample-by-sample path give numpy's integers."""
    K = _K()
    shape = (3, 3, 96, 100)
    a, b = _pair(shape)
    want = _np_sse(a, b)
    for la, lb in COMBOS:
        assert np.array_equal(K.image_sse_u8(_on_device(a, la), _on_device(b, lb)).cpu().numpy(), want), (la, lb)
    assert np.array_equal(K.image_sse_u8(_on_device(a, "chw", 3), _on_device(b, "hwc", 0)).cpu().numpy(), want)
    assert np.array_equal(K.image_sse_u8(_on_device(a, "hwc", 0), _on_device(b, "hwc", 2)).cpu().numpy(), want)


def test_more_destinations_than_a_grid_dimension():
    """More than 65,535 planes, and more than 65,535 images: a workgroup then walks several destinations, one atomic each."""
    K = _K()
    for shape in ((70000, 1, 1, 3), (66000, 3, 2, 2)):
        g = torch.Generator().manual_seed(shape[0])
        a = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        b = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        want = _np_sse(a, b)
        for la, lb in COMBOS:
            assert np.array_equal(K.image_sse_u8(_on_device(a, la), _on_device(b, lb)).cpu().numpy(), want), (shape, la, lb)
        assert np.array_equal(K.image_sse_u8(_on_device(a, "chw", 1), _on_device(b, "hwc", 2)).cpu().numpy(), want), shape


def test_offsets_past_two_to_the_31():
    """More than 2^31 samples in one call (element offsets are 64-bit): one plane by dwords, the same sample by sample, and four pixels
    per lane of three interleaved channels.  The inputs are made on the device; the reference is the same integer sum in torch ops
    there, in pieces that fit int32 intermediates."""
    K = _K()
    if torch.cuda.get_device_properties(0).total_memory < 32 * 2 ** 30:
        pytest.skip("needs 16 GiB of device memory beside what the other tests hold")

    def reference(a, b, piece=2 ** 27):      # a, b: [rows, channels] views -> int64 [channels]
        total = torch.zeros(a.shape[1], dtype=torch.int64, device="cuda")
        for i in range(0, a.shape[0], piece):
            d = a[i:i + piece].int() - b[i:i + piece].int()
            total += (d * d).sum(0, dtype=torch.int64)
        return total.cpu()
    shape = (1, 1, 2 ** 16 + 1, 2 ** 15)
    n = shape[2] * shape[3]
    assert n > 2 ** 31
    big_a = torch.randint(0, 256, (n + 4,), dtype=torch.uint8, device="cuda")
    big_b = torch.randint(0, 256, (n + 4,), dtype=torch.uint8, device="cuda")
    for off in (0, 1):
        a, b = big_a[off:off + n], big_b[off:off + n]
        got = K.image_sse_u8(a.view(shape), b.view(shape)).cpu()
        assert torch.equal(got.view(-1), reference(a.view(-1, 1), b.view(-1, 1))), off
    del big_a, big_b, a, b
    H = W = 2 ** 15      # 3 x 2^30 samples over [H][W][C] memory
    a = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device="cuda")
    b = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device="cuda")
    want = reference(a.view(H * W, 3), b.view(H * W, 3))
    assert torch.equal(K.image_sse_u8(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)).cpu().view(-1), want)
    planes = b.permute(0, 3, 1, 2).contiguous()      # the same values as planes: the mixed pair
    assert torch.equal(K.image_sse_u8(a.permute(0, 3, 1, 2), planes).cpu().view(-1), want)


@pytest.mark.parametrize("la,lb", COMBOS)
def test_output_is_fully_overwritten_and_nothing_else(la, lb):
    from cbench_basic_amd import _lib
    poison = torch.tensor(POISON, dtype=torch.int64)
    for shape in ((2, 3, 3, 3), (3, 3, 16, 20), (2, 2, 4, 6)):
        n = shape[0] * shape[1]
        a, b = _pair(shape)
        a2, b2 = _pair(shape, seed=99)
        buf = torch.full((GUARD + n + GUARD,), POISON, dtype=torch.int64, device="cuda")
        for x, y in ((a, b), (a2, b2)):          # two calls in a row on one buffer: the second starts from the first's sums
            _lib.check(_raw(_on_device(x, la), la, _on_device(y, lb), lb, shape, buf[GUARD:].data_ptr()))
            got = buf.cpu()
            assert np.array_equal(got[GUARD:GUARD + n].numpy().reshape(shape[:2]), _np_sse(x, y)), (shape, la, lb)
            assert bool((got[:GUARD] == poison).all()) and bool((got[GUARD + n:] == poison).all())
    # identical pictures: zeros are written too
    buf = torch.full((GUARD + 6 + GUARD,), POISON, dtype=torch.int64, device="cuda")
    a, _ = _pair((2, 3, 5, 7))
    _lib.check(_raw(_on_device(a, la), la, _on_device(a, lb), lb, (2, 3, 5, 7), buf[GUARD:].data_ptr()))
    assert bool((buf.cpu()[GUARD:GUARD + 6] == 0).all()) and bool((buf.cpu()[:GUARD] == poison).all())


def test_refusals_launch_nothing():
    from cbench_basic_amd import _lib
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    a = torch.zeros(256, dtype=torch.uint8, device="cuda")
    b = torch.ones(256, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), POISON, dtype=torch.int64, device="cuda")
    pa, pb, po = a.data_ptr(), b.data_ptr(), out.data_ptr()
    good = (pa, 0, pb, 1, 1, 3, 4, 4, po)
    cases = {"batch 0": (pa, 0, pb, 1, 0, 3, 4, 4, po), "channels -1": (pa, 0, pb, 1, 1, -1, 4, 4, po), "h 0": (pa, 0, pb, 1, 1, 3, 0, 4, po),
             "w -4": (pa, 0, pb, 1, 1, 3, 4, -4, po), "null a": (None, 0, pb, 1, 1, 3, 4, 4, po), "null b": (pa, 0, None, 1, 1, 3, 4, 4, po),
             "null sse": (pa, 0, pb, 1, 1, 3, 4, 4, None), "layout a": (pa, 2, pb, 1, 1, 3, 4, 4, po), "layout b": (pa, 0, pb, -1, 1, 3, 4, 4, po),
             "sse alignment": (pa, 0, pb, 1, 1, 3, 4, 4, po + 4), "2^40 samples": (pa, 0, pb, 1, 1 << 20, 1 << 10, 1 << 10, 1 << 10, po)}
    for name, args in cases.items():
        assert L.basic_image_sse_u8_dev(*args, st) == _lib.ERR_INVALID, name
        with pytest.raises(ValueError, match="image_sse_u8"):
            _lib.check(L.basic_image_sse_u8_dev(*args, st))
    assert bool((out.cpu() == torch.tensor(POISON, dtype=torch.int64)).all())         # not even cleared
    _lib.check(L.basic_image_sse_u8_dev(*good, st))
    assert out.cpu()[:3].tolist() == [16, 16, 16] and int(out.cpu()[3]) == POISON


def test_python_front_end():
    from cbench_basic_amd import _lib
    K = _K()
    a, b = _pair((2, 3, 8, 12))
    want = _np_sse(a, b)
    da, db = a.cuda(), b.cuda()
    assert np.array_equal(K.image_sse_u8(da, db.contiguous(memory_format=torch.channels_last)).cpu().numpy(), want)
    # no layout of its own (strided, cropped): made contiguous
    assert np.array_equal(K.image_sse_u8(da[:, :, :, ::2], db[:, :, :, ::2]).cpu().numpy(), _np_sse(a[:, :, :, ::2], b[:, :, :, ::2]))
    assert np.array_equal(K.image_sse_u8(da[:, :, 1:7, :5], db[:, :, 1:7, :5]).cpu().numpy(), _np_sse(a[:, :, 1:7, :5], b[:, :, 1:7, :5]))
    with pytest.raises(TypeError):
        K.image_sse_u8(da.float(), db)
    with pytest.raises(TypeError):
        K.image_sse_u8(da, db.int())
    with pytest.raises(ValueError):
        K.image_sse_u8(da, db[:, :, :4])
    with pytest.raises(ValueError):
        K.image_sse_u8(da[0], db[0])
    with pytest.raises(_lib.BasicHipError, match="no CPU fallback"):
        K.image_sse_u8(a, db)
    with pytest.raises(_lib.BasicHipError, match="no CPU fallback"):
        K.image_sse_u8(da, b)
    with pytest.raises(TypeError):
        K.mse_per_image(da, db)               # the float entry still refuses bytes


# ---------------------------------------------------------------- MS-SSIM of uint8 pairs: the float kernel on the converted pair
def test_ms_ssim_u8_is_the_float_kernel_on_the_converted_pair():
    K = _K()
    shape = (1, 3, 176, 192)
    a, _ = _pair(shape)
    g = torch.Generator().manual_seed(4)
    b = (a.int() + torch.randint(-9, 10, shape, generator=g)).clamp(0, 255).to(torch.uint8)
    fa, fb = K.image_u8_to_f32(a.cuda()), K.image_u8_to_f32(b.cuda())
    want, want_terms = K.ms_ssim_per_image(fa, fb, data_range=1.0, return_terms=True)
    assert 0 < float(want[0]) < 1
    for la, lb in COMBOS:
        da, db = _on_device(a, la), _on_device(b, lb)
        got = K.ms_ssim_per_image_u8(da, db)
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32)), (la, lb)      # bit for bit
        got2, terms = K.ms_ssim_per_image_u8(da, db, return_terms=True)
        assert torch.equal(got2.view(torch.int32), want.view(torch.int32)) and tuple(terms.shape) == (1, 3, 5)
        assert torch.equal(terms.view(torch.int32), want_terms.view(torch.int32))
    with pytest.raises(TypeError):
        K.ms_ssim_per_image_u8(fa, db)
    # the metric class takes the same route for a uint8 pair
    from cbench_basic_amd.benchmark import PytorchBatchedDistortion
    r = PytorchBatchedDistortion(metrics=["psnr", "ms-ssim"]).per_item(a.cuda(), b.cuda())
    assert r[0]["ms-ssim"] == float(want[0])


def test_exact_psnr_agrees_with_the_float_kernel_within_its_bound():
    """PSNR from the exact sum against PSNR from mse_per_image of the converted pair.  The bound is the one test_mse_per_image_vs_fp64
    grants the float kernel, 2 (depth + 3) U relative to the mean squared error, here in dB.  (The conversions' own roundings of u / 255
    enter the float figure too; random in sign and weighted by the differences, they come to a small fraction of U on a random pair.)"""
    from test_gpu_entropy_kernels import U, _mse_depth
    from cbench_basic_amd.benchmark import PytorchBatchedDistortion, psnr_from_sse
    K = _K()
    shape = (2, 3, 64, 64)
    a, b = _pair(shape, seed=2024)
    da, db = a.cuda(), b.cuda()
    elems = 3 * 64 * 64
    sse = K.image_sse_u8(da, db).sum(1).cpu()
    assert np.array_equal(sse.numpy(), _np_sse(a, b).sum(1))
    fa, fb = K.image_u8_to_f32(da), K.image_u8_to_f32(db)
    mse = K.mse_per_image(fa, fb).cpu().double()
    for i in range(2):
        aligned = (fa.data_ptr() + 4 * i * elems) % 16 == 0 and (fb.data_ptr() + 4 * i * elems) % 16 == 0
        bound_rel = 2 * (_mse_depth(elems, aligned) + 3) * U
        bound_db = -10 * math.log10(1 - bound_rel)
        exact = psnr_from_sse(int(sse[i]), elems)
        from_float = -10 * math.log10(float(mse[i]))
        print(f"image {i}: exact {exact:.9f} dB, float {from_float:.9f} dB, difference {abs(exact - from_float):.3e} dB, bound {bound_db:.3e} dB")
        assert abs(exact - from_float) <= bound_db
    # and the metric class reports the exact figure for the uint8 pair, the float figure for the float pair
    got = PytorchBatchedDistortion().per_item(da, db, cache_metrics=False)
    assert [r["psnr"] for r in got] == [psnr_from_sse(int(s), elems) for s in sse]
    assert PytorchBatchedDistortion()(da, db)["psnr"] == psnr_from_sse(int(sse.sum()), 2 * elems)
    assert PytorchBatchedDistortion()(da, db)["psnr"] != np.mean([r["psnr"] for r in got])


# ---------------------------------------------------------------- the harness: the picture it measures is the picture it hands out
def _items_u8(n, size=64):
    out = []
    for i in range(n):
        torch.manual_seed(i)
        out.append(torch.randint(0, 256, (1, 3, size, size), dtype=torch.uint8))
    return out


def test_harness_measures_the_picture_it_hands_out(tmp_path):
    from cbench_basic_amd import presets
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion, psnr_from_sse
    K = _K()

    def build():
        return presets.seed_synthetic_weights(presets.hyperprior_codec(), seed=0)
    codec = build().eval().cuda()
    codec.update_state()
    items = _items_u8(3)
    # what a caller gets from the same bytes, and the float figure of today
    pictures, float_psnr = [], []
    for x in items:
        data = codec.compress(x)
        pictures.append(codec.decompress(data, output_dtype=torch.uint8).cpu())
        float_psnr.append(PytorchBatchedDistortion()(codec.decompress(data), K.image_u8_to_f32(x.cuda()), cache_metrics=False)["psnr"])
    want = [psnr_from_sse(int(_np_sse(p, x).sum()), x.numel()) for p, x in zip(pictures, items)]
    assert len(set(want)) == 3 and all(np.isfinite(want))
    assert max(abs(w - f) for w, f in zip(want, float_psnr)) > 1e-6              # the two figures do differ: clamping and rounding

    def run(name, **kw):
        delivered = []
        bench = BasicLosslessCompressionBenchmark(codec, items, distortion_metric=PytorchBatchedDistortion(), output_dir=str(tmp_path / name),
                                                  on_reconstruction=(lambda p, i, x: delivered.append((p, i, x))) if kw.get("metrics_on_uint8") else None,
                                                  **kw)
        metrics = bench.run_benchmark(ignore_exist_metrics=True)
        bench.close()
        return metrics, delivered

    off, none = run("off")
    assert off["_psnr"] == sum(float_psnr) / 3 and none == []
    for name, kw in (("seq", {}), ("coalesced", dict(testing_coalesce_items=3)), ("workers", dict(num_testing_workers=2, codec_builder=build))):
        metrics, delivered = run(name, metrics_on_uint8=True, **kw)
        assert [(p, i) for p, i, _ in delivered] == [("", 0), ("", 1), ("", 2)], name                      # every index once
        for (_, i, x), p in zip(delivered, pictures):
            assert x.dtype == torch.uint8 and x.is_cuda and torch.equal(x.cpu(), p), (name, i)     # the separate decompress of the same bytes
        each = [psnr_from_sse(int(_np_sse(x.cpu(), item).sum()), item.numel()) for (_, _, x), item in zip(delivered, items)]
        assert each == want, name
        if name == "workers":      # the workers' partial sums are merged: another order of the same additions
            assert abs(metrics["_psnr"] - sum(want) / 3) <= 1e-12 * abs(metrics["_psnr"])
        else:
            assert metrics["_psnr"] == sum(want) / 3, name
        assert metrics["_original_length"] == 3 * 64 * 64 and metrics["_compressed_length"] == off["_compressed_length"]


def test_tool_writes_the_pictures_it_measured(tmp_path, capsys):
    Image = pytest.importorskip("PIL.Image")
    from cbench_basic_amd.benchmark import psnr_from_sse
    from cbench_basic_amd.data import RandomImageDataset
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "run_benchmark.py")
    spec = importlib.util.spec_from_file_location("run_benchmark_tool_u8", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "pictures"
    metrics = tool.main(["--uint8", "--metrics-on-uint8", "--save-reconstructions", str(out), "--complexity-levels", "0", "7", "--codec", "basic",
                         "--synthetic", "2", "--size", "64", "--out", str(tmp_path / "run")])
    assert "4 reconstructions written" in capsys.readouterr().out
    ds = RandomImageDataset(num=2, size=(3, 64, 64), dtype=torch.uint8)
    assert sorted(os.listdir(out)) == ["sclevel0", "sclevel7"]                # one folder per level, nothing beside them
    for level in (0, 7):
        folder = out / f"sclevel{level}"
        assert sorted(os.listdir(folder)) == ["00000.png", "00001.png"]
        each = []
        for i in range(2):
            picture = np.asarray(Image.open(str(folder / f"{i:05d}.png")))
            assert picture.dtype == np.uint8 and picture.shape == (64, 64, 3)
            item = ds[i].permute(1, 2, 0).numpy()
            sse = int(((picture.astype(np.int64) - item.astype(np.int64)) ** 2).sum())
            each.append(psnr_from_sse(sse, item.size))
        assert metrics[f"sclevel{level}_psnr"] == sum(each) / 2, (level, each)
