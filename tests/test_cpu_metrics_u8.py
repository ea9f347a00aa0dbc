"""The distortion of 8-bit pictures without a GPU: ``psnr_from_sse`` against values worked out by hand, ``PytorchBatchedDistortion`` on
uint8 pairs on the CPU against numpy (int64 sums, float64 logarithms), float pairs against the arithmetic they always went through, and
the harness with ``metrics_on_uint8=True`` around a stub codec: the metric meets uint8 pairs and ``on_reconstruction`` gets every
item's picture once, after the pass."""
import math

import numpy as np
import pytest
import torch

from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion, psnr_from_sse


def _np_sse(a, b):
    return ((a.numpy().astype(np.int64) - b.numpy().astype(np.int64)) ** 2).sum((2, 3))


def _np_psnr(sse, samples):
    return float(10.0 * np.log10(np.float64(255.0) ** 2 * np.float64(samples) / np.float64(sse)))


def _pair(shape, seed, pad=0):
    g = torch.Generator().manual_seed(seed)
    target = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    noise = torch.randint(-6, 7, shape, generator=g) * (1 + torch.arange(shape[0]).view(-1, 1, 1, 1))   # every image its own error
    output = (target.int() + noise).clamp(0, 255).to(torch.uint8)
    if pad:
        output = torch.nn.functional.pad(output, (0, pad, 0, pad), value=77)
    return output, target


# ---------------------------------------------------------------- psnr_from_sse
def test_psnr_from_sse_by_hand():
    assert psnr_from_sse(0, 100) == math.inf and psnr_from_sse(0, 1, peak=1.0) == math.inf
    # mse 65.025 = 255^2 / 1000: 30 dB; mse 1: 20 log10(255); mse 255^2 (all-0 against all-255): 0 dB
    assert abs(psnr_from_sse(65025, 1000) - 30.0) < 1e-12
    assert abs(psnr_from_sse(100, 100) - 48.13080360867910) < 1e-12
    assert psnr_from_sse(4527820800, 69632) == 0.0
    assert abs(psnr_from_sse(1, 100, peak=1.0) - 20.0) < 1e-12
    assert isinstance(psnr_from_sse(3, 7), float)
    # float64 all the way: one squared error in 2^40 samples is not lost
    assert abs(psnr_from_sse(1, 2 ** 40) - (20 * math.log10(255) + 400 * math.log10(2))) < 1e-9
    # arrays, and the batch form (total over total) is not the mean of the per-item form
    each = psnr_from_sse(np.array([100, 400, 0]), 100)
    assert each.dtype == np.float64 and each[2] == math.inf
    assert abs(each[0] - 48.13080360867910) < 1e-12 and abs(each[1] - (48.13080360867910 - 10 * math.log10(4))) < 1e-12
    batch = psnr_from_sse(100 + 400, 2 * 100)
    assert abs(batch - (48.13080360867910 - 10 * math.log10(2.5))) < 1e-12
    assert abs(batch - each[:2].mean()) > 0.9


# ---------------------------------------------------------------- the C ABI entry, as far as it goes without a device
def test_sse_entry_is_declared_exported_and_refuses_before_a_device_is_needed():
    import ctypes
    import os
    import re
    from cbench_basic_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "basic_hip.h")).read()
    assert "basic_image_sse_u8_dev" in re.findall(r"\b(basic_[a-z0-9_]+)\s*\(", header)
    res, args = _lib._SIGNATURES["basic_image_sse_u8_dev"]
    assert res is ctypes.c_int and len(args) == 10
    L = _lib.lib()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    for bad in ((p, 0, p, 0, 0, 3, 4, 4, p), (p, 0, p, 0, 1, 0, 4, 4, p), (p, 0, p, 0, 1, 3, -1, 4, p), (p, 0, p, 0, 1, 3, 4, 0, p),
                (None, 0, p, 0, 1, 3, 4, 4, p), (p, 0, None, 0, 1, 3, 4, 4, p), (p, 0, p, 0, 1, 3, 4, 4, None), (p, 2, p, 0, 1, 3, 4, 4, p),
                (p, 0, p, -1, 1, 3, 4, 4, p), (p, 0, p, 1, 1, 3, 4, 4, p + 4), (p, 1, p, 0, 1 << 20, 1 << 10, 1 << 10, 1 << 10, p)):
        assert L.basic_image_sse_u8_dev(*bad, None) == _lib.ERR_INVALID, bad
        assert "image_sse_u8" in _lib.last_error()
    with pytest.raises(ValueError, match="8-byte"):
        _lib.check(L.basic_image_sse_u8_dev(p, 0, p, 1, 1, 3, 4, 4, p + 1, None))
    assert not buf.any()


# ---------------------------------------------------------------- the metric on CPU uint8 pairs
@pytest.mark.parametrize("max_val", [1.0, 255])
def test_uint8_pair_on_the_cpu_against_numpy(max_val):
    output, target = _pair((3, 3, 10, 14), seed=5, pad=4)          # the output is larger: the metric crops it
    assert tuple(output.shape) == (3, 3, 14, 18)
    sse = _np_sse(output[..., :10, :14], target)
    assert len({int(s) for s in sse.sum(1)}) == 3
    dm = PytorchBatchedDistortion(max_val=max_val)
    got = dm(output, target)
    assert list(got) == ["psnr"] and got["psnr"] == _np_psnr(sse.sum(), target.numel())
    assert dm.collect_metrics() == {"psnr": got["psnr"]}
    items = PytorchBatchedDistortion(max_val=max_val).per_item(output, target)
    assert [r["psnr"] for r in items] == [_np_psnr(s, 3 * 10 * 14) for s in sse.sum(1)]
    assert abs(np.mean([r["psnr"] for r in items]) - got["psnr"]) > 1e-3      # per item is not the batch form
    lists = PytorchBatchedDistortion(max_val=max_val).per_item([output[i:i + 1] for i in range(3)], [target[i:i + 1] for i in range(3)],
                                                               cache_metrics=False)
    assert lists == items
    # the same picture: no error, inf
    assert PytorchBatchedDistortion(max_val=max_val)(target.clone(), target)["psnr"] == math.inf


def test_uint8_pair_refuses_another_peak():
    output, target = _pair((1, 3, 8, 8), seed=1)
    for bad in (0.5, 2.0, 256):
        dm = PytorchBatchedDistortion(max_val=bad)
        with pytest.raises(ValueError, match="255"):
            dm(output, target)
        with pytest.raises(ValueError, match="255"):
            dm.per_item(output, target)
        assert dm.collect_metrics() == {}
        # a float pair still takes any max_val
        assert np.isfinite(dm(output.float() / 255, target.float() / 255)["psnr"])


def test_uint8_ms_ssim_on_the_cpu_is_the_float_restatement_of_u8_over_255():
    from cbench_basic_amd.benchmark.ms_ssim import ms_ssim
    output, target = _pair((2, 1, 176, 168), seed=9)
    want = [float(ms_ssim(output[i:i + 1].float().div(255), target[i:i + 1].float().div(255), data_range=1.0, size_average=False)[0])
            for i in range(2)]
    dm = PytorchBatchedDistortion(metrics=["ms-ssim", "psnr"])
    items = dm.per_item(output, target, cache_metrics=False)
    assert [list(r) for r in items] == [["ms-ssim", "psnr"]] * 2
    assert [r["ms-ssim"] for r in items] == want and want[0] != want[1] and 0 < want[1] < want[0] < 1
    got = dm(output, target)
    assert abs(got["ms-ssim"] - np.mean(np.float32(want))) < 1e-7
    assert got["psnr"] == _np_psnr(_np_sse(output, target).sum(), target.numel())


def test_float_and_mixed_pairs_give_what_they_gave():
    output_u8, target_u8 = _pair((2, 3, 12, 16), seed=3, pad=2)
    output, target = output_u8.float().div(255), target_u8.float().div(255)
    crop = output[..., :12, :16]
    want = 20 * np.log10(1.0) - 10 * np.log10(torch.mean((crop - target) ** 2).item())      # the float path, written out
    assert PytorchBatchedDistortion()(output, target)["psnr"] == want
    each = [20 * np.log10(1.0) - 10 * np.log10(torch.mean((crop[i:i + 1] - target[i:i + 1]) ** 2).item()) for i in range(2)]
    assert [r["psnr"] for r in PytorchBatchedDistortion().per_item(output, target)] == each
    assert PytorchBatchedDistortion(max_val=0.5)(output, target)["psnr"] == 20 * np.log10(0.5) - 10 * np.log10(torch.mean((crop - target) ** 2).item())
    # one uint8 side: the float path as before (output.type_as(target)), not the 8-bit one
    mixed = PytorchBatchedDistortion()(output_u8, target)["psnr"]
    assert mixed == 20 * np.log10(1.0) - 10 * np.log10(torch.mean((output_u8.float()[..., :12, :16] - target) ** 2).item())
    # and the 8-bit figure of the same pair is another number: the peak is 255 and the sum exact
    exact = PytorchBatchedDistortion()(output_u8, target_u8)["psnr"]
    assert exact == _np_psnr(_np_sse(output_u8[..., :12, :16], target_u8).sum(), target_u8.numel())
    assert abs(exact - want) < 1e-4 and mixed < 0


# ---------------------------------------------------------------- the harness around a stub codec, on the CPU
class _StubCodec:
    """The stub of test_cpu_coalesce.py for 8-bit items: compress = identity, decompress = the item with its low bit cleared, as
    uint8 when asked for a picture and as float otherwise; every call is logged."""

    def __init__(self, log):
        self.log = log
        self.compress_items_calls, self.decompress_items_calls, self.single_calls = 0, 0, 0

    def update_state(self, *a, **k):
        pass

    def set_complex_level(self, level):
        self.log.append(("level", level))

    @staticmethod
    def _picture(c, output_dtype):
        assert c.dtype == torch.uint8
        picture = c & 0xFE
        assert output_dtype in (None, torch.uint8)
        return picture if output_dtype == torch.uint8 else picture.float().div(255)

    def compress(self, x):
        self.single_calls += 1
        self.log.append(("compress", 1))
        return x

    def decompress(self, c, output_dtype=None):
        self.log.append(("decompress", 1))
        return self._picture(c, output_dtype)

    def compress_items(self, items, max_batch=None):
        assert len({tuple(x.shape) for x in items}) == 1 and (max_batch is None or len(items) <= max_batch)
        self.compress_items_calls += 1
        self.log.append(("compress", len(items)))
        return [x for x in items]

    def decompress_items(self, strings, max_batch=None, output_dtype=None):
        self.decompress_items_calls += 1
        self.log.append(("decompress", len(strings)))
        return [self._picture(c, output_dtype) for c in strings]


class _SpyDistortion(PytorchBatchedDistortion):
    """Notes the dtypes of every pair it is asked about."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.seen = []

    def __call__(self, output, target, **k):
        self.seen.append((output.dtype, target.dtype))
        return super().__call__(output, target, **k)

    def per_item(self, output, target, **k):
        self.seen.extend((o.dtype, t.dtype) for o, t in zip(output, target))
        return super().per_item(output, target, **k)


def _u8_items():
    out = []
    for i, wide in enumerate([0, 1, 0, 0, 1, 0, 0]):
        torch.manual_seed(i)
        out.append(torch.randint(0, 256, (1, 3, 16, 24 if wide else 16), dtype=torch.uint8))
    return out


@pytest.mark.parametrize("coalesce", [0, 3])
def test_harness_measures_and_hands_out_the_uint8_picture(tmp_path, coalesce):
    items = _u8_items()
    log, delivered = [], []

    def on_reconstruction(prefix, index, picture):
        log.append(("picture", index))
        delivered.append((prefix, index, picture))
    codec, dm = _StubCodec(log), _SpyDistortion()
    bench = BasicLosslessCompressionBenchmark(codec, items, distortion_metric=dm, force_testing_device=None, output_dir=str(tmp_path),
                                              testing_coalesce_items=coalesce, testing_complexity_levels=[0, 2], metrics_on_uint8=True,
                                              on_reconstruction=on_reconstruction)
    metrics = bench.run_benchmark(ignore_exist_metrics=True)
    bench.close()
    assert (codec.compress_items_calls, codec.single_calls) == ((6, 0) if coalesce else (0, 14))
    # the metric met uint8 pairs only, one per item and level
    assert dm.seen == [(torch.uint8, torch.uint8)] * 14
    # every item index once per level, under that level's prefix, in dataset order, and the picture is the codec's
    assert [(p, i) for p, i, _ in delivered] == [(p, i) for p in ("sclevel0", "sclevel2") for i in range(7)]
    for _, i, picture in delivered:
        assert picture.dtype == torch.uint8 and torch.equal(picture, items[i] & 0xFE)
    # outside timing: a level's pictures arrive after the last codec call of its pass, before the next level is set
    kinds = [k for k, _ in log]
    for lvl in range(2):
        start = [j for j, k in enumerate(kinds) if k == "level"][lvl]
        end = ([j for j, k in enumerate(kinds) if k == "level"] + [len(kinds)])[lvl + 1]
        span = kinds[start + 1:end]
        first = span.index("picture")
        assert set(span[:first]) == {"compress", "decompress"} and span[first:] == ["picture"] * 7
    # the logged psnr is the mean of the items' own exact figures
    each = [_np_psnr(_np_sse(x & 0xFE, x).sum(), x.numel()) for x in items]
    assert all(np.isfinite(each)) and len(set(each)) == 7
    for p in ("sclevel0", "sclevel2"):
        assert metrics[f"{p}_psnr"] == sum(each) / 7
        assert metrics[f"{p}_original_length"] == sum(x.numel() for x in items) / 7


def test_harness_without_the_flag_measures_the_float_output_as_before(tmp_path):
    items = _u8_items()
    codec, dm = _StubCodec([]), _SpyDistortion()
    bench = BasicLosslessCompressionBenchmark(codec, items, distortion_metric=dm, force_testing_device=None, output_dir=str(tmp_path))
    metrics = bench.run_benchmark(ignore_exist_metrics=True)
    assert dm.seen == [(torch.float32, torch.float32)] * 7
    each = [20 * np.log10(1.0) - 10 * np.log10(torch.mean(((x & 0xFE).float().div(255) - x.float().div(255)) ** 2).item()) for x in items]
    assert metrics["_psnr"] == sum(each) / 7
    with pytest.raises(ValueError, match="metrics_on_uint8"):
        BasicLosslessCompressionBenchmark(codec, items, force_testing_device=None, on_reconstruction=lambda *a: None)


def test_harness_quantises_a_float_item_once_and_the_forward_estimate(tmp_path):
    """Float items: the target is the item's 8-bit picture; the forward pass stays a float graph whose output is quantised for the metric."""
    torch.manual_seed(0)
    items = [torch.rand(1, 3, 8, 8) * 1.2 - 0.1 for _ in range(3)]
    quantised = [torch.nan_to_num(x, nan=0.0).clamp(0, 1).mul(255).round().to(torch.uint8) for x in items]

    class Codec:
        def update_state(self):
            pass

        def forward_estimate_bitlen(self, x):
            assert x.dtype == torch.float32
            return x + 1.0 / 255, 10.0

        def compress(self, x):
            return x

        def decompress(self, c, output_dtype=None):
            assert output_dtype == torch.uint8
            return torch.nan_to_num(c, nan=0.0).clamp(0, 1).mul(255).round().to(torch.uint8)
    dm, delivered = _SpyDistortion(), []
    bench = BasicLosslessCompressionBenchmark(Codec(), items, distortion_metric=dm, force_testing_device=None, metrics_on_uint8=True,
                                              nn_codec_use_forward_pass=True, on_reconstruction=lambda p, i, x: delivered.append((p, i, x)))
    metrics = bench.run_benchmark()
    assert dm.seen == [(torch.uint8, torch.uint8)] * 6
    assert [(p, i) for p, i, _ in delivered] == [("", 0), ("", 1), ("", 2)]
    assert all(torch.equal(x, q) for (_, _, x), q in zip(delivered, quantised))
    # three forward estimates (one level off wherever the item is not at the top) and three exact reconstructions (inf): the mean is inf
    assert metrics["_psnr"] == math.inf and metrics["_compressed_length_nn_forward"] == 10.0
