"""Rate targets in the harness and the tool (INTEGRATION.md "Rate control"), without a GPU: ``testing_target_bpps`` runs one pass per
target through compress_to_rate / decompress_q under the level prefix bpp<target>, and both refuse what refuses ``testing_qsteps``."""
import csv
import importlib.util
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch


class _StubCodec:
    """compress_to_rate: the coarsest of four steps' codes (the picture quantised to 255 / (4 step) levels, deflated) that fits the
    budget, else the coarsest, in the real container."""
    STEPS = [0.5, 1.0, 2.0, 4.0]

    def __init__(self):
        self.calls, self.plain_calls = [], 0

    def update_state(self, *a, **k):
        pass

    @staticmethod
    def _code(x, step):
        levels = 255.0 / (4 * step)
        return struct.pack("<3I", *x.shape[1:]) + zlib.compress(torch.round(x * levels).to(torch.uint8).numpy().tobytes(), 9)

    def compress_to_rate(self, x, target_bpp=None):
        from cbench_basic_amd.utils.qstep import pack_qsteps
        self.calls.append(target_bpp)
        budget = int(target_bpp * x.shape[-1] * x.shape[-2] / 8)
        for step in self.STEPS:
            inner = self._code(x, step)
            if len(inner) <= budget:
                break
        return pack_qsteps(step, inner)

    def decompress_q(self, data, output_dtype=None):
        from cbench_basic_amd.utils.qstep import unpack_qsteps
        steps, inner = unpack_qsteps(data, batch=1)
        shape = struct.unpack("<3I", bytes(inner[:12]))
        levels = 255.0 / (4 * float(steps[0]))
        x = torch.from_numpy(np.frombuffer(zlib.decompress(bytes(inner[12:])), dtype=np.uint8).copy()).reshape(1, *shape).float() / levels
        return torch.round(x.clamp(0, 1) * 255).to(torch.uint8) if output_dtype == torch.uint8 else x

    def compress(self, x):
        self.plain_calls += 1
        raise AssertionError("a rate-target pass goes through compress_to_rate")


@pytest.mark.parametrize("on_u8", [False, True])
def test_harness_one_pass_per_target(tmp_path, on_u8):
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion
    items = []
    for i in range(4):
        torch.manual_seed(i)
        items.append(torch.rand(1, 3, 32, 32))
    targets = [24.0, 20.0, 16.0]                     # uniform noise: about 21, 18, 15, 12 bpp at the four steps
    codec = _StubCodec()
    bench = BasicLosslessCompressionBenchmark(codec, items, distortion_metric=PytorchBatchedDistortion(), force_testing_device=None,
                                              metrics_on_uint8=on_u8, output_dir=str(tmp_path), testing_target_bpps=targets)
    res = bench.run_benchmark(ignore_exist_metrics=True)
    bench.close()
    assert codec.calls == [t for t in targets for _ in items] and codec.plain_calls == 0
    prefixes = ["bpp24", "bpp20", "bpp16"]
    for p in prefixes:
        assert f"{p}_compressed_length" in res and f"{p}_psnr" in res and f"{p}_time_compress" in res
    lens = [res[f"{p}_compressed_length"] for p in prefixes]
    assert lens == sorted(lens, reverse=True) and len(set(lens)) == 3               # a lower target: fewer bytes
    with open(tmp_path / "metrics_2d.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert [r[0] for r in rows[1:]] == prefixes


def test_harness_refusals():
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark
    for kw in (dict(testing_qsteps=[1.0]), dict(testing_coalesce_items=4), dict(testing_tile=64), dict(testing_complexity_levels=[0, 1]),
               dict(testing_variable_rate_levels=[0, 1]), dict(nn_codec_use_forward_pass=True)):
        with pytest.raises(ValueError, match="testing_target_bpps"):
            BasicLosslessCompressionBenchmark(None, [], testing_target_bpps=[0.5, 1.0], **kw)
    for bad in ([0.0], [1.0, float("nan")], [float("inf")], [-2.0]):
        with pytest.raises(ValueError):
            BasicLosslessCompressionBenchmark(None, [], testing_target_bpps=bad)
    assert BasicLosslessCompressionBenchmark(None, [], testing_target_bpps=[0.5, 2]).testing_target_bpps == [0.5, 2.0]
    assert BasicLosslessCompressionBenchmark(None, []).testing_target_bpps == []


def _tool():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "run_benchmark.py")
    spec = importlib.util.spec_from_file_location("run_benchmark_tool_rate", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.mark.parametrize("argv,word", [(["--target-bpp", "1", "--qsteps", "2"], "--qsteps"), (["--target-bpp", "1", "--coalesce", "4"], "--coalesce"),
                                       (["--target-bpp", "1", "--tile", "64"], "--tile"),
                                       (["--target-bpp", "1", "--tile", "64", "--tile-pool", "2"], "--tile"),
                                       (["--target-bpp", "1", "--complexity-levels", "0", "1"], "--complexity-levels"),
                                       (["--target-bpp", "1", "--codec", "topogroup"], "--codec hyperprior"),
                                       (["--target-bpp", "1", "--codec", "basic"], "--codec hyperprior"),
                                       (["--target-bpp", "0"], "positive"), (["--target-bpp", "1", "-3"], "positive"),
                                       (["--target-bpp", "nan"], "finite"), (["--target-bpp", "inf"], "finite"),
                                       (["--target-bpp"], "expected at least one argument")])
def test_tool_refusals(argv, word, monkeypatch, capsys):
    tool = _tool()
    monkeypatch.setattr(sys, "argv", ["run_benchmark.py", "--out", "unused"] + argv)
    with pytest.raises(SystemExit) as e:
        tool.main()
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--target-bpp" in err and word in err, err
