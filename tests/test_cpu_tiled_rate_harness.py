"""The tiled step and budget switches of the harness and the tool (INTEGRATION.md "Tiled pictures: step and byte budget"), without a
GPU: ``testing_tile_qsteps`` / ``testing_tile_target_bpps`` run one pass per value through compress_tiled_q / compress_tiled_to_rate
(pooled: their _items forms) under the level prefixes tq<step> / tbpp<target>, need ``testing_tile``, and are refused with each
other, with the untiled knobs and with what refuses those -- while the untiled knobs stay refused with the tiles, as before."""
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
    """One "tile" per picture: the picture quantised to 255 / (4 step) levels and deflated, in a real BTQ1 container whose tile is the
    whole picture.  compress_tiled_to_rate takes the first of four steps whose container fits, else the coarsest."""
    STEPS = [0.5, 1.0, 2.0, 4.0]

    def __init__(self):
        self.calls = []

    def update_state(self, *a, **k):
        pass

    def _pack(self, x, step):
        from cbench_basic_amd.utils.tiling import pack_tiled_q
        _, C, H, W = x.shape
        levels = 255.0 / (4 * step)
        body = zlib.compress(torch.round(x.float() / (255.0 if x.dtype == torch.uint8 else 1.0) * levels).to(torch.uint8).numpy().tobytes(), 9)
        return pack_tiled_q(C, H, W, H, W, [body], step)

    def compress_tiled_q(self, x, qstep, tile=None, overlap=0, pad_to=1):
        self.calls.append(("q", qstep, tile, tuple(overlap), pad_to))
        return self._pack(x, qstep)

    def compress_tiled_to_rate(self, x, target_bpp=None, tile=None, overlap=0, pad_to=1):
        self.calls.append(("bpp", target_bpp, tile, tuple(overlap), pad_to))
        budget = int(target_bpp * x.shape[-1] * x.shape[-2] / 8)
        for step in self.STEPS:
            out = self._pack(x, step)
            if len(out) <= budget:
                break
        return out

    def compress_tiled_items_q(self, xs, qstep, **kw):
        self.calls.append(("items_q", len(xs)))
        return [self.compress_tiled_q(x, qstep, **kw) for x in xs]

    def compress_tiled_items_to_rate(self, xs, target_bpp=None, **kw):
        self.calls.append(("items_bpp", len(xs)))
        return [self.compress_tiled_to_rate(x, target_bpp=target_bpp, **kw) for x in xs]

    def decompress_tiled(self, data, output_dtype=None):
        from cbench_basic_amd.utils.tiling import unpack_tiled_q
        t = unpack_tiled_q(data)
        levels = 255.0 / (4 * float(t.steps[0]))
        x = torch.from_numpy(np.frombuffer(zlib.decompress(t.strings[0]), dtype=np.uint8).copy()).reshape(1, t.channels, t.H, t.W).float() / levels
        return torch.round(x.clamp(0, 1) * 255).to(torch.uint8) if output_dtype == torch.uint8 else x

    def decompress_tiled_items(self, datas, output_dtype=None):
        return [self.decompress_tiled(d, output_dtype=output_dtype) for d in datas]

    def compress_tiled(self, *a, **k):
        raise AssertionError("a tiled step or budget pass goes through compress_tiled_q / compress_tiled_to_rate")

    compress = compress_q = compress_to_rate = compress_tiled_items = compress_tiled


def _items(u8):
    out = []
    for i in range(4):
        torch.manual_seed(i)
        x = torch.rand(1, 3, 32, 32 + 8 * (i % 2))
        out.append((x * 255).round().to(torch.uint8) if u8 else x)
    return out


@pytest.mark.parametrize("u8,on_u8", [(False, False), (True, True), (False, True)])
@pytest.mark.parametrize("pool", [0, 2])
@pytest.mark.parametrize("which", ["tq", "tbpp"])
def test_harness_one_pass_per_value(tmp_path, which, pool, u8, on_u8):
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion
    items = _items(u8)
    values = [0.5, 1.0, 2.0, 4.0] if which == "tq" else [24.0, 20.0, 16.0, 12.0]
    knob = dict(testing_tile_qsteps=values) if which == "tq" else dict(testing_tile_target_bpps=values)
    codec = _StubCodec()
    bench = BasicLosslessCompressionBenchmark(codec, items, distortion_metric=PytorchBatchedDistortion(), force_testing_device=None,
                                              metrics_on_uint8=on_u8, output_dir=str(tmp_path), testing_tile=(32, 32), testing_tile_overlap=4,
                                              testing_tile_pad=8, testing_tile_pool=pool, **knob)
    res = bench.run_benchmark(ignore_exist_metrics=True)
    bench.close()
    singles = [c for c in codec.calls if c[0] in ("q", "bpp")]
    assert [c[1] for c in singles] == [v for v in values for _ in items]
    assert all(c[0] == ("q" if which == "tq" else "bpp") and c[2:] == ((32, 32), (4, 4), (8, 8)) for c in singles)     # overlap and padding reach the call
    pooled = [c for c in codec.calls if c[0].startswith("items")]
    assert len(pooled) == (len(values) * len(items) // pool if pool else 0) and all(c[1] == pool for c in pooled)
    prefixes = [("tq%g" if which == "tq" else "tbpp%g") % v for v in values]
    for p in prefixes:
        assert f"{p}_compressed_length" in res and f"{p}_psnr" in res and f"{p}_time_compress" in res
    lens = [res[f"{p}_compressed_length"] for p in prefixes]
    assert lens == sorted(lens, reverse=True) and len(set(lens)) == len(values)        # a coarser step, a lower target: fewer bytes
    # compressed_length is the container's length
    x0 = items[0]
    first = codec._pack(x0, 0.5)
    assert first[:4] == b"BTQ1" and struct.unpack_from("<f", first, 41)[0] == 0.5
    with open(tmp_path / "metrics_2d.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert [r[0] for r in rows[1:]] == prefixes and "compressed_length" in rows[0] and "psnr" in rows[0]


def test_harness_refusals():
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark as B
    for knob, other in (("testing_tile_qsteps", "testing_tile_target_bpps"), ("testing_tile_target_bpps", "testing_tile_qsteps")):
        with pytest.raises(ValueError, match="needs testing_tile"):
            B(None, [], **{knob: [1.0]})
        for kw in ({other: [2.0]}, dict(testing_complexity_levels=[0, 1]), dict(testing_variable_rate_levels=[0, 1]),
                   dict(nn_codec_use_forward_pass=True)):
            with pytest.raises(ValueError, match=knob):
                B(None, [], testing_tile=64, **{knob: [1.0]}, **kw)
        for kw in (dict(testing_qsteps=[1.0]), dict(testing_target_bpps=[1.0]), dict(testing_coalesce_items=4)):
            with pytest.raises(ValueError):
                B(None, [], testing_tile=64, **{knob: [1.0]}, **kw)
        ok = B(None, [], testing_tile=64, testing_tile_overlap=8, testing_tile_pad=16, testing_tile_pool=3, metrics_on_uint8=True, **{knob: [0.5, 2]})
        assert getattr(ok, knob) == [0.5, 2.0] and getattr(ok, other) == []
    for bad in ([0.0], [65.0], [float("nan")], [2.0 ** -5]):
        with pytest.raises(ValueError):
            B(None, [], testing_tile=64, testing_tile_qsteps=bad)
    for bad in ([0.0], [1.0, float("nan")], [float("inf")], [-2.0]):
        with pytest.raises(ValueError):
            B(None, [], testing_tile=64, testing_tile_target_bpps=bad)
    # the untiled knobs are refused with the tiles exactly as they were
    with pytest.raises(ValueError, match="testing_qsteps does not combine with testing_tile"):
        B(None, [], testing_qsteps=[1.0], testing_tile=64)
    with pytest.raises(ValueError, match="testing_target_bpps does not combine with testing_tile"):
        B(None, [], testing_target_bpps=[1.0], testing_tile=64)
    plain = B(None, [])
    assert plain.testing_tile_qsteps == [] and plain.testing_tile_target_bpps == []


def _tool():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "run_benchmark.py")
    spec = importlib.util.spec_from_file_location("run_benchmark_tool_tiled_rate", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


CASES = []
for _flag, _other in (("--tile-qsteps", "--tile-target-bpp"), ("--tile-target-bpp", "--tile-qsteps")):
    CASES += [([_flag, "1"], _flag, "needs --tile"), ([_flag, "1", "--tile", "64", _other, "2"], _flag, _other),
              ([_flag, "1", "--tile", "64", "--complexity-levels", "0", "1"], _flag, "--complexity-levels"),
              ([_flag, "1", "--tile", "64", "--rate-levels", "0"], _flag, "--rate-levels"),
              ([_flag, "1", "--tile", "64", "--forward-pass"], _flag, "--forward-pass"),
              ([_flag, "1", "--tile", "64", "--coalesce", "4"], _flag, "--coalesce"),
              ([_flag, "1", "--tile", "64", "--codec", "topogroup"], _flag, "--codec hyperprior"),
              ([_flag, "1", "--tile", "64", "--codec", "basic"], _flag, "--codec hyperprior"),
              ([_flag, "0", "--tile", "64"], _flag, ""), ([_flag, "nan", "--tile", "64"], _flag, ""), ([_flag, "1", "inf", "--tile", "64"], _flag, ""),
              ([_flag], _flag, "expected at least one argument")]
CASES += [(["--tile-qsteps", "1", "--tile", "64", "--qsteps", "2"], "--tile-qsteps", "--qsteps"),
          (["--tile-qsteps", "1", "--tile", "64", "--target-bpp", "2"], "--tile-qsteps", "--target-bpp"),
          (["--tile-target-bpp", "1", "--tile", "64", "--qsteps", "2"], "--tile-target-bpp", "--qsteps"),
          (["--tile-target-bpp", "1", "--tile", "64", "--target-bpp", "2"], "--tile-target-bpp", "--target-bpp"),
          (["--tile-qsteps", "65", "--tile", "64"], "--tile-qsteps", "quantiser step"),
          # and the old refusals, unchanged
          (["--qsteps", "1", "--tile", "64"], "--qsteps", "--tile"), (["--target-bpp", "1", "--tile", "64"], "--target-bpp", "--tile"),
          (["--target-bpp", "1", "--tile", "64", "--tile-pool", "2"], "--target-bpp", "--tile"),
          (["--qsteps", "1", "--tile", "64", "--tile-pad", "16"], "--qsteps", "--tile")]


@pytest.mark.parametrize("argv,flag,word", CASES)
def test_tool_refusals(argv, flag, word, monkeypatch, capsys):
    tool = _tool()
    monkeypatch.setattr(sys, "argv", ["run_benchmark.py", "--out", "unused"] + argv)
    with pytest.raises(SystemExit) as e:
        tool.main()
    err = capsys.readouterr().err
    assert e.value.code == 2 and flag in err and word in err, err


def test_tool_accepts_the_composable_switches(monkeypatch):
    """Past the argument checks with every switch the new ones compose with: the tool stops only where it needs the GPU."""
    tool = _tool()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for flag in ("--tile-qsteps", "--tile-target-bpp"):
        monkeypatch.setattr(sys, "argv", ["run_benchmark.py", "--out", "unused", flag, "0.5", "2", "--tile", "64", "--tile-overlap", "8", "--tile-pad",
                                          "16", "--tile-pool", "4", "--uint8", "--metrics-on-uint8", "--stream-lanes", "4"])
        with pytest.raises(SystemExit) as e:
            tool.main()
        assert "needs an MI355X" in str(e.value.code)
