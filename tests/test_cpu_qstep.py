"""The quantiser step of the hyperprior y coder on the CPU (INTEGRATION.md "Quantiser step"): the NumPy restatement at step 1 is
today's rule; the container of compress_q round-trips and refuses what is not one; steps are validated on the host; the tool refuses
the combinations it cannot serve; the harness makes one pass per step and logs what it logs for variable-rate levels."""
import csv
import importlib.util
import math
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

import qstep_exact as QX

TABLE = np.exp(np.linspace(math.log(0.11), math.log(256), 64)).astype(np.float32)


# ---------------------------------------------------------------- the restatement
def test_restatement_at_step_one_is_todays_rule():
    rng = np.random.default_rng(0)
    n = 3 * 280
    y = np.where(rng.random(n) < 0.5, rng.integers(-40, 41, n) / 2.0, rng.normal(size=n) * 6).astype(np.float32)   # ties included
    s = np.exp(rng.uniform(math.log(0.03), math.log(400), n)).astype(np.float32)                                    # below the bound, past the table
    s[:64] = TABLE
    s[64:66] = np.nan
    for steps in ([1.0], [1.0, 1.0, 1.0]):
        sym, idx, yhat = QX.quantize_index_q(y, s, steps, 280, TABLE, 0.11)
        assert np.array_equal(sym, np.rint(y).astype(np.int32)) and np.array_equal(yhat.view(np.int32), np.rint(y).view(np.int32))
        # the existing index rule, as tests/test_gpu_entropy_kernels.py states it: count the entries at or above max(s, bound)
        sb = np.fmax(s, np.float32(0.11))
        want = np.full(n, 63, dtype=np.int32)
        for t in TABLE[:-1]:
            want -= (sb <= t).astype(np.int32)
        assert np.array_equal(idx, want)
        assert (idx[:64] == np.arange(64)).all() and (idx[64:66] == 0).all() and idx.max() == 63
        assert QX.same_reconstruction(QX.dequantize_q(sym, steps, 280), yhat, sym)
        assert np.signbit(yhat[sym == 0]).any()             # rint(-0.25) = -0.0 was among them


def test_restatement_steps_ties_and_image_boundaries():
    y = np.array([0.75, 1.25, 4.5, -4.5, 4.5, -4.5], dtype=np.float32)
    s = np.array([1.0, 1.0, 1.0, 1.0, 3.0, 0.01], dtype=np.float32)
    sym, idx, yhat = QX.quantize_index_q(y, s, [0.5, 1.0, 3.0], 2, TABLE, 0.11)
    assert sym.tolist() == [2, 2, 4, -4, 2, -2]            # 1.5 -> 2, 2.5 -> 2 (half to even); image 1 at step 1; +/-1.5 -> +/-2
    assert yhat.tolist() == [1.0, 1.0, 4.0, -4.0, 6.0, -6.0]
    assert idx.tolist() == QX.index_rule(np.array([2.0, 2.0, 1.0, 1.0, 1.0, np.float32(0.11) / np.float32(3.0)], np.float32), TABLE).tolist()
    assert idx[5] == 0                                      # the bound first, then the step: 0.11 / 3 lies below the table
    # '<' against '<=': a scale of table[j] * step lands on j, the next float above it on j + 1
    j, d = 20, np.float32(4.0)
    on = TABLE[j] * d
    s3 = np.array([on, np.nextafter(on, np.float32(np.inf)), np.nextafter(on, np.float32(0))], dtype=np.float32)
    assert QX.quantize_index_q(np.zeros(3, np.float32), s3, [4.0], 3, TABLE, 0.11)[1].tolist() == [j, j + 1, j]


# ---------------------------------------------------------------- steps and container
def test_check_qsteps():
    from cbench_basic_amd.utils.qstep import QSTEP_MAX, QSTEP_MIN, check_qsteps
    assert (QSTEP_MIN, QSTEP_MAX) == (2.0 ** -4, 2.0 ** 6)
    for good, batch in ((1.0, None), (0.0625, 5), (64, 1), ([0.5, 1, 3], 3), (np.array([2.0]), 7), (torch.tensor([0.7, 3.0]), 2)):
        out = check_qsteps(good, batch)
        assert out.dtype == np.float32 and out.ndim == 1 and out.flags.c_contiguous
    assert check_qsteps(0.7)[0] == np.float32(0.7)
    for bad in (0, 0.0, -1.0, -0.5, float("nan"), float("inf"), -float("inf"), 0.06, 2.0 ** -5, 64.5, 1e9, [1.0, 0.0], [1.0, float("nan")],
                [], [[1.0, 2.0]], "x", None):
        with pytest.raises(ValueError):
            check_qsteps(bad)
    for steps, batch in (([1.0, 2.0], 3), ([1.0, 2.0, 3.0], 2), ([1.0, 2.0], 1)):      # n is 1 or the batch
        with pytest.raises(ValueError, match="one per image"):
            check_qsteps(steps, batch)


def test_container_round_trip_and_refusals():
    from cbench_basic_amd.utils.qstep import QSTEP_MAGIC, pack_qsteps, unpack_qsteps
    inner = bytes(range(200))
    for steps in ([1.0], [0.5, 1.0, 3.0], [0.7]):
        data = pack_qsteps(steps, inner)
        n = len(steps)
        assert data[:4] == QSTEP_MAGIC == b"BQS1" and struct.unpack("<I", data[4:8])[0] == n
        assert data[8:8 + 4 * n] == np.asarray(steps, "<f4").tobytes() and data[8 + 4 * n:] == inner
        got, rest = unpack_qsteps(data, batch=3)
        assert got.dtype == np.float32 and got.tolist() == np.asarray(steps, np.float32).tolist() and bytes(rest) == inner
        assert bytes(unpack_qsteps(memoryview(data))[1]) == inner
    good = pack_qsteps([0.5, 2.0], inner)
    for bad in (b"", b"BQS", b"BQS1", b"BQS1\x01\x00\x00", b"BQS2" + good[4:], b"BTL1" + good[4:], good[:12], good[:15], inner):
        with pytest.raises(ValueError):
            unpack_qsteps(bad)
    with pytest.raises(ValueError):                       # zero steps stated
        unpack_qsteps(b"BQS1" + struct.pack("<I", 0) + inner)
    with pytest.raises(ValueError):                       # more steps stated than the buffer holds
        unpack_qsteps(b"BQS1" + struct.pack("<I", 1 << 30) + inner)
    for batch in (3, 5):                                  # n = 2 is neither 1 nor the batch
        with pytest.raises(ValueError, match="one per image"):
            unpack_qsteps(good, batch=batch)
    assert unpack_qsteps(good, batch=2)[0].tolist() == [0.5, 2.0]
    for v in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -5, 128.0):      # invalid steps inside a well-formed container
        with pytest.raises(ValueError):
            unpack_qsteps(b"BQS1" + struct.pack("<If", 1, v) + inner)
    with pytest.raises(ValueError):
        pack_qsteps([0.0], inner)


# ---------------------------------------------------------------- the tool
def _tool():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "run_benchmark.py")
    spec = importlib.util.spec_from_file_location("run_benchmark_tool_qstep", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.mark.parametrize("argv,word", [(["--qsteps", "2", "--coalesce", "4"], "--coalesce"), (["--qsteps", "2", "--tile", "64"], "--tile"),
                                       (["--qsteps", "2", "--tile", "64", "--tile-overlap", "8"], "--tile"),
                                       (["--qsteps", "2", "--tile", "64", "--tile-pad", "32"], "--tile"),
                                       (["--qsteps", "2", "--tile", "64", "--tile-pool", "2"], "--tile"),
                                       (["--qsteps", "2", "--complexity-levels", "0", "1"], "--complexity-levels"),
                                       (["--qsteps", "2", "--codec", "topogroup"], "--codec hyperprior"),
                                       (["--qsteps", "2", "--codec", "basic"], "--codec hyperprior"),
                                       (["--qsteps", "0"], "[0.0625, 64"), (["--qsteps", "1", "-3"], "[0.0625, 64"),
                                       (["--qsteps", "nan"], "finite"), (["--qsteps", "inf"], "finite"), (["--qsteps", "100"], "[0.0625, 64"),
                                       (["--qsteps"], "expected at least one argument")])
def test_tool_refusals(argv, word, monkeypatch, capsys):
    tool = _tool()
    monkeypatch.setattr(sys, "argv", ["run_benchmark.py", "--out", "unused"] + argv)
    with pytest.raises(SystemExit) as e:
        tool.main()
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--qsteps" in err and word in err, err


# ---------------------------------------------------------------- the harness with a stub codec
class _StubCodec:
    """compress_q: the picture quantised to 255 / (4 step) levels, deflated, in the real container; a twin with rate levels that mean
    the same steps goes through compress / decompress."""
    STEPS = [0.5, 1.0, 2.0, 4.0]

    def __init__(self):
        self.q_calls, self.plain_calls, self.level = [], 0, None

    def update_state(self, *a, **k):
        pass

    def set_rate_level(self, level):
        self.level = level

    @staticmethod
    def _code(x, step):
        levels = 255.0 / (4 * step)
        return struct.pack("<3I", *x.shape[1:]) + zlib.compress(torch.round(x * levels).to(torch.uint8).numpy().tobytes(), 9)

    @staticmethod
    def _decode(inner, step, output_dtype):
        shape = struct.unpack("<3I", bytes(inner[:12]))
        levels = 255.0 / (4 * step)
        x = torch.from_numpy(np.frombuffer(zlib.decompress(bytes(inner[12:])), dtype=np.uint8).copy()).reshape(1, *shape).float() / levels
        return torch.round(x.clamp(0, 1) * 255).to(torch.uint8) if output_dtype == torch.uint8 else x

    def compress_q(self, x, qstep):
        from cbench_basic_amd.utils.qstep import pack_qsteps
        self.q_calls.append(qstep)
        return pack_qsteps(qstep, self._code(x, qstep))

    def decompress_q(self, data, output_dtype=None):
        from cbench_basic_amd.utils.qstep import unpack_qsteps
        steps, inner = unpack_qsteps(data, batch=1)
        return self._decode(inner, float(steps[0]), output_dtype)

    def compress(self, x):
        self.plain_calls += 1
        return b"BQS1" + struct.pack("<If", 1, self.STEPS[self.level]) + self._code(x, self.STEPS[self.level])   # the same length

    def decompress(self, data, output_dtype=None):
        return self._decode(data[12:], self.STEPS[self.level], output_dtype)


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


@pytest.mark.parametrize("on_u8", [False, True])
def test_harness_one_pass_per_step_logged_as_rate_levels_are(tmp_path, on_u8):
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion
    from cbench_basic_amd.benchmark.metrics import BJDeltaMetric
    items = []
    for i in range(5):
        torch.manual_seed(i)
        items.append(torch.rand(1, 3, 32, 32))
    ref_pts = ([300.0, 400.0, 500.0, 600.0], [20.0, 25.0, 30.0, 35.0])
    res, codecs = {}, {}
    for name, kw in (("q", dict(testing_qsteps=_StubCodec.STEPS)), ("vr", dict(testing_variable_rate_levels=[0, 1, 2, 3]))):
        codecs[name] = _StubCodec()
        bench = BasicLosslessCompressionBenchmark(codecs[name], items, distortion_metric=PytorchBatchedDistortion(),
                                                  force_testing_device=None, metrics_on_uint8=on_u8,
                                                  testing_variable_rate_bj_delta_metric=BJDeltaMetric(reference_pts=ref_pts),
                                                  output_dir=str(tmp_path / name), **kw)
        res[name] = bench.run_benchmark(ignore_exist_metrics=True)
        bench.close()
    q, vr = res["q"], res["vr"]
    assert codecs["q"].q_calls == [s for s in _StubCodec.STEPS for _ in items] and codecs["q"].plain_calls == 0
    assert codecs["vr"].q_calls == [] and codecs["vr"].plain_calls == 4 * len(items)
    prefixes = ["q0.5", "q1", "q2", "q4"]
    rename = lambda k: k if not k.startswith("vrlevel") else prefixes[int(k[7])] + k[8:]
    assert [rename(k) for k in vr] == list(q)              # the same metric names in the same order, under q<step>
    for p in prefixes:
        assert f"{p}_compressed_length" in q and f"{p}_psnr" in q and f"{p}_time_compress" in q
    assert "BD-psnr" in q and np.isfinite(q["BD-psnr"]) and q["BD-psnr"] != -100
    for k in vr:
        if "time_" not in k and "speed_" not in k:
            assert q[rename(k)] == vr[k], k
    lens = [q[f"{p}_compressed_length"] for p in prefixes]
    assert lens == sorted(lens, reverse=True) and len(set(lens)) == 4          # a coarser step: fewer bytes
    # the files: one metrics.csv row, one metrics_2d.csv row per step, named by its prefix, with the columns of the rate levels' rows
    r1, r1v = _rows(tmp_path / "q" / "metrics.csv"), _rows(tmp_path / "vr" / "metrics.csv")
    assert len(r1) == len(r1v) == 2 and [rename(c) for c in r1v[0]] == r1[0]
    r2, r2v = _rows(tmp_path / "q" / "metrics_2d.csv"), _rows(tmp_path / "vr" / "metrics_2d.csv")
    assert len(r2) == len(r2v) == 5 and r2[0] == r2v[0]
    assert [row[0] for row in r2[1:]] == prefixes and [row[0] for row in r2v[1:]] == ["vrlevel0", "vrlevel1", "vrlevel2", "vrlevel3"]
    assert "BD-psnr" in r2[0]


def test_harness_refusals():
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark
    for kw in (dict(testing_coalesce_items=4), dict(testing_tile=64), dict(testing_complexity_levels=[0, 1]),
               dict(testing_variable_rate_levels=[0, 1]), dict(nn_codec_use_forward_pass=True)):
        with pytest.raises(ValueError, match="testing_qsteps"):
            BasicLosslessCompressionBenchmark(None, [], testing_qsteps=[1.0, 2.0], **kw)
    for bad in ([0.0], [1.0, float("nan")], [128.0], [-2.0]):
        with pytest.raises(ValueError):
            BasicLosslessCompressionBenchmark(None, [], testing_qsteps=bad)
    assert BasicLosslessCompressionBenchmark(None, [], testing_qsteps=[0.5, 2]).testing_qsteps == [0.5, 2.0]
    assert BasicLosslessCompressionBenchmark(None, []).testing_qsteps == []
