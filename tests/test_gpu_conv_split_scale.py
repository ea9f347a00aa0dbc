"""GPU: the power-of-two scaling of the split-fp16 synthesis kernel (csrc/conv.hip conv_split_f16_kernel).

The kernel scales every output channel's weights into [2^13, 2^14) and every image's activations into [2^14, 2^15) before
it splits them into two fp16 pieces, and undoes both by the exponent in the epilogue.  Without the scaling the low pieces of
small operands fall into fp16's subnormal range (22-41x the fp32 chain's error at activations of order 2^-10, measured by
scripts/micro/mfma_f16_split.hip); with a scale
per tensor or per tile an image's bits would depend on its neighbours.  So the tests move the magnitudes of the
activations and of the weights over many octaves, per tensor, per image and per channel, and check

  * accuracy: RMS error against the fp64 CPU computation <= 1.5 x the fp32 kernel's (BASIC_CONV_F32=1) on the same case,
    max abs error <= 1e-5 x max |ref| of the case (asserted of the fp32 kernel first, so the bound can be met at all),
    and an output that differs from the fp32 kernel's (the split path did run);
  * invariance: an image's bits do not depend on the batch around it, and the two activation sources agree;
  * edges: an all-zero image, an image that holds an infinity.

The references are the fp64 computation and the fp32 kernel, never the split path itself.

Bias.  Where a case scales the whole input (or the whole weight tensor) by s, the bias is scaled by s with it: with the
0.1-sized bias left alone under a 2^-20 input the sum conv + bias would round the convolution's error away, and the case
would say nothing about the scaling (nor could the output differ from the fp32 kernel's).  Every other case keeps the bias.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# cin, cout, B, H, W: g_s layers 1..3 as in test_gpu_conv_split.py LAYERS, and one shape whose 256-position tile holds four
# 8 x 8 images, the last tile partial
SHAPES = [(192, 128, 2, 16, 16), (128, 128, 2, 32, 32), (128, 128, 1, 24, 40), (128, 128, 5, 8, 8)]
ERR_FACTOR = 1.5
MAX_REL = 1e-5


def _base(shape, tag=""):
    cin, cout, B, H, W = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, tag)).encode()) % (2 ** 31))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cin, cout, 5, 5, generator=g) * (1.0 / (cin * 25) ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    gamma = torch.rand(cout, cout, generator=g) * 0.02 + 0.1 * torch.eye(cout)
    beta = torch.rand(cout, generator=g) + 0.5
    return g, x, w, b, gamma, beta


def _act_case(name, g, x, w, b):
    B, cin = x.shape[:2]
    if name in ("x*2^-20", "x*1e-3", "x*3e3"):
        s = {"x*2^-20": 2.0 ** -20, "x*1e-3": 1e-3, "x*3e3": 3e3}[name]
        return x * s, w, b * s
    if name == "two-images":  # two images of one batch, 2^-12 and 2^9 (a one-image batch is doubled)
        if B == 1:
            x = torch.cat([x, x.flip(-1)])
        x = x.clone()
        x[0] *= 2.0 ** -12
        x[-1] *= 2.0 ** 9
        return x, w, b
    if name == "channels":    # every input channel by its own 2^u, u from -14 .. 0
        u = torch.randint(-14, 1, (cin,), generator=g)
        return x * torch.exp2(u.float()).view(1, cin, 1, 1), w, b
    if name == "integers":    # what g_s layer 1 sees: dequantised symbols
        return torch.round(40 * x), w, b
    raise KeyError(name)


def _weight_case(name, g, x, w, b):
    if name in ("w*2^-30", "w*2^12"):
        s = 2.0 ** (-30 if name == "w*2^-30" else 12)
        return x, w * s, b * s
    w = w.clone()
    if name == "zero-channel":
        w[:, 5] = 0
        return x, w, b
    if name == "loud-channel":
        w[:, 77] *= 2.0 ** 10
        return x, w, b
    raise KeyError(name)


ACT_CASES = ["x*2^-20", "x*1e-3", "x*3e3", "two-images", "channels", "integers"]
WEIGHT_CASES = ["w*2^-30", "w*2^12", "zero-channel", "loud-channel"]


def _reference64(x, w, b, gamma, beta):
    cout = w.shape[1]
    ref = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=2, output_padding=1)
    norm = F.conv2d(ref * ref, gamma.double().reshape(cout, cout, 1, 1), beta.double())
    return ref * torch.sqrt(norm)


def _plan(w, b, gamma, beta):
    from cbench_basic_amd.nn import kernels as K
    return K.ConvPlan(w, b, 2, 2, 1, True, K.ACT_IGDN, gamma, beta)


def _run(plan, x, monkeypatch, f32=False, debug="8"):
    monkeypatch.setenv("BASIC_CONV_DEBUG", debug)
    if f32:
        monkeypatch.setenv("BASIC_CONV_F32", "1")
    else:
        monkeypatch.delenv("BASIC_CONV_F32", raising=False)
    out = plan(x.cuda())
    torch.cuda.synchronize()
    return out.cpu()


def _check_accuracy(name, x, w, b, gamma, beta, monkeypatch):
    ref = _reference64(x, w, b, gamma, beta)
    plan = _plan(w, b, gamma, beta)
    got = _run(plan, x, monkeypatch)
    got32 = _run(plan, x, monkeypatch, f32=True)
    rms = lambda t: float(((t.double() - ref) ** 2).mean().sqrt())
    mx = lambda t: float((t.double() - ref).abs().max())
    scale = float(ref.abs().max())
    print(f"{name} {tuple(x.shape)}: rms split {rms(got):.3e} fp32 {rms(got32):.3e} ({rms(got) / rms(got32):.2f}x), "
          f"max split {mx(got):.3e} fp32 {mx(got32):.3e}, bound {MAX_REL * scale:.3e}, max |ref| {scale:.3e}")
    assert mx(got32) <= MAX_REL * scale, "the fp32 kernel itself misses the max bound"
    assert not torch.equal(got, got32), "the split path did not run"
    assert rms(got) <= ERR_FACTOR * rms(got32)
    assert mx(got) <= MAX_REL * scale


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("name", ACT_CASES)
def test_activation_magnitudes(name, shape, monkeypatch):
    g, x, w, b, gamma, beta = _base(shape)
    x, w, b = _act_case(name, g, x, w, b)
    _check_accuracy(name, x, w, b, gamma, beta, monkeypatch)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("name", WEIGHT_CASES)
def test_weight_magnitudes(name, shape, monkeypatch):
    g, x, w, b, gamma, beta = _base(shape)
    x, w, b = _weight_case(name, g, x, w, b)
    _check_accuracy(name, x, w, b, gamma, beta, monkeypatch)


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[0]], ids=str)
def test_image_independent_of_its_batch(shape, monkeypatch):
    """Image 0 alone, with six images like it, and beside a neighbour 2^20 louder: the same bits."""
    cin, cout, B, H, W = shape
    g, x, w, b, gamma, beta = _base((cin, cout, 7, H, W), "batch")
    x = x * 1e-3
    plan = _plan(w, b, gamma, beta)
    alone = _run(plan, x[:1].contiguous(), monkeypatch)
    seven = _run(plan, x, monkeypatch)
    loud = _run(plan, torch.cat([x[:1], x[1:2] * 2.0 ** 20]), monkeypatch)
    assert torch.equal(alone[0], seven[0])
    assert torch.equal(alone[0], loud[0])
    assert torch.equal(_run(plan, (x[1:2] * 2.0 ** 20).contiguous(), monkeypatch)[0], loud[1])


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[0]], ids=str)
def test_patch_equals_direct_scaled(shape, monkeypatch):
    """Images of different magnitudes in one tile: the LDS patch and the direct loads (BASIC_CONV_DEBUG bit 1024) agree."""
    g, x, w, b, gamma, beta = _base(shape, "sources")
    x, w, b = _act_case("two-images", g, x, w, b)
    plan = _plan(w, b, gamma, beta)
    assert torch.equal(_run(plan, x, monkeypatch), _run(plan, x, monkeypatch, debug="1032"))


def test_all_zero_image(monkeypatch):
    """An all-zero image (no scale to derive) gives exactly the fp32 kernel's output: the bias through the IGDN."""
    g, x, w, b, gamma, beta = _base(SHAPES[3], "zero")
    x[2] = 0
    plan = _plan(w, b, gamma, beta)
    got, got32 = _run(plan, x, monkeypatch), _run(plan, x, monkeypatch, f32=True)
    assert torch.equal(got[2], got32[2])
    assert not torch.equal(got[1], got32[1]), "the split path did not run"
    zeros = torch.zeros_like(x)
    assert torch.equal(_run(plan, zeros, monkeypatch), _run(plan, zeros, monkeypatch, f32=True))


def test_infinity_stays_in_its_image(monkeypatch):
    """An image that holds an infinity leaves the other images of the batch, its tile-mates included, as they were."""
    g, x, w, b, gamma, beta = _base(SHAPES[3], "inf")
    plan = _plan(w, b, gamma, beta)
    clean = _run(plan, x, monkeypatch)
    x[1, 17, 3, 4] = float("inf")
    got = _run(plan, x, monkeypatch)
    for i in (0, 2, 3, 4):
        assert torch.equal(got[i], clean[i]), i
    assert not bool(torch.isfinite(got[1]).all())
