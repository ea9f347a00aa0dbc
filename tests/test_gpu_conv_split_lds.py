"""GPU: the two activation sources of the split-bf16 synthesis kernel (csrc/conv.hip conv_split_bf16_kernel).

The patch source stages each channel block's input patch in LDS, every value split once; the direct source loads and
splits the activations of every tap.  Both feed the MFMAs the same pieces in the same order, so a layer's output must be
the same bit for bit whichever source ran.  BASIC_CONV_DEBUG bit 1024 forces the direct source.  A tile whose patch,
TB x (TH + KH - 1) x (TW + 2) positions, exceeds the LDS left beside the weight stages (416 positions) always takes the
direct source.
"""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DIRECT = "1024"            # BASIC_CONV_DEBUG bit: split-bf16 activations by direct loads only
PATCH_POS = 416            # patch positions that fit beside the weight stages
TAU = 2.0 ** -20           # per-element error bound relative to A = conv(|x|, |w|) + |b| (as test_gpu_conv_paths.py)
SPLIT_RMS_FACTOR = 1.5
RMS_FLOOR = 2.0 ** -26

# (cin, cout, B, H, W, bias); every layer is a k5 s2 p2 op1 transposed conv + IGDN, H x W its input (= m-grid of both phases)
GS = [(192, 128, 16, 16), (128, 128, 32, 32), (128, 128, 64, 64)]   # g_s layers 1-3 of the hyperprior codec
CASES = [(ci, co, B, H, W, True) for ci, co, H, W in GS for B in (1, 7, 32)] + [
    # the geometry matrix of test_gpu_conv_paths.py (SPLIT_CASES)
    (16, 128, 1, 3, 5, True),
    (48, 97, 3, 1, 1, True),
    (112, 100, 1, 1, 7, True),
    (128, 127, 2, 5, 1, True),
    (144, 128, 1, 17, 9, True),
    (192, 97, 1, 8, 64, True),
    (192, 128, 1, 32, 48, True),
    (16, 100, 257, 1, 1, True),
    (48, 127, 257, 1, 1, True),
    (144, 97, 3, 17, 9, True),
    (128, 100, 3, 3, 5, False),
    (16, 97, 1, 8, 64, True),
    (192, 100, 1, 5, 1, False),
]
# patch larger than the LDS budget in both row phases (KH = 3 and 2): direct source only
FALLBACK = [(128, 128, 20, 4, 4, True), (64, 100, 5, 2, 16, True), (32, 128, 33, 1, 8, False)]


def _pow2_ceil(n):
    return 1 << (n - 1).bit_length()


def patch_positions(H, W, kh):
    """The host's tile choice restated: 256 positions = TB x TH x TW (TW <= 16), and the patch of such a tile."""
    tw = min(_pow2_ceil(W), 16)
    th = min(_pow2_ceil(H), 256 // tw)
    tb = 256 // (tw * th)
    return tb * (th + kh - 1) * (tw + 2)


def _id(sc):
    cin, cout, B, H, W, bias = sc
    src = "patch" if patch_positions(H, W, 2) <= PATCH_POS else "direct"
    return "cin%d-cout%d-B%d-%dx%d%s-%s" % (cin, cout, B, H, W, "" if bias else "-nobias", src)


def _layer(sc, seed, real_gamma=True):
    cin, cout, B, H, W, bias = sc
    g = torch.Generator().manual_seed(zlib.crc32(repr((sc, seed)).encode()) % (2 ** 31))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cin, cout, 5, 5, generator=g) * (1.0 / (cin * 25) ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1 if bias else None
    if real_gamma:
        gamma = torch.rand(cout, cout, generator=g) * 0.02 + 0.1 * torch.eye(cout)
        beta = torch.rand(cout, generator=g) + 0.5
    else:
        gamma, beta = torch.zeros(cout, cout), torch.ones(cout)
    return x, w, b, gamma, beta


def _plan(w, b, gamma, beta):
    from cbench_basic_amd.nn import kernels as K
    return K.ConvPlan(w, b, 2, 2, 1, True, K.ACT_IGDN, gamma, beta)


def _run(plan, x, monkeypatch, debug="", f32=False):
    if debug:
        monkeypatch.setenv("BASIC_CONV_DEBUG", debug)
    else:
        monkeypatch.delenv("BASIC_CONV_DEBUG", raising=False)
    if f32:
        monkeypatch.setenv("BASIC_CONV_F32", "1")
    else:
        monkeypatch.delenv("BASIC_CONV_F32", raising=False)
    out = plan(x if x.is_cuda else x.cuda())
    torch.cuda.synchronize()
    return out.cpu()


def _first_diff(a, b):
    bad = a != b
    i = tuple(bad.nonzero()[0].tolist())
    return f"{int(bad.sum())} of {bad.numel()} elements differ, first at {list(i)}: {float(a[i])} vs {float(b[i])}"


@pytest.mark.parametrize("sc", CASES, ids=_id)
def test_patch_equals_direct(sc, monkeypatch):
    """Real gamma (the IGDN epilogue at work): the default launch equals the forced direct source bit for bit, and
    differs from the fp32 kernel (the split path ran)."""
    x, w, b, gamma, beta = _layer(sc, "eq")
    plan = _plan(w, b, gamma, beta)
    monkeypatch.delenv("BASIC_CONV_DEBUG", raising=False)
    assert plan.launches(sc[2], sc[3], sc[4]) == 2
    got = _run(plan, x, monkeypatch)
    direct = _run(plan, x, monkeypatch, DIRECT)
    assert torch.equal(got, direct), _first_diff(got, direct)
    assert not torch.equal(got, _run(plan, x, monkeypatch, f32=True)), "the split-bf16 path did not run"


@pytest.mark.parametrize("sc", [c for c in CASES if patch_positions(c[3], c[4], 3) <= PATCH_POS][:6], ids=_id)
def test_patch_misaligned_input(sc, monkeypatch):
    """Inputs 4 and 8 bytes past a 16-byte boundary, inside NaN-filled buffers: the patch loads read only the tensor
    and give the aligned run's output bit for bit."""
    x, w, b, gamma, beta = _layer(sc, "align")
    plan = _plan(w, b, gamma, beta)
    ref = _run(plan, x, monkeypatch)
    for off in (1, 2):
        buf = torch.full((64 + off + x.numel() + 256,), float("nan"), device="cuda")
        xv = buf[64 + off: 64 + off + x.numel()].view(x.shape)
        xv.copy_(x.cuda())
        got = _run(plan, xv, monkeypatch)
        assert not bool(torch.isnan(got).any()), "a value outside the input tensor reached the output"
        assert torch.equal(got, ref), _first_diff(got, ref)


def test_slimmable_slice(monkeypatch):
    """A [192, 192, 5, 5] transposed weight at cin_active = cout_active = 128: both sources agree bit for bit."""
    from cbench_basic_amd.nn import kernels as K
    g = torch.Generator().manual_seed(7)
    w = torch.randn(192, 192, 5, 5, generator=g) * 0.02
    b = torch.randn(192, generator=g) * 0.1
    gamma = torch.rand(128, 128, generator=g) * 0.02 + 0.1 * torch.eye(128)
    beta = torch.rand(128, generator=g) + 0.5
    x = torch.randn(2, 128, 6, 10, generator=g)
    plan = K.ConvPlan(w, b, 2, 2, 1, True, K.ACT_IGDN, gamma, beta, cin_active=128, cout_active=128)
    assert patch_positions(6, 10, 3) <= PATCH_POS
    got, direct = _run(plan, x, monkeypatch), _run(plan, x, monkeypatch, DIRECT)
    assert torch.equal(got, direct), _first_diff(got, direct)


def _ratio(got, lin, A):
    return (got.double() - lin).abs() / A.clamp(min=1e-30)


@pytest.mark.parametrize("sc", FALLBACK, ids=_id)
def test_fallback_against_fp64(sc, monkeypatch):
    """Tiles whose patch does not fit take the direct source: within TAU * A of fp64 per element, RMS within 1.5x the
    fp32 kernel's (gamma = 0, beta = 1: the IGDN is the identity)."""
    assert patch_positions(sc[3], sc[4], 2) > PATCH_POS and patch_positions(sc[3], sc[4], 3) > PATCH_POS
    x, w, b, gamma, beta = _layer(sc, "fallback", real_gamma=False)
    plan = _plan(w, b, gamma, beta)
    got = _run(plan, x, monkeypatch)
    assert torch.equal(got, _run(plan, x, monkeypatch, DIRECT))
    got32 = _run(plan, x, monkeypatch, f32=True)
    assert not torch.equal(got, got32), "the split-bf16 path did not run"
    bd = b.double() if b is not None else None
    lin = F.conv_transpose2d(x.double(), w.double(), bd, stride=2, padding=2, output_padding=1)
    A = F.conv_transpose2d(x.double().abs(), w.double().abs(), bd.abs() if bd is not None else None,
                           stride=2, padding=2, output_padding=1)
    r, r32 = _ratio(got, lin, A), _ratio(got32, lin, A)
    assert float(r.max()) <= TAU, float(r.max())
    rms, rms32 = math.sqrt(float(r.pow(2).mean())), math.sqrt(float(r32.pow(2).mean()))
    assert rms <= SPLIT_RMS_FACTOR * rms32 + RMS_FLOOR, (rms, rms32)
