"""GPU: the split-bf16 path of the synthesis transform's 128-channel layers (conv_split_bf16_kernel).

  * each targeted layer shape against an fp64 CPU reference: RMS error within 1.5x the fp32 kernel's (BASIC_CONV_F32=1),
  * the layers whose output is coded (analysis, hyper synthesis) stay on the fp32 kernel: the codec's bitstream on bench
    images is byte for byte the fp32 path's, and only the reconstruction moves, by fp32 rounding,
  * an image's output is bit-identical at batch 1, 7 and 32.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# cin, cout, transposed, act, B, H, W -- g_s layers 1..3 (5x5 s2 deconv + IGDN)
LAYERS = [
    (192, 128, True, "igdn", 2, 16, 16),
    (128, 128, True, "igdn", 2, 32, 32),
    (128, 128, True, "igdn", 1, 24, 40),
]
# the same geometries with an output that is coded (g_a: GDN, h_s: ReLU): never on the split path
FP32_ONLY = [
    (128, 128, False, "gdn", 2, 64, 64),
    (128, 128, True, "relu", 1, 24, 40),
]
ERR_FACTOR = 1.5


def _layer(case, seed_extra=0):
    cin, cout, tr, act, B, H, W = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()) % (2 ** 31) + seed_extra)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn((cin, cout, 5, 5) if tr else (cout, cin, 5, 5), generator=g) * (1.0 / (cin * 25) ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    gamma = beta = None
    if act in ("gdn", "igdn"):
        gamma = torch.rand(cout, cout, generator=g) * 0.02 + 0.1 * torch.eye(cout)
        beta = torch.rand(cout, generator=g) + 0.5
    return x, w, b, gamma, beta


def _reference64(case, x, w, b, gamma, beta):
    cin, cout, tr, act, B, H, W = case
    x, w, b = x.double(), w.double(), b.double()
    ref = F.conv_transpose2d(x, w, b, stride=2, padding=2, output_padding=1) if tr else F.conv2d(x, w, b, stride=2, padding=2)
    if act == "relu":
        ref = F.relu(ref)
    elif act in ("gdn", "igdn"):
        norm = F.conv2d(ref * ref, gamma.double().reshape(cout, cout, 1, 1), beta.double())
        ref = ref * (torch.sqrt(norm) if act == "igdn" else torch.rsqrt(norm))
    return ref


def _plan(case, w, b, gamma, beta):
    from cbench_basic_amd.nn import kernels as K
    cin, cout, tr, act, B, H, W = case
    code = dict(none=K.ACT_NONE, relu=K.ACT_RELU, gdn=K.ACT_GDN, igdn=K.ACT_IGDN)[act]
    return K.ConvPlan(w, b, 2, 2, 1 if tr else 0, tr, code, gamma, beta)


def _run(plan, x, monkeypatch, f32):
    # small test grids would take the 32-channel-slice variant for the plain-activation layers: forbid it (bit 8)
    monkeypatch.setenv("BASIC_CONV_DEBUG", "8")
    if f32:
        monkeypatch.setenv("BASIC_CONV_F32", "1")
    else:
        monkeypatch.delenv("BASIC_CONV_F32", raising=False)
    out = plan(x.cuda())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("case", LAYERS, ids=[str(c) for c in LAYERS])
def test_split_error_vs_fp64(case, monkeypatch):
    x, w, b, gamma, beta = _layer(case)
    ref = _reference64(case, x, w, b, gamma, beta)
    plan = _plan(case, w, b, gamma, beta)
    got_split = _run(plan, x, monkeypatch, f32=False)
    got_f32 = _run(plan, x, monkeypatch, f32=True)
    rms = lambda t: float(((t.double() - ref) ** 2).mean().sqrt())
    e_split, e_f32 = rms(got_split), rms(got_f32)
    scale = float(ref.abs().max())
    print(f"{case}: rms error split {e_split:.3e}, fp32 {e_f32:.3e}, max |ref| {scale:.3f}")
    assert not torch.equal(got_split, got_f32), "the split path did not run"
    assert e_split <= ERR_FACTOR * e_f32
    assert float((got_split.double() - ref).abs().max()) <= 1e-5 * max(1.0, scale)


@pytest.mark.parametrize("case", FP32_ONLY, ids=[str(c) for c in FP32_ONLY])
def test_coded_layers_stay_fp32(case, monkeypatch):
    """Layers whose output is quantised and coded give bit for bit the fp32 kernel's result."""
    x, w, b, gamma, beta = _layer(case)
    plan = _plan(case, w, b, gamma, beta)
    assert torch.equal(_run(plan, x, monkeypatch, f32=False), _run(plan, x, monkeypatch, f32=True))


@pytest.mark.parametrize("case", [LAYERS[0], LAYERS[1]], ids=lambda c: str(c))
def test_split_batch_invariant(case, monkeypatch):
    """One fixed K order per output element: image 0 comes out bit for bit the same at batch 1, 7 and 32."""
    cin, cout, tr, act, B, H, W = case
    x, w, b, gamma, beta = _layer((cin, cout, tr, act, 32, H, W))
    plan = _plan(case, w, b, gamma, beta)
    outs = [_run(plan, x[:n].contiguous(), monkeypatch, f32=False) for n in (1, 7, 32)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], outs[2][0])
    assert torch.equal(outs[1][3], outs[2][3])


def _bench_image(i, size=256):
    torch.manual_seed(int(i))
    return torch.rand(3, size, size)


def test_split_codec_vs_fp32_path(monkeypatch):
    """The codec on bench images with the split path against the fp32 path: identical latents, scales and symbols (the
    bitstream does not change), and a reconstruction within fp32 rounding of the fp32 path's."""
    from cbench_basic_amd.nn import kernels as K
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    codec = seed_synthetic_weights(hyperprior_codec(), seed=0).eval().to("cuda:0")
    codec.update_state()
    ec = codec.entropy_coder
    x = torch.stack([_bench_image(i) for i in range(4)]).cuda()

    def symbols(f32):
        if f32:
            monkeypatch.setenv("BASIC_CONV_F32", "1")
        else:
            monkeypatch.delenv("BASIC_CONV_F32", raising=False)
        y = ec.latent_inference_modules["x_y"](x)
        z = ec.latent_inference_modules["y_z"](y)
        zhat = ec.latent_node_entropy_coders["z"](z)
        scales = ec.latent_generative_modules["z_y"](zhat)[..., : y.shape[-2], : y.shape[-1]].contiguous()
        yc = ec.latent_node_entropy_coders["y"]
        yc._ready()
        sym, idx, _ = K.gc_quantize_index(y, scales, yc._scale_table_dev)
        xhat = ec.latent_generative_modules["y_x"](sym.float())
        torch.cuda.synchronize()
        return y.cpu(), zhat.cpu(), sym.cpu(), idx.cpu(), xhat.cpu()

    y32, z32, s32, i32, xh32 = symbols(True)
    ysp, zsp, ssp, isp, xhsp = symbols(False)
    print(f"split vs fp32: max |dxhat| {float((xhsp - xh32).abs().max()):.3e}")
    assert torch.equal(ysp, y32) and torch.equal(zsp, z32)
    assert torch.equal(ssp, s32) and torch.equal(isp, i32)
    assert not torch.equal(xhsp, xh32), "the split path did not run"
    assert float((xhsp - xh32).abs().max()) < 1e-4
