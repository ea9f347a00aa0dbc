"""The fused MS-SSIM kernels (csrc/msssim.hip, basic_msssim_per_image_dev) against the fp64 evaluation of tests/msssim_exact.py.

Bounds: |hip - fp64| <= 4 * dev32 on the per-image values and <= 4 * dev32_terms on the [B, C, 5] terms, where dev32 and
dev32_terms are the distances of the package's fp32 torch restatement (on the CPU) from the same fp64 evaluation, measured in
this session over the same cases.  Why 4: the kernel is another fp32 evaluation of the same formula with another summation
order (tile sums instead of a flat mean), so it may sit a few times as far from fp64 as the restatement does; a tap off by one,
a wrong pooling divisor or padding side, a lost row at a tile seam or a missing clamp each move a term by 1e-4 or more, and a
1 x 1 map makes it total.  Then the closed forms, bitwise independence of the batch, the dispatch of ``ms_ssim`` and of its two
callers, and the argument checks."""
import numpy as np
import pytest
import torch

import msssim_exact as E

pytestmark = pytest.mark.gpu


def _K():
    from cbench_basic_amd.nn import kernels
    return kernels


def _M():
    from cbench_basic_amd.benchmark import ms_ssim
    return ms_ssim


def _bounds():
    dev32, dev32_terms = E.restatement_deviation(_M())
    return 4 * dev32, 4 * dev32_terms


def _hip(case):
    r = E.reference(case)
    v, t = _K().ms_ssim_per_image(r["x"].cuda(), r["y"].cuda(), return_terms=True)
    return v.cpu().double().numpy(), t.cpu().double().numpy()


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_value_and_terms_vs_fp64(case):
    tol, tol_terms = _bounds()
    r, (rvalue, rterms) = E.reference(case), E.restatement(case, _M())
    v, t = _hip(case)
    assert v.shape == r["value"].shape and t.shape == r["terms"].shape
    dv, dt = np.abs(v - r["value"]).max(), np.abs(t - r["terms"]).max()
    print(f"{E.case_id(case)}: value dev hip {dv:.3e} restatement {np.abs(rvalue - r['value']).max():.3e} bound {tol:.3e} | "
          f"terms dev hip {dt:.3e} restatement {np.abs(rterms - r['terms']).max():.3e} bound {tol_terms:.3e}")
    assert np.isfinite(v).all() and np.isfinite(t).all()
    assert dv <= tol
    assert dt <= tol_terms


@pytest.mark.parametrize("shape", E.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("base", E.BASES)
def test_closed_forms(shape, base):
    v, t = _hip((shape, base, "same"))
    assert np.abs(v - 1).max() <= 1e-6 and np.abs(t - 1).max() <= 1e-6
    v, t = _hip((shape, base, "inverse"))
    assert (v == 0.0).all()
    assert np.isfinite(v).all() and np.isfinite(t).all() and (t >= 0).all()


@pytest.mark.parametrize("shape", [(3, 1, 163, 190), (2, 3, 161, 161)], ids=lambda s: "x".join(map(str, s)))
def test_batch_independence_bitwise(shape):
    K = _K()
    r = E.reference((shape, "rand", "n0.05"))
    x, y = r["x"].cuda(), r["y"].cuda()
    v, t = K.ms_ssim_per_image(x, y, return_terms=True)
    B, C, H, W = shape
    need = _lib().lib().basic_msssim_workspace_bytes(1, C, H, W)
    side = torch.cuda.Stream()
    for i in range(B):
        vi, ti = K.ms_ssim_per_image(x[i:i + 1], y[i:i + 1], return_terms=True)
        assert torch.equal(vi, v[i:i + 1]) and torch.equal(ti, t[i:i + 1])
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            vs = K.ms_ssim_per_image(x[i:i + 1], y[i:i + 1])
        side.synchronize()
        assert torch.equal(vs, v[i:i + 1])
        big = torch.empty((2 * need + 4096,), device="cuda", dtype=torch.uint8)
        vb = K.ms_ssim_per_image(x[i:i + 1], y[i:i + 1], workspace=big)
        assert torch.equal(vb, v[i:i + 1])
    # position in the batch: the images in reverse order
    vr = K.ms_ssim_per_image(x.flip(0), y.flip(0))
    assert torch.equal(vr.flip(0), v)


def _lib():
    from cbench_basic_amd import _lib
    return _lib


def _count_kernel_calls(monkeypatch):
    K = _K()
    calls, real = [], K.ms_ssim_per_image

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(K, "ms_ssim_per_image", counted)
    return calls


def test_dispatch(monkeypatch):
    K, M = _K(), _M()
    case = ((1, 3, 176, 208), "rand", "n0.05")
    r = E.reference(case)
    x, y = r["x"].cuda(), r["y"].cuda()
    want = K.ms_ssim_per_image(x, y)
    calls = _count_kernel_calls(monkeypatch)
    assert torch.equal(M.ms_ssim(x, y, size_average=False), want) and len(calls) == 1
    assert torch.equal(M.ms_ssim(x, y), want.mean()) and len(calls) == 2
    # the torch path is still there, on the same device, and agrees within the bounds of the first test
    tol, _ = _bounds()
    via_torch = M.ms_ssim(x, y, size_average=False, impl="torch")
    assert len(calls) == 2 and via_torch.is_cuda
    assert np.abs(via_torch.cpu().double().numpy() - r["value"]).max() <= tol
    # anything but the default window, weights and K stays on the torch path; the shape checks stand in front of both
    M.ms_ssim(x, y, win_sigma=1.0)
    M.ms_ssim(x, y, K=(0.01, 0.02))
    assert len(calls) == 2
    with pytest.raises(ValueError):
        M.ms_ssim(x[..., :160, :], y[..., :160, :])
    with pytest.raises(ValueError):
        M.ms_ssim(x, y[:, :2])
    assert len(calls) == 2


def test_noncontiguous_reconstruction():
    K = _K()
    r = E.reference(((1, 3, 176, 208), "rand", "n0.05"))
    x = r["x"].cuda()
    wide = torch.zeros(1, 3, 180, 216, device="cuda")
    wide[..., :176, :208] = r["y"].cuda()
    rec = wide.narrow(2, 0, 176).narrow(3, 0, 208)
    assert not rec.is_contiguous()
    assert torch.equal(K.ms_ssim_per_image(rec, x), K.ms_ssim_per_image(rec.contiguous(), x))


def test_callers_land_in_the_kernel(monkeypatch):
    from cbench_basic_amd.benchmark import PytorchBatchedDistortion
    from cbench_basic_amd.modules.entropy_coder.latent_graph import LossyDummyEntropyCoder
    K = _K()
    r = E.reference(((2, 3, 161, 161), "rand", "n0.05"))
    x, y = r["x"].cuda(), r["y"].cuda()
    v = K.ms_ssim_per_image(y, x)
    calls = _count_kernel_calls(monkeypatch)

    res = PytorchBatchedDistortion(metrics=["psnr", "ms-ssim"])(y, x)
    assert len(calls) == 1 and list(res) == ["psnr", "ms-ssim"]
    assert res["ms-ssim"] == float(v.mean())

    lam = 0.37
    coder = LossyDummyEntropyCoder(lambda_rd=lam, distortion_type="ms-ssim")
    wide = torch.zeros(2, 3, 176, 176, device="cuda")
    wide[..., :161, :161] = y
    out = coder(x, prior=wide)
    assert len(calls) == 2 and out.shape == x.shape
    md = coder.get_raw_cache("metric_dict")
    assert torch.equal(md["ms_ssim"], v.mean())
    want = (1 - v).mean() * (3 * 161 * 161) * lam   # lambda x mean(1 - v) x elements, in the coder's order
    assert torch.equal(md["weighted_distortion"], want)


def test_argument_checks():
    """Refused before any launch: nothing here reaches a kernel."""
    L = _lib()
    K = _K()
    x = torch.rand(1, 1, 161, 161, device="cuda")
    with pytest.raises(L.BasicHipError) as e:
        K.ms_ssim_per_image(x[..., :160, :], x[..., :160, :])
    assert "160" in str(e.value)
    need = L.lib().basic_msssim_workspace_bytes(1, 1, 161, 161)
    short = torch.empty((need - 1,), device="cuda", dtype=torch.uint8)
    with pytest.raises(L.BasicHipError) as e:
        K.ms_ssim_per_image(x, x, workspace=short)
    assert "workspace" in str(e.value)
    ws = torch.empty((need,), device="cuda", dtype=torch.uint8)
    with pytest.raises(L.BasicHipError) as e:
        L.check(L.lib().basic_msssim_per_image_dev(x.data_ptr(), x.data_ptr(), 1, 1, 161, 161, 1.0, ws.data_ptr(), need, None, None,
                                                   L.current_stream_ptr()))
    assert "null" in str(e.value)
    torch.cuda.synchronize()
