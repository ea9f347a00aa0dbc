"""The fp64 reference of a conv layer and the checks against it, shared by the conv tests (not a test module).

A layer is a `Case`; `_layer` draws its data, `_plan` builds the ConvPlan, `_linear64` / `_bound_a` are the fp64 reference and
the magnitude A = conv(|x|, |w|) + |b| that every summation error is relative to.

Checks:
  * exact integers (|x| <= 15, |w| <= 7, |b| <= 64, every partial sum < 2^20): products and sums are exact in any order
    and in one bf16 piece, so linear and ReLU outputs equal the fp64 reference bit for bit, Leaky ReLU equals fp32 of the
    exact value times 0.01f, and GDN / IGDN with gamma = 0 and beta in {1/4, 1, 4, 16} per channel is the linear output
    times a power of two, within the one rsq / sqrt rounding (2^-21 relative);
  * randn data: |got - ref64| <= TAU * A element-wise (GDN / IGDN with gamma = 0, beta = 1); with a real gamma, that bound
    propagated to first order through the normalisation;
  * guard bands: inputs as views into NaN-filled buffers, outputs as views into buffers whose bands hold a NaN of a fixed
    payload: every output element written, the bands bitwise unchanged.
"""
import math
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

TAU = 2.0 ** -20           # per-element error bound relative to A = conv(|x|, |w|) + |b| (fp32 chain: DESIGN.md §12)
GDN_REL = 2.0 ** -21       # one rsq / sqrt rounding
SPLIT_RMS_FACTOR = 1.5     # split-bf16 RMS(err / A) against the fp32 kernel's on the same inputs
RMS_FLOOR = 2.0 ** -26     # ... plus a quarter ulp, for layers so small that the fp32 kernel's error is almost zero
GUARD = 0x7FC0BEEF         # NaN payload of the guard bands
BAND = 256                 # floats of guard band on each side of a view

Case = namedtuple("Case", "cin cout k s p op tr act B H W debug launches")


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


def _code(act):
    from cbench_basic_amd.nn import kernels as K
    return dict(none=K.ACT_NONE, relu=K.ACT_RELU, leaky=K.ACT_LEAKY_RELU, gdn=K.ACT_GDN, igdn=K.ACT_IGDN)[act]


def _layer(c, integer, seed, gamma_kind="zero", bias=True):
    """x, w, b, gamma, beta of case c: small integers, or randn data scaled as a trained layer's."""
    g = torch.Generator().manual_seed(seed)
    wshape = (c.cin, c.cout, c.k, c.k) if c.tr else (c.cout, c.cin, c.k, c.k)
    if integer:
        x = torch.randint(-15, 16, (c.B, c.cin, c.H, c.W), generator=g).float()
        w = torch.randint(-7, 8, wshape, generator=g).float()
        b = torch.randint(-64, 65, (c.cout,), generator=g).float()
    else:
        x = torch.randn(c.B, c.cin, c.H, c.W, generator=g)
        w = torch.randn(wshape, generator=g) * (1.0 / (c.cin * c.k * c.k) ** 0.5)
        b = torch.randn(c.cout, generator=g) * 0.1
    gamma = beta = None
    if c.act in ("gdn", "igdn"):
        if gamma_kind == "zero":   # the normalisation is a per-channel power of two (integers) or 1 (randn)
            gamma = torch.zeros(c.cout, c.cout)
            beta = (torch.tensor([0.25, 1.0, 4.0, 16.0])[torch.randint(0, 4, (c.cout,), generator=g)] if integer
                    else torch.ones(c.cout))
        else:
            gamma = torch.rand(c.cout, c.cout, generator=g) * 0.02 + 0.1 * torch.eye(c.cout)
            beta = torch.rand(c.cout, generator=g) + 0.5
    return x, w, (b if bias else None), gamma, beta


def _plan(c, w, b, gamma, beta, **kw):
    from cbench_basic_amd.nn import kernels as K
    return K.ConvPlan(w, b, c.s, c.p, c.op, c.tr, _code(c.act), gamma, beta, **kw)


def _linear64(c, x, w, b):
    x, w = x.double(), w.double()
    b = b.double() if b is not None else None
    if c.tr:
        return F.conv_transpose2d(x, w, b, stride=c.s, padding=c.p, output_padding=c.op)
    return F.conv2d(x, w, b, stride=c.s, padding=c.p)


def _bound_a(c, x, w, b):
    """A = conv(|x|, |w|) + |b| in fp64: what every summation error of an output element is relative to."""
    return _linear64(c, x.abs(), w.abs(), b.abs() if b is not None else None)


def _set_env(monkeypatch, debug="", f32=False):
    if debug:
        monkeypatch.setenv("BASIC_CONV_DEBUG", debug)
    else:
        monkeypatch.delenv("BASIC_CONV_DEBUG", raising=False)
    if f32:
        monkeypatch.setenv("BASIC_CONV_F32", "1")
    else:
        monkeypatch.delenv("BASIC_CONV_F32", raising=False)


def _run(plan, x, monkeypatch, debug="", f32=False):
    _set_env(monkeypatch, debug, f32)
    out = plan(x.cuda())
    torch.cuda.synchronize()
    return out.cpu()


def _check_exact(c, got, lin, beta):
    """Integer data: bit for bit (linear, ReLU, Leaky ReLU's one fp32 multiply), power-of-two GDN factor within 2^-21."""
    assert got.shape == lin.shape
    got = got.double()
    if c.act in ("gdn", "igdn"):
        f = beta.double().reshape(1, -1, 1, 1) ** (0.5 if c.act == "igdn" else -0.5)
        ref = lin * f
        err = (got - ref).abs()
        bad = err > GDN_REL * ref.abs()
        assert not bad.any(), f"{int(bad.sum())} elements off, first at {bad.nonzero()[0].tolist()}: " \
                              f"got {float(got[bad][0])}, want {float(ref[bad][0])}"
        return
    if c.act == "relu":
        ref = lin.clamp(min=0)
    elif c.act == "leaky":
        ref = torch.where(lin > 0, lin, (lin.float() * torch.tensor(0.01, dtype=torch.float32)).double())
    else:
        ref = lin
    bad = got != ref
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}: " \
                          f"got {float(got[bad][0])}, want {float(ref[bad][0])}"


def _ref_plain(c, lin):
    """fp64 reference of a randn layer whose GDN / IGDN (gamma = 0, beta = 1) is the identity."""
    if c.act == "relu":
        return lin.clamp(min=0)
    if c.act == "leaky":
        return torch.where(lin > 0, lin, lin * 0.01)
    return lin


def _err_ratio(c, got, lin, A):
    """|got - ref64| / A per element (the Leaky ReLU slope's own fp32 rounding taken out)."""
    ref = _ref_plain(c, lin)
    err = (got.double() - ref).abs()
    if c.act == "leaky":
        err = (err - 2.0 ** -23 * ref.abs()).clamp(min=0)
    return err / A.clamp(min=1e-30)


def _check_bound(c, got, lin, A, what):
    r = _err_ratio(c, got, lin, A)
    worst = float(r.max())
    print(f"{what}: max |err| / A = {worst:.3e} (tau {TAU:.3e}), rms {float(r.pow(2).mean().sqrt()):.3e}")
    assert worst <= TAU, f"{what}: max |err| / A = {worst:.3e} > tau at {np.unravel_index(int(r.argmax()), r.shape)}"
    return r


def _gdn_bound(c, got, lin, A, gamma, beta):
    """Real gamma: the bound TAU * A on y = conv + b, propagated to first order through y * sqrt(n) (IGDN) or
    y * rsqrt(n) (GDN), n = beta + gamma . y^2, plus the fp32 norm GEMM's own rounding and the rsq / sqrt rounding."""
    cout = lin.shape[1]
    gm = gamma.double().reshape(cout, cout, 1, 1)
    ey = TAU * A
    n = F.conv2d(lin * lin, gm, beta.double())
    dn = F.conv2d(2 * lin.abs() * ey, gm) + (cout + 2) * 2.0 ** -24 * n
    sq = n.sqrt()
    if c.act == "igdn":
        ref = lin * sq
        bound = sq * ey + lin.abs() * dn / (2 * sq)
    else:
        ref = lin / sq
        bound = ey / sq + lin.abs() * dn / (2 * n * sq)
    bound = bound + GDN_REL * ref.abs()
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"gdn bound: max err / bound = {worst:.3f}")
    assert worst <= 1.0
    scale = max(1.0, float(ref.abs().max()))   # the suite's existing criterion beside it
    assert float(err.max()) <= 1e-4 * scale


# ---------------------------------------------------------------------------------------------------------------------
# guard bands and alignment


def _in_view(x, off):
    """x as a contiguous view `off` floats into a NaN-filled device buffer (plus a NaN band after it)."""
    buf = torch.full((off + x.numel() + BAND,), float("nan"), device="cuda")
    v = buf[off: off + x.numel()].view(x.shape)
    v.copy_(x.cuda())
    return v


def _out_view(shape, off):
    """A view `off` floats into a buffer: the region NaN, the bands a NaN of payload GUARD."""
    n = math.prod(shape)
    buf = torch.full((off + n + BAND,), GUARD, dtype=torch.int32, device="cuda").view(torch.float32)
    buf[off: off + n] = float("nan")
    return buf, buf[off: off + n].view(shape)


def _guarded_run(plan, c, x, in_off, out_off, monkeypatch, debug):
    _set_env(monkeypatch, debug)
    xv = _in_view(x, in_off)
    oh, ow = plan.out_hw(c.H, c.W)
    buf, ov = _out_view((c.B, c.cout, oh, ow), out_off)
    plan(xv, out=ov)
    torch.cuda.synchronize()
    bands = buf.view(torch.int32).cpu()
    n = ov.numel()
    assert bool((bands[:out_off] == GUARD).all()) and bool((bands[out_off + n:] == GUARD).all()), \
        "the kernel wrote outside its output tensor"
    got = ov.cpu()
    assert not bool(torch.isnan(got).any()), \
        f"{int(torch.isnan(got).sum())} output elements unwritten or fed by a value outside the input tensor"
    return got


def _out_offsets(c):
    # the cout <= 3 kernels store 8-byte pairs with no host-side alignment check: 8-byte aligned offsets only
    return (64, 2) if c.cout <= 3 else (64, 1)
