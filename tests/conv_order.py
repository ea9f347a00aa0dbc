"""An ordered fp32 reference for the plain-activation layers of the fp32 tap kernel (conv_tap_mfma_kernel), written from the
description in DESIGN.md, "K order of the fp32 tap kernel", not from the kernel or its packed weights:

    out[b, co, o] = act(bias[co] (+) chain)          (+): one fp32 add after the chain
    chain:  acc = 0;  for stage (ck input channels), for tap, for channel pair (c, c + 1) of the stage:
                acc = fma32(x[c + 1], w[c + 1], fma32(x[c], w[c], acc))

with x the input element the tap reads (zero outside the image and for channels >= cin, whose weights are zero too), every fma32
exactly rounded (one rounding of x * w + acc: what scripts/micro/mfma_arith.hip measured for v_mfma_f32_32x32x2_f32, k = 0 first,
profiles/r03_mfma_arith.txt), ReLU a select and Leaky ReLU the single product float32(0.01) * v.

A schedule is a list of phases (the sub-pixel phases of a transposed layer; one phase for a convolution), each with its ordered
taps and its channels per stage.  canonical_schedule() builds it from the rule alone:

  * a convolution: one phase, the k x k taps row-major; a transposed convolution of stride s: s x s phases, phase (py, px) holding
    the taps with ky = (py + p) mod s (kx alike), ordered by the patch position they read (row-major in (dy, dx), dy = (py + p -
    ky) / s: descending ky and kx);
  * channels per stage by the taps of the phase: more than 9 -> 2, 7..9 -> 4, at most 6 -> 8;
  * a stride-2 transposed layer whose column phases fuse (px = 1 reads a sub-grid of the columns px = 0 reads, 3 x (3 | 2) or
    2 x (3 | 2) taps: the 5 x 5, p = 2 layers): 4 channels per stage in every phase, each phase accumulating only its own taps;
  * channel pairs ascend, k = 0 before k = 1.

The keyword-only arguments of ordered_reference() restate mistakes, only to show that the reference tells them apart."""
import zlib
from collections import namedtuple

import numpy as np

ACT_NONE, ACT_RELU, ACT_LEAKY = "none", "relu", "leaky"
F32, F64 = np.float32, np.float64

# w: [cout, cin, k, k], or [cin, cout, k, k] for a transposed layer; b: [cout] or None
Layer = namedtuple("Layer", "w b k s p op tr act")
Tap = namedtuple("Tap", "ky kx dy dx")
Phase = namedtuple("Phase", "oy0 ox0 s_in s_out taps ck")


def seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


# ------------------------------------------------------------------------------------------------------------ exactly rounded fma
def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, element-wise on float32 arrays.  The product of two fp32 values is exact in fp64; the
    fp64 sum with c is rounded to odd (its error from TwoSum: a nonzero error makes the last bit sticky), and a value rounded to odd
    at 53 bits rounds to 24 bits as the exact value does."""
    p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
    c = np.asarray(c, F32).astype(F64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                       # s + e == p + c exactly
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where((e != 0) & even, np.nextafter(s, toward), s)
    return s.astype(F32)


def fma32_naive(a, b, c):
    """Two roundings (fp64, then fp32): wrong where the fp64 sum lands on an fp32 tie that the exact value misses."""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


# ------------------------------------------------------------------------------------------------------------------- the schedule
def stage_channels(ntaps):
    return 2 if ntaps > 9 else (4 if ntaps > 6 else 8)


def _phase_axis(layer, ph):
    """(k index, shift) of the taps phase `ph` keeps along one axis, ordered by shift (the patch position)."""
    if not layer.tr:
        return [(k, k - layer.p) for k in range(layer.k)]
    taps = [(k, (ph + layer.p - k) // layer.s) for k in range(layer.k) if (ph + layer.p - k) % layer.s == 0]
    return sorted(taps, key=lambda t: t[1])


def canonical_schedule(layer, ck=None):
    """The rule of the module docstring; `ck` overrides the channels per stage of every phase (the CPU tests' other schedules)."""
    nph = layer.s if layer.tr else 1
    axes = [_phase_axis(layer, ph) for ph in range(nph)]
    fused = False
    if layer.tr and layer.s == 2:
        a, b = axes
        # px = 1 reads 2 of the 3 patch columns px = 0 reads, the right-hand ones; the row phases have 3 and 2 rows alike
        fused = len(a) == 3 and len(b) == 2 and a[2][1] - a[0][1] == 2 and b[1][1] - b[0][1] == 1 and b[0][1] - a[0][1] == 1
    phases = []
    for py in range(nph):
        for px in range(nph):
            taps = [Tap(ky, kx, dy, dx) for ky, dy in axes[py] for kx, dx in axes[px]]
            per = ck if ck is not None else (4 if fused else stage_channels(len(taps)))
            phases.append(Phase(py, px, 1 if layer.tr else layer.s, layer.s if layer.tr else 1, taps, per))
    return phases


def out_hw(layer, h, w):
    if layer.tr:
        return tuple((n - 1) * layer.s - 2 * layer.p + layer.k + layer.op for n in (h, w))
    return tuple((n + 2 * layer.p - layer.k) // layer.s + 1 for n in (h, w))


# ------------------------------------------------------------------------------------------------------------------ the reference
def ordered_reference(layer, x, schedule, *, swap_pair=False, transpose_taps=False, bias_first=False):
    """-> float32 [B, cout, oh, ow].  One vectorised numpy step per (stage, tap, channel pair)."""
    x = np.asarray(x, F32)
    w = np.asarray(layer.w, F32)
    B, cin, H, W = x.shape
    cout = w.shape[1] if layer.tr else w.shape[0]
    assert (w.shape[0] if layer.tr else w.shape[1]) == cin and layer.act in (ACT_NONE, ACT_RELU, ACT_LEAKY)
    bias = np.zeros(cout, F32) if layer.b is None else np.asarray(layer.b, F32)
    oh, ow = out_hw(layer, H, W)
    out = np.zeros((B, cout, oh, ow), F32)
    zero_w = np.zeros((1, cout, 1, 1), F32)
    for ph in schedule:
        mh, mw = -(-(oh - ph.oy0) // ph.s_out), -(-(ow - ph.ox0) // ph.s_out)
        if mh <= 0 or mw <= 0:
            continue
        my, mx = np.arange(mh)[:, None], np.arange(mw)[None, :]
        taps = sorted(ph.taps, key=lambda t: (t.dx, t.dy)) if transpose_taps else ph.taps

        def operands(c, t):
            """x [B, 1, mh, mw] and w [1, cout, 1, 1] of input channel c under tap t: zeros for a padded channel or position."""
            if c >= cin:
                return np.zeros((B, 1, mh, mw), F32), zero_w
            iy, ix = my * ph.s_in + t.dy, mx * ph.s_in + t.dx
            inside = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            xv = np.where(inside, x[:, c][:, np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)], F32(0))
            wv = w[c, :, t.ky, t.kx] if layer.tr else w[:, c, t.ky, t.kx]
            return xv.reshape(B, 1, mh, mw), wv.reshape(1, cout, 1, 1)

        acc = np.zeros((B, cout, mh, mw), F32)
        if bias_first:
            acc = acc + bias.reshape(1, cout, 1, 1)
        for c0 in range(0, cin, ph.ck):
            for t in taps:
                for c in range(c0, c0 + ph.ck, 2):
                    k0, k1 = (c + 1, c) if swap_pair else (c, c + 1)
                    x0, w0 = operands(k0, t)
                    x1, w1 = operands(k1, t)
                    acc = fma32(x1, w1, fma32(x0, w0, acc))
        v = acc if bias_first else acc + bias.reshape(1, cout, 1, 1)       # one fp32 add
        if layer.act == ACT_RELU:
            v = np.where(v > 0, v, F32(0))
        elif layer.act == ACT_LEAKY:
            v = np.where(v > 0, v, F32(0.01) * v)                          # one fp32 product
        out[:, :, ph.oy0::ph.s_out, ph.ox0::ph.s_out] = v
    return out


# ----------------------------------------------------------------------------------------------------------------------- the cases
# cin cout k s p op tr act H W: the layers of tests/test_gpu_conv_order.py (B = 3 for the reference, 5 for the batch checks)
Shape = namedtuple("Shape", "cin cout k s p op tr act H W")
CASES = {
    # mt 4: the whole-cout launch against the 32-channel slices; cin ragged against a stage of 4, not against a stage of 2
    "ha5_128": Shape(18, 128, 5, 2, 2, 0, False, ACT_RELU, 13, 18),
    "ha5_256": Shape(18, 256, 5, 2, 2, 0, False, ACT_LEAKY, 13, 18),      # two chunks of mt 4
    "k4_128": Shape(12, 128, 4, 2, 1, 0, False, ACT_NONE, 9, 10),         # runtime tap table, 16 taps; 4 images per tile
    "ha5_64": Shape(18, 64, 5, 2, 2, 0, False, ACT_RELU, 13, 18),         # mt 2, 3, 5, 6
    "ha5_96": Shape(18, 96, 5, 2, 2, 0, False, ACT_RELU, 13, 18),
    "ha5_160": Shape(18, 160, 5, 2, 2, 0, False, ACT_RELU, 13, 18),
    "ha5_192": Shape(18, 192, 5, 2, 2, 0, False, ACT_RELU, 13, 18),
    "ha3_128": Shape(20, 128, 3, 1, 1, 0, False, ACT_LEAKY, 5, 6),        # first h_a layer; 2 images per tile
    "hs3_384": Shape(24, 384, 3, 1, 1, 0, False, ACT_NONE, 5, 6),         # last h_s layer of the mean-scale graph
    "hs5t_128": Shape(20, 128, 5, 2, 2, 1, True, ACT_RELU, 6, 7),         # fused column phases, whole and sliced
    "hs5t_192": Shape(20, 192, 5, 2, 2, 1, True, ACT_LEAKY, 6, 7),        # mt 6: four separate phases against fused slices
    "hs5t_100": Shape(20, 100, 5, 2, 2, 1, True, ACT_RELU, 6, 7),         # ragged last slice
}
BATCH = 5        # images generated per case
REF_BATCH = 3    # ... of which the ordered reference evaluates the first three


def sensitive(shape, generator_seed):
    """randn * 2^k, k uniform in -6..6 per element: partial sums of very different magnitudes, so that the order of the additions
    shows in the last bits of most outputs."""
    rng = np.random.default_rng(generator_seed)
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-6, 7, shape))).astype(F32)


def case_data(name):
    """(Layer, x [BATCH, cin, H, W]) of a case: order-sensitive activations, weights scaled as a trained layer's
    (conv_ref._layer(integer=False))."""
    c = CASES[name]
    rng = np.random.default_rng(seed(name, "order"))
    wshape = (c.cin, c.cout, c.k, c.k) if c.tr else (c.cout, c.cin, c.k, c.k)
    w = (rng.standard_normal(wshape) / (c.cin * c.k * c.k) ** 0.5).astype(F32)
    b = (rng.standard_normal(c.cout) * 0.1).astype(F32)
    x = sensitive((BATCH, c.cin, c.H, c.W), seed(name, "x"))
    return Layer(w, b, c.k, c.s, c.p, c.op, c.tr, c.act), x
