"""The premises of tests/conv_order.py and tests/test_gpu_conv_order.py, checked without a GPU:

  * fma32 is exactly rounded: equal to rational arithmetic on random operands and on constructed operands whose fp64 sum lands on an
    fp32 tie that the exact value misses, where rounding twice gives the wrong float;
  * on integer data (exact in any order) the ordered reference is the fp64 convolution bit for bit, under every schedule;
  * the order-sensitive data are order-sensitive: 2 and 4 channels per stage differ in at least a quarter of the outputs of every case;
  * the reference notices a wrong operator: a swapped channel pair, a transposed tap order, the bias added before the chain."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_order as co

MIN_SHARE = 0.25   # of the outputs, between 2 and 4 channels per stage (a condition on the inputs)


def _round_f32(q):
    """The float32 nearest the rational q (ties to even), normal range or zero."""
    if q == 0:
        return np.float32(0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1) and -126 <= e < 127
    scaled = q / Fraction(2) ** (e - 23)              # in [2^23, 2^24)
    n, rem = divmod(scaled, 1)
    n = int(n)
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(sign * float(n) * 2.0 ** (e - 23))   # n <= 2^24: exact in fp64, and the product is a float32


def _exact_fma(a, b, c):
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _tie_cases():
    """a * b = +-2^(j - 24) (1 - 2^-46) against c = +-2^j (1 + m 2^-23), m odd: the exact sum lies 2^(j - 70) below the tie between two
    floats, the fp64 sum exactly on it, and the tie goes to the even neighbour: the wrong one."""
    a, b, c = [], [], []
    for j in (-9, 0, 5):
        for m in (1, 3, 4097, 2 ** 23 - 1):
            for sign in (1.0, -1.0):
                a.append(np.float32(1 + 2.0 ** -23))
                b.append(np.float32(sign * (1 - 2.0 ** -23) * 2.0 ** (j - 24)))
                c.append(np.float32(sign * (1 + m * 2.0 ** -23) * 2.0 ** j))
    return np.array(a), np.array(b), np.array(c)


def test_fma32_is_exactly_rounded():
    rng = np.random.default_rng(co.seed("fma32"))
    n = 4000
    a = co.sensitive(n, co.seed("fma32", "a"))
    b = (rng.standard_normal(n) * 0.1).astype(np.float32)
    c = co.sensitive(n, co.seed("fma32", "c"))
    c[: n // 4] = -(a[: n // 4].astype(np.float64) * b[: n // 4]).astype(np.float32)     # cancellation: the sum is the product's tail
    got = co.fma32(a, b, c)
    want = np.array([_exact_fma(*t) for t in zip(a, b, c)])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))

    a, b, c = _tie_cases()
    want = np.array([_exact_fma(*t) for t in zip(a, b, c)])
    assert np.array_equal(co.fma32(a, b, c).view(np.uint32), want.view(np.uint32))
    wrong = co.fma32_naive(a, b, c) != want
    assert wrong.all(), "the constructed cases do not exercise the correction"


def _int_layer(name):
    """The integer data of conv_ref._layer(integer=True) at the case's shape: |x| <= 15, |w| <= 7, |b| <= 64."""
    c = co.CASES[name]
    g = torch.Generator().manual_seed(co.seed(name, "int"))
    wshape = (c.cin, c.cout, c.k, c.k) if c.tr else (c.cout, c.cin, c.k, c.k)
    x = torch.randint(-15, 16, (2, c.cin, c.H, c.W), generator=g).float()
    w = torch.randint(-7, 8, wshape, generator=g).float()
    b = torch.randint(-64, 65, (c.cout,), generator=g).float()
    return co.Layer(w.numpy(), b.numpy(), c.k, c.s, c.p, c.op, c.tr, c.act), x


def _fp64(layer, x):
    x, w, b = torch.as_tensor(x).double(), torch.as_tensor(layer.w).double(), torch.as_tensor(layer.b).double()
    if layer.tr:
        v = F.conv_transpose2d(x, w, b, stride=layer.s, padding=layer.p, output_padding=layer.op)
    else:
        v = F.conv2d(x, w, b, stride=layer.s, padding=layer.p)
    if layer.act == co.ACT_RELU:
        v = v.clamp(min=0)
    elif layer.act == co.ACT_LEAKY:
        v = torch.where(v > 0, v, (v.float() * torch.tensor(0.01, dtype=torch.float32)).double())
    return v.float().numpy()


INT_CASES = ["ha5_64", "k4_128", "ha3_128", "hs5t_100"]   # 5x5, 4x4 and 3x3 convolutions, the four phases of a transposed layer


@pytest.mark.parametrize("name", INT_CASES)
def test_integer_data_equal_fp64_under_every_schedule(name):
    layer, x = _int_layer(name)
    want = _fp64(layer, x)
    for ck in (None, 2, 4, 8):
        got = co.ordered_reference(layer, x.numpy(), co.canonical_schedule(layer, ck))
        assert got.shape == want.shape and np.array_equal(got, want), (name, ck)


def test_canonical_schedule_rule():
    """Channels per stage and tap order of the rule, spelt out for the layer classes of the cases."""
    def sched(name):
        return co.canonical_schedule(co.case_data(name)[0])
    (ph,) = sched("ha5_128")
    assert ph.ck == 2 and [(t.ky, t.kx) for t in ph.taps] == [(ky, kx) for ky in range(5) for kx in range(5)]
    assert [ph.ck for ph in sched("k4_128")] == [2] and [ph.ck for ph in sched("ha3_128")] == [4]
    phases = sched("hs5t_192")
    assert [(ph.oy0, ph.ox0, len(ph.taps), ph.ck) for ph in phases] == [(0, 0, 9, 4), (0, 1, 6, 4), (1, 0, 6, 4), (1, 1, 4, 4)]
    # patch order: ascending (dy, dx), i.e. descending (ky, kx)
    assert [(t.ky, t.kx, t.dy, t.dx) for t in phases[3].taps] == [(3, 3, 0, 0), (3, 1, 0, 1), (1, 3, 1, 0), (1, 1, 1, 1)]
    assert [(t.ky, t.dy) for t in phases[0].taps[::3]] == [(4, -1), (2, 0), (0, 1)]
    # a transposed layer whose column phases do not fuse: by the taps of each phase
    k3 = co.Layer(np.zeros((4, 8, 3, 3), np.float32), None, 3, 2, 1, 1, True, co.ACT_NONE)
    assert [(len(ph.taps), ph.ck) for ph in co.canonical_schedule(k3)] == [(1, 8), (2, 8), (2, 8), (4, 8)]


@pytest.mark.parametrize("name", list(co.CASES))
def test_cases_are_order_sensitive(name):
    layer, x = co.case_data(name)
    x = x[:1]
    a = co.ordered_reference(layer, x, co.canonical_schedule(layer, 2))
    b = co.ordered_reference(layer, x, co.canonical_schedule(layer, 4))
    share = float((a != b).mean())
    print(f"{name}: {share:.3f} of the outputs differ between 2 and 4 channels per stage")
    assert share >= MIN_SHARE, (name, share)


@pytest.mark.parametrize("name", ["ha5_64", "hs5t_100"])
def test_reference_notices_a_wrong_operator(name):
    layer, x = co.case_data(name)
    x = x[:1]
    sched = co.canonical_schedule(layer)
    want = co.ordered_reference(layer, x, sched)
    for wrong in ("swap_pair", "transpose_taps", "bias_first"):
        got = co.ordered_reference(layer, x, sched, **{wrong: True})
        share = float((got != want).mean())
        print(f"{name} {wrong}: {share:.3f} of the outputs change")
        assert share > 0, (name, wrong)
