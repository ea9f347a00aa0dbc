"""The quantiser-step kernels of csrc/entropy.hip through the C ABI (basic_gc_quantize_index_q_dev, basic_gc_dequantize_q_dev,
basic_gauss_nll_per_image_q_dev), exactly equal to the NumPy float32 restatement of tests/qstep_exact.py -- never to another kernel,
except where the claim IS the equality with one: at step 1 the outputs are those of basic_gc_quantize_index_dev /
basic_i32_to_f32_dev bit for bit.

Signed zero: the encoder's yhat = rint(y / step) * step keeps rint's -0.0, as today's kernel does; an integer symbol 0 decodes to
+0.0, as today's decoder does.  So the decoder's yhat has the encoder's bits wherever the symbol is not 0 and is the same float (a
zero) where it is (qstep_exact.same_reconstruction)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import qstep_exact as QX

pytestmark = pytest.mark.gpu

GUARD = 0x7FC0BEEF
FRESH = 0x7FC00001
BAND = 4096
BOUND = 0.11
ONE_PASS = 256 * 8 * 256     # elements of one grid pass: the grid is capped at 2048 workgroups of 256 threads
TABLE = torch.exp(torch.linspace(math.log(0.11), math.log(256), 64)).numpy().astype(np.float32)   # get_scale_table()


def _L():
    from cbench_basic_amd import _lib
    return _lib, _lib.lib()


def _guarded(n, off=64):
    buf = torch.full((off + n + BAND,), GUARD, dtype=torch.int32, device="cuda")
    buf[off: off + n] = FRESH
    return buf, buf[off: off + n]


def _intact(buf, n, off=64):
    h = buf.cpu()
    return bool((h[:off] == GUARD).all()) and bool((h[off + n:] == GUARD).all())


def _deciders(d, count=3):
    """Latents and scales at which the division's rounding decides under step d: a multiply by the float32 reciprocal gives another
    symbol (y next to a half-integer multiple of d) or another index (scale next to table[j] * d).  Found by search; none for a
    power of two, whose reciprocal is exact."""
    d = np.float32(d)
    recip = np.float32(1) / d
    c = ((np.arange(0, 4096, dtype=np.float32) + np.float32(0.5)) * d).astype(np.float32)
    cand = np.concatenate([c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(0))])
    ys = cand[np.rint((cand / d).astype(np.float32)) != np.rint((cand * recip).astype(np.float32))][:count]
    near = [(TABLE * d).astype(np.float32)]
    for towards in (np.inf, 0):
        t = near[0]
        for _ in range(3):
            t = np.nextafter(t, np.float32(towards))
            near.append(t)
    cs = np.concatenate(near)
    cs = cs[cs > 0.111]
    ss = cs[QX.index_rule((cs / d).astype(np.float32), TABLE) != QX.index_rule((cs * recip).astype(np.float32), TABLE)][:count]
    return ys, ss


def _planted(per, steps):
    """Per image the values the issue names, as (y, scale) pairs for the image's step d; at most 64 of them."""
    t = TABLE
    out = []
    for d in np.asarray(steps, dtype=np.float32):
        pairs = [(0.75, 1.0), (1.25, 1.0), (4.5, 1.0), (-4.5, 1.0), (-0.25, 1.0), (0.25 * d, 1.0), (-0.5 * d, 2.0), (1.5 * d, 2.0), (2.5 * d, 2.0)]
        for j in (0, 1, 17, 40, 62, 63):                      # scale = table[j] * d and its neighbours: '<' against '<='
            on = np.float32(t[j] * d)
            pairs += [(1.0, on), (1.0, np.nextafter(on, np.float32(np.inf))), (1.0, np.nextafter(on, np.float32(0)))]
        pairs += [(3.0, 0.05), (3.0, 0.0), (3.0, -1.0), (3.0, 0.10999), (3.0, np.float32(BOUND))]                 # below the bound
        pairs += [(3.0, t[63] * d * 2), (3.0, 1e30), (3.0, np.inf)]                                              # past the table
        pairs += [(3.0, np.nan), (-2.5, np.nan)]
        ys, ss = _deciders(d)
        pairs += [(v, 1.0) for v in ys] + [(1.0, v) for v in ss]       # (appended: the positions above stay where they are)
        assert len(pairs) <= 64
        out.append(np.asarray(pairs, dtype=np.float32))
    return out


def _inputs(B, per, steps, seed):
    rng = np.random.default_rng(seed)
    n = B * per
    y = np.where(rng.random(n) < 0.3, rng.integers(-60, 61, n) / 4.0, rng.normal(size=n) * 9).astype(np.float32)
    s = np.exp(rng.uniform(math.log(0.03), math.log(2000), n)).astype(np.float32)
    per_img = steps if len(steps) == B else list(steps) * B
    for b, pairs in enumerate(_planted(per, per_img) if per >= 128 else []):      # (images of a few elements hold random values only)
        # at the image's start and at its end: both sides of every image boundary carry planted values
        y[b * per: b * per + len(pairs)], s[b * per: b * per + len(pairs)] = pairs[:, 0], pairs[:, 1]
        y[(b + 1) * per - len(pairs): (b + 1) * per], s[(b + 1) * per - len(pairs): (b + 1) * per] = pairs[::-1, 0], pairs[::-1, 1]
    return y, s


def _run_q(y, s, per, steps, want_yhat=True):
    """The three entry points on sentinel-guarded buffers -> sym, idx, yhat bits, decoder's yhat bits (host int32 arrays)."""
    _lib, L = _L()
    n = y.size
    d_y, d_s, d_t = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(TABLE).cuda()
    d_steps = torch.tensor(np.asarray(steps, dtype=np.float32), device="cuda")
    (bs, sym), (bi, idx), (by, yh), (bd, dq) = _guarded(n), _guarded(n), _guarded(n), _guarded(n)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.basic_gc_quantize_index_q_dev(d_y.data_ptr(), d_s.data_ptr(), n, per, d_steps.data_ptr(), d_steps.numel(), d_t.data_ptr(),
                                               len(TABLE), BOUND, sym.data_ptr(), idx.data_ptr(), yh.data_ptr() if want_yhat else None, st))
    _lib.check(L.basic_gc_dequantize_q_dev(sym.data_ptr(), n, per, d_steps.data_ptr(), d_steps.numel(), dq.data_ptr(), st))
    torch.cuda.synchronize()
    for name, buf in (("symbols", bs), ("indexes", bi), ("yhat", by), ("dequantised", bd)):
        assert _intact(buf, n), f"the launch wrote outside {name}"
    return tuple(t.cpu().numpy() for t in (sym, idx, yh, dq))


CASES = [("boundary inside a workgroup", 3, 8 * 5 * 7, (0.5, 1.0, 3.0)),
         ("past the grid cap", 3, 192 * 32 * 32, (0.7, 1.0, 64.0)),
         ("boundary inside the second stride", 3, 262_147, (0.7, 0.0625, 3.0)),
         ("broadcast, small", 3, 8 * 5 * 7, (3.0,)), ("broadcast, past the grid cap", 3, 192 * 32 * 32, (0.7,)),
         ("images shorter than a wavefront", 40, 24, tuple(0.25 + 0.35 * i for i in range(40)))]


@pytest.mark.parametrize("name,B,per,steps", CASES, ids=[c[0] for c in CASES])
def test_quantize_index_q_is_the_restatement(name, B, per, steps):
    n = B * per
    if "past" in name:
        assert n == 589_824 > ONE_PASS
    if "second stride" in name:
        assert ONE_PASS < 2 * per < ONE_PASS + 256 and (2 * per) % 256      # the boundary lies inside the first workgroup of the second stride
    y, s = _inputs(B, per, steps, seed=n + len(steps))
    want_sym, want_idx, want_yhat = QX.quantize_index_q(y, s, steps, per, TABLE, BOUND)
    sym, idx, yh, dq = _run_q(y, s, per, steps)
    bad = [int((sym != want_sym).sum()), int((idx != want_idx).sum()), int((yh != want_yhat.view(np.int32)).sum())]
    print(f"{name}: n = {n}, differing symbols {bad[0]}, indexes {bad[1]}, yhat bits {bad[2]}")
    assert bad == [0, 0, 0]
    assert QX.same_reconstruction(dq.view(np.float32), want_yhat, want_sym)
    assert np.array_equal(dq.view(np.float32), QX.dequantize_q(want_sym, steps, per))
    # what the data held: the division's rounding decided somewhere (a reciprocal multiply gives another symbol or index), ties went
    # to even, every table row and both ends of the table were met, NaN scales took the bound's index
    if per < 128:
        return
    d = QX.steps_per_element(steps, B, per)
    sb = np.fmax(s, np.float32(BOUND))
    recip = (np.float32(1) / d).astype(np.float32)
    for v in set(float(v) for v in steps) - {0.0625, 0.5, 1.0, 64.0}:      # 0.7, 3: not powers of two
        at = d == np.float32(v)
        with np.errstate(invalid="ignore"):
            assert (np.rint((y * recip).astype(np.float32)) != np.rint((y / d).astype(np.float32)))[at].any(), v
        assert (QX.index_rule((sb * recip).astype(np.float32), TABLE) != want_idx)[at].any(), v
    assert 63 in want_idx and len(set(want_idx.tolist())) >= 48      # (row 0 is out of reach of a step below 1: the bound comes first)
    assert (want_idx[np.isnan(s)] == QX.index_rule(np.float32(BOUND) / d[np.isnan(s)], TABLE)).all() and np.isnan(s).any()
    # the decoder's use: y := scales, no yhat -- the same indexes, and nothing written to a yhat that is not there
    _, idx2, yh2, _ = _run_q(s, s, per, steps, want_yhat=False)
    assert np.array_equal(idx2, want_idx) and (yh2 == FRESH).all()


def test_planted_values_read_as_the_issue_states_them():
    """B = 3, per_image = 280, steps (0.5, 1, 3): the ties and the table edges by hand, not by the restatement."""
    per, steps = 280, (0.5, 1.0, 3.0)
    y, s = _inputs(3, per, steps, seed=1)
    sym, idx, yh, dq = _run_q(y, s, per, steps)
    yh = yh.view(np.float32)
    assert sym[0:2].tolist() == [2, 2] and yh[0:2].tolist() == [1.0, 1.0]                  # 0.75 / 0.5 = 1.5 -> 2, 1.25 / 0.5 = 2.5 -> 2
    assert sym[2 * per + 2: 2 * per + 4].tolist() == [2, -2] and yh[2 * per + 2: 2 * per + 4].tolist() == [6.0, -6.0]   # +/-4.5 / 3 = +/-1.5
    assert sym[per + 2: per + 4].tolist() == [4, -4]                                       # +/-4.5 at step 1: half to even
    for b in range(3):
        base = b * per + 9
        for k, j in enumerate((0, 1, 17, 40, 62, 63)):
            on, above, below = idx[base + 3 * k: base + 3 * k + 3].tolist()
            if steps[b] in (0.5, 1.0) and TABLE[j] * steps[b] > 0.111:       # a power of two: table[j] * step / step is table[j] again (above the bound)
                assert on == j and above == min(j + 1, 63) and below == (j if j else 0), (b, j)
        low = idx[base + 18: base + 23].tolist()
        assert len(set(low)) == 1 and low[0] == QX.index_rule(np.float32(BOUND) / np.float32([steps[b]]), TABLE)[0]   # the bound first, then the step
        assert idx[base + 23: base + 26].tolist() == [63, 63, 63]


def test_step_one_is_todays_kernels_bit_for_bit():
    _lib, L = _L()
    for B, per, steps in ((3, 280, (1.0, 1.0, 1.0)), (3, 280, (1.0,)), (3, 192 * 32 * 32, (1.0,)), (3, 262_147, (1.0, 1.0, 1.0))):
        y, s = _inputs(B, per, [1.0] * B, seed=7 + per)
        n = y.size
        sym, idx, yh, dq = _run_q(y, s, per, steps)
        d_y, d_s, d_t = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(TABLE).cuda()
        (b0, sym0), (b1, idx0), (b2, yh0), (b3, f0) = _guarded(n), _guarded(n), _guarded(n), _guarded(n)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.basic_gc_quantize_index_dev(d_y.data_ptr(), d_s.data_ptr(), n, d_t.data_ptr(), len(TABLE), BOUND, sym0.data_ptr(), idx0.data_ptr(),
                                                 yh0.data_ptr(), st))
        _lib.check(L.basic_i32_to_f32_dev(sym0.data_ptr(), n, f0.data_ptr(), st))
        torch.cuda.synchronize()
        assert np.array_equal(sym, sym0.cpu().numpy()) and np.array_equal(idx, idx0.cpu().numpy())
        assert np.array_equal(yh, yh0.cpu().numpy()) and np.array_equal(dq, f0.cpu().numpy())      # int32 views: bits
        assert (yh.view(np.float32)[sym == 0] == 0).all() and np.signbit(yh.view(np.float32)[sym == 0]).any()


def test_entry_points_refuse_bad_shapes():
    _lib, L = _L()
    a = torch.zeros(560, device="cuda")
    i = torch.zeros(560, dtype=torch.int32, device="cuda")
    j = torch.zeros_like(i)
    t = torch.from_numpy(TABLE).cuda()
    steps = torch.ones(3, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()
    for n, per, ns in ((560, 280, 3), (560, 280, 0), (560, 300, 1), (560, 0, 1), (560, -280, 2), (560, 560, 2)):
        with pytest.raises(ValueError):
            _lib.check(L.basic_gc_quantize_index_q_dev(P(a), P(a), n, per, P(steps), ns, P(t), 64, BOUND, P(i), P(j), None, st))
        with pytest.raises(ValueError):
            _lib.check(L.basic_gc_dequantize_q_dev(P(i), n, per, P(steps), ns, P(a), st))
    with pytest.raises(ValueError):
        _lib.check(L.basic_gc_quantize_index_q_dev(P(a), P(a), 560, 280, None, 1, P(t), 64, BOUND, P(i), P(j), None, st))
    out = torch.zeros(2, device="cuda")
    for ns in (0, 3):
        with pytest.raises(ValueError):
            _lib.check(L.basic_gauss_nll_per_image_q_dev(P(a), P(a), 2, 7, 40, P(steps), ns, BOUND, 1e-9, P(out), st))
    # the Python front-ends validate the steps on the host, before any launch
    from cbench_basic_amd.nn import kernels as K
    y = a.reshape(2, 7, 40)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -5, 65.0, [1.0, 2.0, 3.0], []):
        with pytest.raises(ValueError):
            K.gc_quantize_index_q(y, y, bad, t)
        with pytest.raises(ValueError):
            K.gc_dequantize_q(i.reshape(2, 7, 40), bad)
        with pytest.raises(ValueError):
            K.gauss_nll_per_image(y, y, False, steps=bad)
    sym, idx, yhat = K.gc_quantize_index_q(y + 3, y + 2, [0.5, 4.0], t)
    assert sym[0].unique().tolist() == [6] and sym[1].unique().tolist() == [1] and torch.equal(K.gc_dequantize_q(sym, [0.5, 4.0]), yhat)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the rate estimate under a step
@pytest.mark.parametrize("steps", [(0.5, 0.7, 3.0), (0.7,), (1.0,)], ids=["per-image", "broadcast", "one"])
@pytest.mark.parametrize("B,C,hw", [(3, 5, 21), (3, 7, 300)])
def test_gauss_nll_q_vs_fp64(B, C, hw, steps):
    """The tolerance of tests/test_gpu_entropy_kernels.py for gauss_nll_per_image (_check_rate: 4 x the formula's own fp32 error + the
    summation bound, below 1e-4 of the value), on its body inputs: s log-uniform in [0.05, 8], integer symbols with |q| <= 2.5 s'."""
    from test_gpu_entropy_kernels import LIK_BOUND, SCALE_BOUND, _check_rate
    from cbench_basic_amd.nn import kernels as K
    g = torch.Generator().manual_seed(hw + len(steps))
    s = torch.exp(torch.rand(B, C, hw, generator=g) * (math.log(8) - math.log(0.05)) + math.log(0.05))
    d = torch.from_numpy(QX.steps_per_element(steps, B, C * hw).copy()).reshape(B, C, hw)
    sq = torch.clamp(s, min=SCALE_BOUND) / d
    q = torch.trunc((torch.rand(B, C, hw, generator=g) * 2 - 1) * 2.5 * sq)
    got = K.gauss_nll_per_image(q.cuda(), s.cuda(), False, SCALE_BOUND, LIK_BOUND, steps=list(steps))
    t32 = QX.nll_terms_q(q.numpy(), s.numpy(), steps, SCALE_BOUND, LIK_BOUND, torch.float32)
    t64 = QX.nll_terms_q(q.numpy(), s.numpy(), steps, SCALE_BOUND, LIK_BOUND, torch.float64)
    mutants = {"one position on": QX.nll_terms_q(q.numpy(), torch.roll(s, 1, dims=2).numpy(), steps, SCALE_BOUND, LIK_BOUND, torch.float64)}
    if any(v != 1.0 for v in steps):
        mutants["the step forgotten"] = QX.nll_terms_q(q.numpy(), s.numpy(), (1.0,), SCALE_BOUND, LIK_BOUND, torch.float64)
        if len(steps) > 1:
            mutants["every image with its neighbour's step"] = QX.nll_terms_q(q.numpy(), s.numpy(), steps[1:] + steps[:1], SCALE_BOUND, LIK_BOUND,
                                                                               torch.float64)
    _check_rate(f"gauss_nll_q ({B}, {C}, {hw}) steps {steps}", got, t32, t64, mutants)
