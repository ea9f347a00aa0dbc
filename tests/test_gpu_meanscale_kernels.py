"""The mean-scale kernels of csrc/entropy.hip on the GPU (INTEGRATION.md "Mean-scale hyperprior"): basic_gc_quantize_index_ms_dev,
basic_gc_dequantize_ms_dev and basic_gc_rate_curve_ms_dev equal the NumPy restatement (tests/meanscale_exact.py) exactly -- int32
symbols and indexes, the BITS of yhat, integer bit sums.  No tolerance, and never another kernel as the reference (the one
exception is the premise the format states: with mu = +0.0 the _ms entry points reproduce the zero-mean entry points).

Shapes (B, per_image): one thread's worth (1, 7); several image boundaries inside one 256-element chunk (3, 100); a boundary on a
chunk boundary (2, 256) and one past it (3, 257); many chunks (5, 3072); and (3, 184512) = 553,536 elements, past the 524,288 the
grid covers in one stride.  Each in both layouts: the chunked prior read in place (param_stride = 2 per_image, and once a wider
stride), and two separate arrays.  Before anything is compared each test asserts that its data would catch the likely mistakes."""
import ctypes

import numpy as np
import pytest
import torch

import meanscale_exact as MX
import qstep_exact as QX
import rate_exact as RX

pytestmark = pytest.mark.gpu

TIES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.25, -0.75, 1.25, 4.5, -7.5, 10.5]   # of y - mu: ties at step 1 (and none), 0.5 and 3


@pytest.fixture(scope="module")
def gc():
    from cbench_basic_amd.modules.prior_model.prior_coder.compressai_coder import CompressAIMeanScaleGaussianConditionalCoder
    from cbench_basic_amd.nn import kernels as K
    c = CompressAIMeanScaleGaussianConditionalCoder().eval().cuda()
    c.update_state()
    c._ready()
    cdf, sizes, offsets = c._cdf_host
    return dict(tables=c._tables, sizes=sizes, offsets=offsets, scale_table=c.scale_table.cpu().numpy(), table_dev=c._scale_table_dev,
                bound=c.scale_bound, costs=K.rans_tables_costs(c._tables))


def _inputs(B, per, seed):
    """y ~ N(0, 2), mu uniform in [-3, 3), scales log-uniform over [0.05, 300] (below the bound, across the whole table); planted per
    image, where it has room: mu = +0.0 and -0.0 under a symbol 0, the absorbing mean 1000.3, a NaN scale, ties of y - mu."""
    rng = np.random.default_rng(seed)
    y = rng.normal(0.0, 2.0, (B, per)).astype(np.float32)
    mu = rng.uniform(-3.0, 3.0, (B, per)).astype(np.float32)
    scales = np.exp(rng.uniform(np.log(0.05), np.log(300.0), (B, per))).astype(np.float32)
    for b in range(B):
        o = (b * 3) % max(1, per - 16) if per > 16 else 0   # another place in every image
        mu[b, o], y[b, o] = 0.0, -0.2
        mu[b, o + 1], y[b, o + 1] = -0.0, -0.2
        mu[b, o + 2] = 1000.3
        y[b, o + 2] = mu[b, o + 2] + np.float32(1.2)
        scales[b, o + 3] = np.nan
        for j, t in enumerate(TIES[:max(0, per - 4 - o)]):
            m = np.float32(0.25 * ((j + b) % 9 - 4))     # dyadic: mu + tie is exact, so y - mu is the tie again
            mu[b, o + 4 + j], y[b, o + 4 + j] = m, np.float32(m + np.float32(t))
    return y, scales, mu


def _steps_options(B):
    per_image = [0.5, 1.0, 3.0, 2.0 ** -4, 2.0 ** 6][:B]
    return [None, [1.0], per_image, [2.0 ** -4], [2.0 ** 6]]


def _differs(a, b):
    return any(not np.array_equal(np.asarray(p).view(np.int32), np.asarray(q).view(np.int32)) for p, q in zip(a, b))


def _mutant_guard(y, scales, mu, steps, per, tab, bound, want):
    """The restatement answers differently when the means are forgotten, taken from the neighbouring image, swapped with the scales,
    or subtracted after the step: data that could not tell would prove nothing."""
    B = y.size // per
    flat = lambda a: a.reshape(-1)
    assert _differs(MX.quantize_index_ms(flat(y), flat(scales), np.zeros(y.size, np.float32), steps, per, tab, bound), want), "means forgotten"
    if B > 1:
        assert _differs(MX.quantize_index_ms(flat(y), flat(scales), flat(np.roll(mu, 1, axis=0)), steps, per, tab, bound), want), "neighbour's means"
    with np.errstate(invalid="ignore"):   # the NaN scale becomes a NaN mean here
        assert _differs(MX.quantize_index_ms(flat(y), flat(mu), flat(scales), steps, per, tab, bound), want), "halves swapped"
    if steps is not None and any(s != 1.0 for s in steps):
        d = QX.steps_per_element(steps, B, per)
        q = np.rint(((flat(y) / d).astype(np.float32) - flat(mu)).astype(np.float32))
        assert not np.array_equal(q.astype(np.int32), want[0]), "step before the subtraction"


def _device_params(scales, mu, layout):
    """-> the (prior, means) arguments of the nn.kernels wrappers for a layout."""
    B, per = scales.shape
    if layout == "separate":
        return torch.from_numpy(scales).cuda(), torch.from_numpy(mu).cuda()
    if layout == "chunked":
        return torch.from_numpy(np.concatenate([scales, mu], axis=1)).cuda(), None
    wide = torch.full((B, 2 * per + 3), float("nan")).cuda()     # "wide": param_stride = 2 per + 3, a view into a larger tensor
    wide[:, :2 * per] = torch.from_numpy(np.concatenate([scales, mu], axis=1)).cuda()
    return wide[:, :2 * per], None


SHAPES = [(1, 7), (3, 100), (2, 256), (3, 257), (5, 3072), (3, 184512)]


@pytest.mark.parametrize("layout", ["chunked", "separate"])
@pytest.mark.parametrize("B,per", SHAPES)
def test_quantize_index_and_dequantize_are_exact(gc, B, per, layout):
    from cbench_basic_amd.nn import kernels as K
    y, scales, mu = _inputs(B, per, seed=B * 1000 + per)
    yd = torch.from_numpy(y).cuda()
    prior, means = _device_params(scales, mu, layout)
    tab, bound = gc["scale_table"], gc["bound"]
    for steps in _steps_options(B):
        want = MX.quantize_index_ms(y, scales, mu, steps, per, tab, bound)
        _mutant_guard(y, scales, mu, steps, per, tab, bound, want)
        sym, idx, yhat = K.gc_quantize_index_ms(yd, prior, gc["table_dev"], bound, steps=steps, means=means)
        assert sym.shape == yd.shape and sym.dtype == torch.int32 and yhat.dtype == torch.float32
        got = [t.cpu().numpy().reshape(-1) for t in (sym, idx, yhat)]
        assert np.array_equal(got[0], want[0]), steps
        assert np.array_equal(got[1], want[1]), steps
        assert np.array_equal(got[2].view(np.int32), want[2].view(np.int32)), steps
        # indexes only (the decoder's call): the same indexes, nothing else written
        s0, i0, y0 = K.gc_quantize_index_ms(None, prior, gc["table_dev"], bound, steps=steps, means=means)
        assert s0 is None and y0 is None and np.array_equal(i0.cpu().numpy().reshape(-1), want[1])
        # without yhat
        s1, i1, y1 = K.gc_quantize_index_ms(yd, prior, gc["table_dev"], bound, steps=steps, means=means, want_yhat=False)
        assert y1 is None and torch.equal(s1, sym) and torch.equal(i1, idx)
        # the decoder
        dec = K.gc_dequantize_ms(sym, prior, steps=steps, means=means).cpu().numpy().reshape(-1)
        assert np.array_equal(dec.view(np.int32), MX.dequantize_ms(want[0], mu, steps, per).view(np.int32)), steps
        assert MX.same_reconstruction(dec, got[2], got[0], mu)
    # the planted cases are in the data
    sym = MX.quantize_index_ms(y, scales, mu, None, per, tab, bound)[0].reshape(B, per)
    assert (sym[(mu == 0) & np.signbit(mu)] == 0).any() and (sym[(mu == 0) & ~np.signbit(mu)] == 0).any()
    assert np.isnan(scales).sum() == B and (mu == np.float32(1000.3)).sum() == B
    if B * per >= 300:   # log-uniform over [0.05, 300]: one scale in eleven lies under the bound
        assert (scales < bound).any() and (scales > 200).any()


def test_a_wider_param_stride_reads_the_same_elements(gc):
    from cbench_basic_amd.nn import kernels as K
    B, per = 3, 257
    y, scales, mu = _inputs(B, per, seed=9)
    prior, _ = _device_params(scales, mu, "wide")
    assert prior.stride(0) == 2 * per + 3 and not prior.is_contiguous()
    for steps in (None, [0.5, 1.0, 3.0]):
        want = MX.quantize_index_ms(y, scales, mu, steps, per, gc["scale_table"], gc["bound"])
        _mutant_guard(y, scales, mu, steps, per, gc["scale_table"], gc["bound"], want)
        sym, idx, yhat = K.gc_quantize_index_ms(torch.from_numpy(y).cuda(), prior, gc["table_dev"], gc["bound"], steps=steps)
        assert np.array_equal(sym.cpu().numpy().reshape(-1), want[0]) and np.array_equal(idx.cpu().numpy().reshape(-1), want[1])
        assert np.array_equal(yhat.cpu().numpy().reshape(-1).view(np.int32), want[2].view(np.int32))
        dec = K.gc_dequantize_ms(sym, prior, steps=steps).cpu().numpy().reshape(-1)
        assert np.array_equal(dec.view(np.int32), MX.dequantize_ms(want[0], mu, steps, per).view(np.int32))
        bits = K.rate_curve(torch.from_numpy(y).cuda(), prior, torch.tensor([1.0, 2.0]).cuda(), gc["table_dev"], gc["tables"], gc["bound"], 1,
                            means=K.CHUNKED)
        assert np.array_equal(bits.cpu().numpy(), MX.rate_curve_ms(y, scales, mu, B, per, 1, np.array([1.0, 2.0], np.float32), gc["scale_table"],
                                                                   gc["bound"], gc["costs"], gc["sizes"], gc["offsets"], 4))
    # a layout whose image is not contiguous is refused on the host
    with pytest.raises(ValueError):
        K.gc_quantize_index_ms(torch.from_numpy(y).cuda(), torch.zeros(B, 4 * per).cuda()[:, ::2], gc["table_dev"], gc["bound"])
    with pytest.raises(ValueError):
        K.gc_quantize_index_ms(torch.from_numpy(y).cuda(), torch.zeros(B, per).cuda(), gc["table_dev"], gc["bound"])


# ---------------------------------------------------------------- rate curve
@pytest.mark.parametrize("layout", ["chunked", "separate"])
@pytest.mark.parametrize("lanes,K_,cpi", [(1, 2, 0), (4, 3, 1), (1, 8, 1), (4, 9, 0), (1, 16, 0), (4, 17, 1), (4, 32, 0), (1, 32, 1)])
def test_rate_curve_ms_is_exact(gc, lanes, K_, cpi, layout):
    """n_cand on both sides of every kNC instantiation (2 | 3 .. 8 | 9 .. 16 | 17 .. 32), one and four segments an image, shared and
    per-image candidates; per_seg = 1285 or 5140 elements: more than one workgroup per segment, none a multiple of the block."""
    from cbench_basic_amd.nn import kernels as K
    B, per_seg = 3, (5140 if lanes == 1 else 1285)
    per = lanes * per_seg
    y, scales, mu = _inputs(B, per, seed=lanes * 100 + K_)
    rng = np.random.default_rng(K_)
    cand = rng.uniform(0.0625, 64.0, (B, K_) if cpi else (K_,)).astype(np.float32)
    cand.reshape(-1)[:2] = [1.0, 0.5]
    want = MX.rate_curve_ms(y, scales, mu, B * lanes, per_seg, lanes, cand, gc["scale_table"], gc["bound"], gc["costs"], gc["sizes"],
                            gc["offsets"], 4)
    # the data tells the mistakes apart in the sums too
    zero = np.zeros_like(mu)
    with np.errstate(invalid="ignore"):   # swapped halves: the NaN scale becomes a NaN mean
        for wrong in ((scales, zero), (scales, np.roll(mu, 1, axis=0)), (mu, scales)):
            assert not np.array_equal(want, MX.rate_curve_ms(y, wrong[0], wrong[1], B * lanes, per_seg, lanes, cand, gc["scale_table"],
                                                             gc["bound"], gc["costs"], gc["sizes"], gc["offsets"], 4))
    prior, means = _device_params(scales, mu, layout)
    yd, cd = torch.from_numpy(y).cuda(), torch.from_numpy(cand).cuda()
    bits = K.rate_curve(yd, prior, cd, gc["table_dev"], gc["tables"], gc["bound"], lanes, means=K.CHUNKED if means is None else means)
    again = K.rate_curve(yd, prior, cd, gc["table_dev"], gc["tables"], gc["bound"], lanes, means=K.CHUNKED if means is None else means)
    assert bits.shape == (B * lanes, K_) and bits.dtype == torch.int64 and torch.equal(bits, again)
    assert np.array_equal(bits.cpu().numpy(), want)


def test_rate_steps_with_means_follow_the_restatement(gc):
    """curve -> select -> refine -> curve -> select with means=: every pass's curve is the restatement's at that pass's candidates."""
    from cbench_basic_amd.nn import kernels as K
    B, lanes, per_seg, K_ = 3, 2, 257, 8
    y, scales, mu = _inputs(B, lanes * per_seg, seed=21)
    prior, _ = _device_params(scales, mu, "chunked")
    budgets = torch.tensor([900, 1 << 40, 1], dtype=torch.int64).cuda()
    steps, choice, pred, trace = K.rate_steps(torch.from_numpy(y).cuda(), prior, budgets, None, RX.first_grid(K_), 2, gc["table_dev"],
                                              gc["tables"], gc["bound"], lanes, return_trace=True, means=K.CHUNKED)
    assert len(trace) == 2
    for cand, bits, _ in trace:
        assert np.array_equal(bits.cpu().numpy(), MX.rate_curve_ms(y, scales, mu, B * lanes, per_seg, lanes, cand.cpu().numpy(), gc["scale_table"],
                                                                   gc["bound"], gc["costs"], gc["sizes"], gc["offsets"], 4))
    ws, wc, wp = RX.select(trace[-1][1].cpu().numpy(), lanes, per_seg, trace[-1][0].cpu().numpy(), budgets.cpu().numpy(), None)
    assert np.array_equal(choice.cpu().numpy(), wc) and np.array_equal(pred.cpu().numpy(), wp)
    assert np.array_equal(steps.cpu().numpy().view(np.int32), ws.view(np.int32))
    assert wc[2] & RX.NO_FIT and not wc[1] & RX.NO_FIT


# ---------------------------------------------------------------- the premise: mu = +0.0 is the zero-mean coder
def test_zero_means_reproduce_the_zero_mean_entry_points(gc):
    from cbench_basic_amd.nn import kernels as K
    B, per = 3, 3073
    y, scales, _ = _inputs(B, per, seed=4)
    yd, sd, zd = torch.from_numpy(y).cuda(), torch.from_numpy(scales).cuda(), torch.zeros(B, per).cuda()
    sym, idx, yhat = K.gc_quantize_index_ms(yd, sd, gc["table_dev"], gc["bound"], means=zd)
    rs, ri, ry = K.gc_quantize_index(yd, sd, gc["table_dev"], gc["bound"])
    assert torch.equal(sym, rs) and torch.equal(idx, ri) and torch.equal(yhat, ry)            # values: -0.0 == +0.0
    for steps in ([1.0], [0.5, 1.0, 3.0]):
        sym, idx, yhat = K.gc_quantize_index_ms(yd, sd, gc["table_dev"], gc["bound"], steps=steps, means=zd)
        rs, ri, ry = K.gc_quantize_index_q(yd, sd, steps, gc["table_dev"], gc["bound"])
        assert torch.equal(sym, rs) and torch.equal(idx, ri) and torch.equal(yhat, ry)
    for lanes, K_ in ((1, 2), (1, 16), (7, 5)):       # 3073 = 7 * 439
        cand = torch.from_numpy(RX.first_grid(K_)).cuda()
        a = K.rate_curve(yd, sd, cand, gc["table_dev"], gc["tables"], gc["bound"], lanes, means=zd)
        b = K.rate_curve(yd, sd, cand, gc["table_dev"], gc["tables"], gc["bound"], lanes)
        assert torch.equal(a, b) and int(a.min()) > 0


# ---------------------------------------------------------------- refusals: BASIC_ERR_INVALID before any launch
def test_entry_points_refuse_without_a_launch(gc):
    from cbench_basic_amd import _lib
    L = _lib.lib()
    B, per = 3, 10
    n = B * per
    y, prior = torch.zeros(n).cuda(), torch.ones(2 * n).cuda()
    steps = torch.ones(3).cuda()
    sym = torch.full((n,), -77, dtype=torch.int32).cuda()
    idx = torch.full((n,), -77, dtype=torch.int32).cuda()
    yhat = torch.full((n,), -77.0).cuda()
    bits = torch.full((B, 2), -77, dtype=torch.int64).cuda()
    cand = torch.ones(2).cuda()
    tab, tl, bound = gc["table_dev"].data_ptr(), gc["table_dev"].numel(), ctypes.c_float(gc["bound"])
    p = lambda t: t.data_ptr()
    mu = p(prior) + 4 * per

    def quant(d_y=p(y), n_=n, per_=per, stride=2 * per, d_steps=p(steps), n_steps=3, d_sym=p(sym), d_yhat=p(yhat), d_means=mu):
        return L.basic_gc_quantize_index_ms_dev(d_y, p(prior), d_means, n_, per_, stride, d_steps, n_steps, tab, tl, bound, d_sym, p(idx), d_yhat, None)

    def dequant(n_=n, per_=per, stride=2 * per, n_steps=3):
        return L.basic_gc_dequantize_ms_dev(p(sym), mu, n_, per_, stride, p(steps), n_steps, p(yhat), None)

    def curve(stride=2 * per, d_means=mu):
        return L.basic_gc_rate_curve_ms_dev(p(y), p(prior), d_means, stride, B, per, 1, p(cand), 2, 0, tab, tl, bound, gc["tables"]._h, p(bits), None)

    refused = [quant(n_=n - 1), quant(per_=7), quant(n_steps=2), quant(stride=per - 1), quant(d_sym=None), quant(d_sym=None, d_yhat=None),
               quant(d_means=None), quant(d_y=None), quant(d_y=None, d_yhat=None), dequant(n_=n - 1), dequant(n_steps=2),
               dequant(stride=per - 1), curve(stride=per - 1), curve(d_means=None)]
    assert refused == [_lib.ERR_INVALID] * len(refused)
    torch.cuda.synchronize()
    for t in (sym, idx, bits):
        assert bool((t == -77).all())
    assert bool((yhat == -77.0).all())
    # and the same calls, well-formed, run (n_steps 0, 1 and B; a NULL d_steps means no step whatever n_steps says)
    for kw in (dict(), dict(n_steps=1), dict(n_steps=0), dict(d_steps=None, n_steps=3), dict(d_y=None, d_sym=None, d_yhat=None, d_means=None)):
        assert quant(**kw) == _lib.OK
    assert dequant() == _lib.OK and dequant(n_steps=0) == _lib.OK and curve() == _lib.OK
    torch.cuda.synchronize()
    assert bool((idx != -77).all()) and bool((bits != -77).all())
