"""The rate kernels of csrc/entropy.hip on the GPU (INTEGRATION.md "Rate control"): every entry of basic_gc_rate_curve_dev equals the
NumPy restatement (tests/rate_exact.py, on the library's own cost table read back) AND the cost of the symbols and indexes that
basic_gc_quantize_index_q_dev -- an independent kernel -- writes at that step; two calls agree bit for bit; select and refine equal
their restatements; the entry points refuse what they say they refuse.

Shapes: every per_seg of {1, 63, 64, 65, 257, 4097} (one thread, around a wavefront, more than one workgroup's stride, more than one
workgroup per segment), B of {1, 3}, segs_per_image of {1, 2, 4}, n_cand of {1, 2, 5, 32} (every instantiation of the kernel, with
live and dead accumulators), both candidate layouts -- a covering set of 14 of the 288 combinations, every value at least twice."""
import numpy as np
import pytest
import torch

import qstep_exact as QX
import rate_exact as RX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gc():
    from cbench_basic_amd.modules.prior_model.prior_coder.compressai_coder import CompressAIGaussianConditionalCoder
    from cbench_basic_amd.nn import kernels as K
    c = CompressAIGaussianConditionalCoder().eval().cuda()
    c.update_state()
    c._ready()
    cdf, sizes, offsets = c._cdf_host
    return dict(coder=c, tables=c._tables, cdf=cdf, sizes=sizes, offsets=offsets, scale_table=c.scale_table.cpu().numpy(),
                table_dev=c._scale_table_dev, bound=c.scale_bound, costs=K.rans_tables_costs(c._tables))


def test_the_tables_cost_table_is_the_host_functions(gc):
    from cbench_basic_amd.nn import kernels as K
    assert gc["costs"].shape == gc["cdf"].shape
    assert np.array_equal(gc["costs"], K.rans_cost_table(gc["cdf"], gc["sizes"], 16))
    assert np.abs(gc["costs"].astype(np.int64) - RX.cost_table(gc["cdf"], gc["sizes"]).astype(np.int64)).max() <= 1


def _inputs(gc, B, lanes, per_seg, cand, seed):
    """y, sigma float32 [B][lanes * per_seg] with the edge cases planted where the shape has room for them."""
    rng = np.random.default_rng(seed)
    n = lanes * per_seg
    sigma = np.exp(rng.uniform(np.log(0.03), np.log(300.0), (B, n))).astype(np.float32)      # below the bound (0.11) too
    y = (rng.standard_normal((B, n)).astype(np.float32) * sigma * np.where(rng.random((B, n)) < 0.2, 6.0, 1.0)).astype(np.float32)
    dmin = float(np.min(cand))
    plant = [("nan_sigma", None), ("at_max", None), ("big+", np.float32(2.0 ** 30 * dmin)), ("big-", np.float32(-(2.0 ** 30) * dmin))]
    for b in range(B):
        for j, (what, v) in enumerate(plant):
            pos = (j * 37 + b) % n if n > 4 else None
            if pos is None:
                continue
            if what == "nan_sigma":
                sigma[b, pos] = np.nan
            elif what == "at_max":      # sigma under the bound, at the first candidate: value == max  <=>  sym = size - 2 + offset of its row
                c0 = np.float32(np.asarray(cand).reshape(-1)[0])
                row = int(QX.index_rule(np.array([np.float32(gc["bound"]) / c0], np.float32), gc["scale_table"])[0])
                sigma[b, pos] = 0.05
                y[b, pos] = np.float32(int(gc["sizes"][row]) - 2 + int(gc["offsets"][row])) * c0
            else:
                y[b, pos] = v
    return y, sigma


CASES = [  # (B, segs_per_image, per_seg, n_cand, cand_per_image)
    (1, 1, 1, 1, 0), (3, 2, 1, 2, 1), (1, 4, 63, 5, 0), (3, 1, 63, 32, 1), (1, 2, 64, 2, 1), (3, 4, 64, 1, 0), (1, 1, 65, 32, 0),
    (3, 2, 65, 5, 1), (1, 4, 257, 32, 1), (3, 1, 257, 2, 0), (1, 2, 4097, 5, 1), (3, 4, 4097, 32, 0), (3, 1, 4097, 1, 1), (1, 1, 4097, 16, 0)]


@pytest.mark.parametrize("B,lanes,per_seg,K_,cpi", CASES)
def test_rate_curve_is_exact(gc, B, lanes, per_seg, K_, cpi):
    from cbench_basic_amd.nn import kernels as K
    rng = np.random.default_rng(B * 1000 + lanes * 100 + per_seg + K_)
    cand = rng.uniform(0.0625, 64.0, (B, K_) if cpi else (K_,)).astype(np.float32)
    cand.reshape(-1)[0] = 1.0
    if K_ >= 5:
        cand.reshape(-1)[1:4] = [0.0625, 64.0, 0.7]
    y, sigma = _inputs(gc, B, lanes, per_seg, cand, seed=per_seg + K_)
    yd, sd, cd = torch.from_numpy(y).cuda(), torch.from_numpy(sigma).cuda(), torch.from_numpy(cand).cuda()
    bits = K.rate_curve(yd, sd, cd, gc["table_dev"], gc["tables"], gc["bound"], lanes)
    again = K.rate_curve(yd, sd, cd, gc["table_dev"], gc["tables"], gc["bound"], lanes)
    assert bits.shape == (B * lanes, K_) and bits.dtype == torch.int64
    assert torch.equal(bits, again)
    got = bits.cpu().numpy()
    # 1. the restatement
    want = RX.rate_curve(y, sigma, B * lanes, per_seg, lanes, cand, gc["scale_table"], gc["bound"], gc["costs"], gc["sizes"], gc["offsets"], 4)
    assert np.array_equal(got, want)
    # 2. what the quantiser kernel itself writes at each step
    raw0 = escapes = 0
    for k in range(K_):
        steps = cand[:, k] if cpi else cand[k:k + 1]
        sym, idx, _ = K.gc_quantize_index_q(yd, sd, steps, gc["table_dev"], gc["bound"], want_yhat=False)
        sym, idx = sym.cpu().numpy().reshape(-1), idx.cpu().numpy().reshape(-1)
        assert np.array_equal(got[:, k], RX.symbol_costs(sym, idx, gc["costs"], gc["sizes"], gc["offsets"], 4).reshape(B * lanes, per_seg).sum(1))
        value, mx = sym.astype(np.int64) - gc["offsets"][idx], gc["sizes"][idx] - 2
        raw0 += int((value == mx).sum())
        escapes += int(((value < 0) | (value > mx)).sum())
    if lanes * per_seg > 4:     # the planted cases are there: a value at max (raw 0) and escapes
        assert raw0 >= 1 and escapes >= 2
        assert np.abs(y).max() / cand.min() == 2.0 ** 30


def test_rate_curve_on_a_constant_latent_by_hand(gc):
    """sigma = 1, y = 0 at step 1: every symbol is row idx(1.0)'s centre; the sum is n times that one table entry."""
    from cbench_basic_amd.nn import kernels as K
    n = 1000
    y, s = torch.zeros(2, n).cuda(), torch.ones(2, n).cuda()
    bits = K.rate_curve(y, s, torch.tensor([1.0]).cuda(), gc["table_dev"], gc["tables"], gc["bound"], 1).cpu().numpy()
    row = int(QX.index_rule(np.array([1.0], np.float32), gc["scale_table"])[0])
    centre = int(gc["costs"][row, -int(gc["offsets"][row])])
    assert bits.tolist() == [[n * centre], [n * centre]]
    assert centre == min(int(v) for v in gc["costs"][row, :gc["sizes"][row] - 1])      # the centre is the row's cheapest symbol


def test_select_and_refine_follow_the_restatement(gc):
    from cbench_basic_amd.nn import kernels as K
    B, lanes, per_seg, K_ = 3, 2, 257, 8
    cand = RX.first_grid(K_, (0.25, 32.0))
    y, sigma = _inputs(gc, B, lanes, per_seg, cand, seed=5)
    yd, sd = torch.from_numpy(y).cuda(), torch.from_numpy(sigma).cuda()
    cd = torch.from_numpy(cand).cuda()
    bits = K.rate_curve(yd, sd, cd, gc["table_dev"], gc["tables"], gc["bound"], lanes)
    hb = bits.cpu().numpy()
    extra = np.array([3, 0, 11], np.int32)
    preds = np.array([[4 * int(extra[b]) + sum(RX.stream_bound(hb[b * lanes + l, k], per_seg) for l in range(lanes)) for k in range(K_)]
                      for b in range(B)])
    # budgets: exactly one candidate's prediction, one byte under the cheapest (nothing fits), far above everything
    budgets = np.array([preds[0, 4], preds[1].min() - 1, 1 << 40], np.int64)
    steps, choice, pred = K.rate_select(bits, per_seg, cd, torch.from_numpy(budgets).cuda(), torch.from_numpy(extra).cuda(), lanes)
    ws, wc, wp = RX.select(hb, lanes, per_seg, cand, budgets, extra)
    assert np.array_equal(choice.cpu().numpy(), wc) and np.array_equal(pred.cpu().numpy(), wp)
    assert np.array_equal(steps.cpu().numpy().view(np.int32), ws.view(np.int32))
    assert wc[1] == (K_ - 1) | RX.NO_FIT and wc[2] == 0 and 0 < wc[0] <= 4
    grid = K.rate_refine(cd, choice)
    want = RX.refine(cand, wc, B)
    assert np.array_equal(grid.cpu().numpy().view(np.int32), want.view(np.int32))
    # second pass on the per-image grids, no extra words
    bits2 = K.rate_curve(yd, sd, grid, gc["table_dev"], gc["tables"], gc["bound"], lanes)
    assert np.array_equal(bits2.cpu().numpy(), RX.rate_curve(y, sigma, B * lanes, per_seg, lanes, want, gc["scale_table"], gc["bound"],
                                                             gc["costs"], gc["sizes"], gc["offsets"], 4))
    steps2, choice2, pred2 = K.rate_select(bits2, per_seg, grid, torch.from_numpy(budgets).cuda(), None, lanes)
    ws2, wc2, wp2 = RX.select(bits2.cpu().numpy(), lanes, per_seg, want, budgets, None)
    assert np.array_equal(choice2.cpu().numpy(), wc2) and np.array_equal(pred2.cpu().numpy(), wp2)
    assert np.array_equal(steps2.cpu().numpy().view(np.int32), ws2.view(np.int32))
    grid3 = K.rate_refine(grid, choice2)
    assert np.array_equal(grid3.cpu().numpy().view(np.int32), RX.refine(want, wc2, B).view(np.int32))
    # settled images repeat their step
    assert (grid3.cpu().numpy()[2] == cand[0]).all()


def test_select_and_refine_on_hand_made_curves():
    from cbench_basic_amd.nn import kernels as K
    per = 1000
    bb = lambda v: ((v // 4 - 2) << 21) - 4 * per
    bits = np.array([[bb(400), bb(200), bb(300), bb(100)], [bb(400), bb(300), bb(250), bb(240)], [bb(200), bb(100), bb(80), bb(40)]], np.int64)
    cand = torch.tensor([0.5, 1.0, 2.0, 4.0]).cuda()
    steps, choice, pred = K.rate_select(torch.from_numpy(bits).cuda(), per, cand, torch.tensor([200, 200, 200]).cuda())
    assert choice.tolist() == [1, 3 | RX.NO_FIT, 0] and steps.tolist() == [1.0, 4.0, 0.5] and pred.tolist() == [200, 240, 200]
    assert K.rate_refine(cand, choice).tolist() == [[0.625, 0.75, 0.875, 1.0], [4.0] * 4, [0.5] * 4]
    lo = np.float32(1.7)
    hi = np.nextafter(lo, np.float32(2))
    for grid, ch in ((np.array([lo, hi, 3, 4], np.float32), 1), (np.array([0.1, 0.2, lo, hi], np.float32), 3)):
        got = K.rate_refine(torch.from_numpy(grid).cuda(), torch.tensor([ch], dtype=torch.int32).cuda()).cpu().numpy()
        assert np.array_equal(got.view(np.int32), RX.refine(grid, [ch], 1).view(np.int32)) and got[0, 3] == hi
    rng = np.random.default_rng(7)
    grids = np.sort(rng.uniform(0.0625, 64, (64, 7)).astype(np.float32), axis=1)
    ch = rng.integers(0, 7, 64).astype(np.int32)
    got = K.rate_refine(torch.from_numpy(grids).cuda(), torch.from_numpy(ch).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.int32), RX.refine(grids, ch, 64).view(np.int32))


def test_rate_steps_chains_the_three(gc):
    from cbench_basic_amd.nn import kernels as K
    B, lanes, per = 3, 1, 4097
    cand = RX.first_grid(16)
    y, sigma = _inputs(gc, B, lanes, per, cand, seed=9)
    yd, sd = torch.from_numpy(y).cuda(), torch.from_numpy(sigma).cuda()
    budgets = np.array([3000, 1500, 6000], np.int64)
    steps, choice, pred, trace = K.rate_steps(yd, sd, torch.from_numpy(budgets).cuda(), None, cand, 3, gc["table_dev"], gc["tables"],
                                              gc["bound"], lanes, return_trace=True)
    c, grids = cand, []
    for p in range(3):
        bits = RX.rate_curve(y, sigma, B, per, 1, c, gc["scale_table"], gc["bound"], gc["costs"], gc["sizes"], gc["offsets"], 4)
        assert np.array_equal(trace[p][1].cpu().numpy(), bits)
        ws, wc, wp = RX.select(bits, 1, per, c, budgets)
        assert np.array_equal(trace[p][2].cpu().numpy(), wc)
        grids.append(c)
        c = RX.refine(c, wc, B)
    assert np.array_equal(steps.cpu().numpy().view(np.int32), ws.view(np.int32)) and np.array_equal(pred.cpu().numpy(), wp)
    assert (pred.cpu().numpy() <= budgets).all() and not (choice.cpu().numpy() & RX.NO_FIT).any()
    for bad in (dict(passes=0), dict(passes=4), dict(candidates=[1.0]), dict(candidates=[2.0, 1.0]), dict(candidates=[0.01, 1.0])):
        kw = dict(candidates=cand, passes=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            K.rate_steps(yd, sd, torch.from_numpy(budgets).cuda(), None, kw["candidates"], kw["passes"], gc["table_dev"], gc["tables"])


def test_entry_points_refuse(gc):
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    L = _lib.lib()
    y = torch.zeros(4, 64).cuda()
    cand = torch.ones(33).cuda()
    bits = torch.zeros(4 * 33, dtype=torch.int64).cuda()
    tab, t = gc["table_dev"], gc["tables"]

    def curve(n_seg=4, per_seg=64, segs=1, n_cand=2, cpi=0, tables=t):
        return L.basic_gc_rate_curve_dev(y.data_ptr(), y.data_ptr(), n_seg, per_seg, segs, cand.data_ptr(), n_cand, cpi, tab.data_ptr(),
                                         tab.numel(), 0.11, tables._h, bits.data_ptr(), None)
    assert curve() == _lib.OK
    for kw in (dict(n_cand=0), dict(n_cand=33), dict(cpi=2), dict(n_seg=4, segs=3), dict(n_seg=0), dict(per_seg=0), dict(segs=0),
               dict(per_seg=(1 << 41) + 1)):
        assert curve(**kw) == _lib.ERR_INVALID, kw
    freqs = np.full((2, 8), 5, np.int32)
    no_bypass = K.RansTables(freqs=freqs, nsym=[8, 8], offsets=[0, 0], precision=16, bypass=False)
    coarse = K.RansTables(freqs=freqs, nsym=[8, 8], offsets=[0, 0], precision=12, bypass=True)
    assert curve(tables=no_bypass) == _lib.ERR_INVALID and curve(tables=coarse) == _lib.ERR_INVALID
    assert "bypass" in _lib.last_error()
    i64, f32, i32 = (torch.zeros(4, dtype=d).cuda() for d in (torch.int64, torch.float32, torch.int32))

    def select(n_images=4, segs=1, per_seg=64, n_cand=2, cpi=0):
        return L.basic_rate_select_dev(bits.data_ptr(), n_images, segs, per_seg, cand.data_ptr(), n_cand, cpi, None, i64.data_ptr(),
                                       f32.data_ptr(), i32.data_ptr(), i64.data_ptr(), None)
    assert select() == _lib.OK
    for kw in (dict(n_images=0), dict(segs=0), dict(per_seg=0), dict(n_cand=0), dict(n_cand=33), dict(cpi=3), dict(per_seg=1 << 42)):
        assert select(**kw) == _lib.ERR_INVALID, kw
    out = torch.zeros(4 * 32).cuda()
    refine = lambda n_cand=2, cpi=0, n=4, dst=out: L.basic_rate_refine_dev(cand.data_ptr(), cpi, n_cand, i32.data_ptr(), n, cand.data_ptr(),
                                                                            dst.data_ptr(), None)
    assert refine() == _lib.OK
    for kw in (dict(n_cand=0), dict(n_cand=33), dict(cpi=2), dict(n=0), dict(dst=cand)):
        assert refine(**kw) == _lib.ERR_INVALID, kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        K.rate_curve(y, y, cand[:2], tab, t, 0.11, lanes=3)
    with pytest.raises(ValueError):
        K.rate_curve(y, y, torch.ones(3, 2).cuda(), tab, t, 0.11)
