"""basic_rate_select_groups_dev on the GPU (INTEGRATION.md "Tiled pictures: step and byte budget"): exactly the NumPy restatement
(tests/tiled_rate_exact.py) on synthetic curves -- groups of 1, 2, 65 and 257 tiles in one call (less than a wave, more than a
wave, more than a workgroup of 256), listed in shuffled order, lanes 1 and 4, mixed per_seg, K of 2, 16 and 32 with shared and
per-group grids, a curve that is not monotone, a budget equal to the prediction and one byte below it, a group nothing fits beside
one that fits, large extra words and sums past 2^32 -- the same at every block width, and every refusal before anything is written."""
import numpy as np
import pytest
import torch

import tiled_rate_exact as TX

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 65, 257]


def _case(lanes, K_, per_group, seed):
    """Synthetic curves: (bits [S][K], first_seg, per_seg, extra, groups, cand), tiles scattered over the rows and the groups' lists shuffled."""
    rng = np.random.default_rng(seed)
    T = sum(SIZES) + 3                                    # three tiles in no group
    order = rng.permutation(T)
    first_seg = (order * lanes).astype(np.int32)          # tile t owns rows order[t] * lanes ..: not in tile order
    per_seg = rng.choice([1, 63, 4096, 65536, 1 << 30], T).astype(np.int64)
    # about 2^34 .. 2^45 units of 2^-16 bit a stream, falling with k, with noise: sums of bytes pass 2^32 in the large groups
    base = np.exp2(rng.uniform(34, 45, (T * lanes, 1)))
    fall = np.exp2(-np.arange(K_) * (8.0 / K_))[None, :]
    bits = (base * fall * rng.uniform(0.9, 1.1, (T * lanes, K_))).astype(np.int64)
    extra = rng.integers(0, 1 << 20, T).astype(np.int32)
    extra[:4] = [0, (1 << 31) - 1, 1 << 30, 7]            # large words: 4 * extra needs 64 bits
    tiles = rng.permutation(T)[:sum(SIZES)]
    groups, at = [], 0
    for n in SIZES:
        groups.append([int(t) for t in tiles[at:at + n]])
        at += n
    cand = np.sort(rng.uniform(0.0625, 64, (len(SIZES), K_) if per_group else (K_,)).astype(np.float32), axis=-1)
    return bits, first_seg, per_seg, extra, groups, cand


def _preds(bits, first_seg, lanes, per_seg, extra, groups, K_):
    return [[sum(TX.tile_pred(bits.tolist(), int(first_seg[t]), lanes, int(per_seg[t]), int(extra[t]), k) for t in g) for k in range(K_)] for g in groups]


def _run(K, bits, first_seg, per_seg, extra, groups, cand, budgets, lanes, **kw):
    out = K.rate_select_groups(torch.from_numpy(bits).cuda(), first_seg, per_seg, groups, torch.from_numpy(cand).cuda(),
                               torch.from_numpy(np.asarray(budgets, np.int64)).cuda(), None if extra is None else torch.from_numpy(extra).cuda(),
                               lanes, **kw)
    return [t.cpu().numpy() for t in out]


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g, w.view(np.int32) if w.dtype == np.float32 else w)


@pytest.mark.parametrize("lanes,K_,per_group", [(1, 2, 0), (4, 2, 1), (1, 16, 1), (4, 16, 0), (1, 32, 0), (4, 32, 1)])
def test_select_groups_is_the_restatement(lanes, K_, per_group):
    from cbench_basic_amd.nn import kernels as K
    bits, first_seg, per_seg, extra, groups, cand = _case(lanes, K_, per_group, seed=lanes * 100 + K_)
    # not monotone on purpose: the two-tile group's candidate 0 is made the cheapest of all, its last the dearest
    for t in groups[1]:
        rows = slice(int(first_seg[t]), int(first_seg[t]) + lanes)
        bits[rows, 0], bits[rows, K_ - 1] = bits[rows].min() // 2, bits[rows].max() * 2
    preds = _preds(bits, first_seg, lanes, per_seg, extra, groups, K_)
    assert max(max(p) for p in preds) > 1 << 32
    mid = K_ // 2
    # group 0: exactly candidate mid's prediction; group 1: far under candidate 0's only where the curve is monotone -- here candidate 0
    # fits a budget that candidates 1.. do not (a bisection would not look there); group 2: nothing fits; group 3: one byte under mid's
    budgets = [preds[0][mid], preds[1][0], min(preds[2]) - 1, preds[3][mid] - 1]
    got = _run(K, bits, first_seg, per_seg, extra, groups, cand, budgets, lanes)
    want = TX.select_groups(bits, first_seg, lanes, per_seg, extra, groups, cand, budgets)
    _same(got, want)
    steps, choice, pred, tile_steps, tile_pred = got
    assert choice[0] <= mid and pred[0] <= budgets[0] and (choice[0] == mid or preds[0][choice[0]] <= budgets[0])
    assert choice[1] == 0 and all(p > budgets[1] for p in preds[1][1:])                 # first fit, not a bisection
    assert choice[2] == (K_ - 1) | TX.NO_FIT and pred[2] == preds[2][K_ - 1] > budgets[2]  # no fit beside groups that fit
    assert choice[3] != mid and pred[3] <= budgets[3] or choice[3] & TX.NO_FIT
    for g, members in enumerate(groups):
        assert int(tile_pred[members].sum()) == int(pred[g]) and (tile_steps[members] == steps[g]).all()
    listed = {t for g in groups for t in g}
    free = [t for t in range(len(first_seg)) if t not in listed]
    assert len(free) == 3 and (tile_steps[free] == 1).all() and (tile_pred[free] == 0).all()
    # the same input at every block width, and without extra words
    for width in (64, 128, 512, 1024):
        _same(_run(K, bits, first_seg, per_seg, extra, groups, cand, budgets, lanes, block_threads=width), want)
    _same(_run(K, bits, first_seg, per_seg, None, groups, cand, budgets, lanes, block_threads=64),
          TX.select_groups(bits, first_seg, lanes, per_seg, None, groups, cand, budgets))


def test_budget_at_and_one_byte_below_the_prediction():
    from cbench_basic_amd.nn import kernels as K
    bits, first_seg, per_seg, extra, groups, cand = _case(1, 16, 0, seed=5)
    bits = np.sort(bits, axis=1)[:, ::-1].copy()                                     # strictly falling curves: one answer per budget
    preds = _preds(bits, first_seg, 1, per_seg, extra, groups, 16)
    for k in (0, 7, 15):
        at = _run(K, bits, first_seg, per_seg, extra, groups, cand, [p[k] for p in preds], 1)
        below = _run(K, bits, first_seg, per_seg, extra, groups, cand, [p[k] - 1 for p in preds], 1)
        assert at[1].tolist() == [k] * 4 and at[2].tolist() == [p[k] for p in preds]
        assert below[1].tolist() == ([k + 1] * 4 if k < 15 else [15 | TX.NO_FIT] * 4)
        _same(below, TX.select_groups(bits, first_seg, 1, per_seg, extra, groups, cand, [p[k] - 1 for p in preds]))


def test_refine_takes_groups_for_images():
    """rate_refine_kernel is unchanged: the groups' choices go where the images' went."""
    import rate_exact as RX
    from cbench_basic_amd.nn import kernels as K
    bits, first_seg, per_seg, extra, groups, cand = _case(1, 16, 0, seed=9)
    preds = _preds(bits, first_seg, 1, per_seg, extra, groups, 16)
    budgets = [preds[0][3], preds[1][0], min(preds[2]) - 1, preds[3][9]]
    steps, choice, pred, _, _ = K.rate_select_groups(torch.from_numpy(bits).cuda(), first_seg, per_seg, groups, torch.from_numpy(cand).cuda(),
                                                    torch.tensor(budgets).cuda(), torch.from_numpy(extra).cuda(), 1)
    grid = K.rate_refine(torch.from_numpy(cand).cuda(), choice).cpu().numpy()
    assert grid.shape == (4, 16) and np.array_equal(grid.view(np.int32), RX.refine(cand, choice.cpu().numpy(), 4).view(np.int32))


def test_the_entry_point_refuses_before_it_writes():
    """Arguments only: every refusal comes back from the host checks, nothing is enqueued, and the sentinels stay."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    L = _lib.lib()
    T, G, K_, lanes = 6, 2, 4, 2
    bits = torch.zeros((T * lanes, K_), dtype=torch.int64).cuda()
    cand = torch.ones(32).cuda()
    budget = torch.zeros(G, dtype=torch.int64).cuda()
    plan = torch.full((64,), -7, dtype=torch.int64).cuda()
    outs = dict(steps=torch.full((G,), -7.0).cuda(), choice=torch.full((G,), -7, dtype=torch.int32).cuda(),
                pred=torch.full((G,), -7, dtype=torch.int64).cuda(), tsteps=torch.full((T,), -7.0).cuda(),
                tpred=torch.full((T,), -7, dtype=torch.int64).cuda())
    first = np.arange(T, dtype=np.int32) * lanes
    per = np.full(T, 100, np.int64)
    gfirst, gtiles = np.array([0, 2, 6], np.int32), np.array([5, 0, 1, 2, 3, 4], np.int32)

    def call(n_seg=T * lanes, lanes=lanes, n_tiles=T, first=first, per=per, n_groups=G, gfirst=gfirst, gtiles=gtiles, n_cand=K_, cpg=0,
             block=0, null=None):
        p = dict(bits=bits.data_ptr(), first=first.ctypes.data, per=per.ctypes.data, gfirst=gfirst.ctypes.data, gtiles=gtiles.ctypes.data,
                 plan=plan.data_ptr(), cand=cand.data_ptr(), budget=budget.data_ptr(), **{k: v.data_ptr() for k, v in outs.items()})
        if null:
            p[null] = None
        return L.basic_rate_select_groups_dev(p["bits"], n_seg, lanes, n_tiles, p["first"], p["per"], None, n_groups, p["gfirst"], p["gtiles"],
                                              p["plan"], p["cand"], n_cand, cpg, p["budget"], p["steps"], p["choice"], p["pred"], p["tsteps"],
                                              p["tpred"], block, None)
    i32 = lambda *v: np.array(v, np.int32)
    bad = [dict(n_cand=0), dict(n_cand=33), dict(cpg=2), dict(lanes=0), dict(n_tiles=0), dict(n_groups=0), dict(n_seg=0),
           dict(gfirst=i32(0, 2, 2)),                       # an empty group
           dict(gfirst=i32(0, 0, 6)), dict(gfirst=i32(1, 2, 6)), dict(gfirst=i32(0, 2, 7)),
           dict(gtiles=i32(5, 0, 1, 2, 3, 6)), dict(gtiles=i32(5, 0, 1, 2, 3, -1)),          # a tile index out of range
           dict(gtiles=i32(5, 0, 1, 2, 3, 5)), dict(gtiles=i32(0, 0, 1, 2, 3, 4)),           # a tile listed twice
           dict(first=i32(0, 2, 4, 6, 8, 11)), dict(first=i32(-1, 2, 4, 6, 8, 10)), dict(n_seg=T * lanes - 1),   # rows outside the curves
           dict(per=np.array([100] * 5 + [0], np.int64)), dict(per=np.array([100] * 5 + [1 << 42], np.int64)),
           dict(block=32), dict(block=96), dict(block=2048), dict(block=-64)]
    bad += [dict(null=name) for name in ("bits", "first", "per", "gfirst", "gtiles", "plan", "cand", "budget", "steps", "choice", "pred",
                                         "tsteps", "tpred")]
    for kw in bad:
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert "rate_select_groups" in _lib.last_error()
    torch.cuda.synchronize()
    assert (plan == -7).all() and all((v == -7).all() for v in outs.values())
    assert call() == _lib.OK                                      # the same arguments, unbroken
    torch.cuda.synchronize()
    assert outs["choice"].tolist() == [3 | TX.NO_FIT] * 2 and (outs["tsteps"] == 1).all()     # budget 0: nothing fits
    # the Python entry: shapes that do not match
    good = dict(bits=bits, tile_first_seg=first, tile_per_seg=per, groups=[[5, 0], [1, 2, 3, 4]], cand=cand[:K_], budgets=budget)
    for kw in (dict(tile_per_seg=per[:-1]), dict(budgets=budget[:1]), dict(cand=cand[:K_ + 1]), dict(cand=torch.ones(3, K_).cuda()),
               dict(tile_extra_words=torch.zeros(T - 1, dtype=torch.int32).cuda()), dict(groups=[])):
        with pytest.raises(ValueError):
            K.rate_select_groups(**{**good, **kw}, lanes=lanes)
    with pytest.raises(_lib.BasicHipError):
        K.rate_select_groups(**{**good, "groups": [[5, 0], [0, 2, 3, 4]]}, lanes=lanes)
