"""Rate control of the hyperprior y coder, what needs no GPU (INTEGRATION.md "Rate control"): the byte bound against the CPU rANS
oracle on the sweep that established it, the library's host cost table against the NumPy restatement (tests/rate_exact.py), the
select rule and the float32 refinement on hand-made cases, and every refusal of a request."""
import numpy as np
import pytest

import qstep_exact as QX
import rate_exact as RX

BOUND = 0.11


@pytest.fixture(scope="module")
def y_tables(oracle):
    """The y coder's tables (64 scales, compressai's GaussianConditional.update) quantised with the oracle:
    (cdf int32 [64][L], sizes, offsets, scale table float32 [64])."""
    import torch
    from scipy.stats import norm
    st = torch.exp(torch.linspace(np.log(0.11), np.log(256.0), 64)).float()
    mult = -norm.ppf(1e-9 / 2)
    center = torch.ceil(st * mult).int()
    length = 2 * center + 1
    L = int(length.max())
    samples = torch.abs(torch.arange(L).int() - center[:, None]).float()
    phi = lambda v: 0.5 * torch.erfc(-(2 ** -0.5) * v)
    upper, lower = phi((0.5 - samples) / st[:, None]), phi((-0.5 - samples) / st[:, None])
    pmf, tail = (upper - lower).numpy(), (2 * lower[:, :1]).numpy()
    cdf = np.zeros((64, L + 2), dtype=np.int32)
    for i in range(64):
        q = oracle.pmf_to_quantized_cdf(np.concatenate([pmf[i, :int(length[i])], tail[i]]).astype(np.float32), 16)
        cdf[i, :len(q)] = q
    return cdf, (length + 2).numpy().astype(np.int32), (-center).numpy().astype(np.int32), st.numpy()


# ---------------------------------------------------------------- the byte bound
def test_byte_bound_on_the_oracle_sweep(oracle, y_tables):
    """192 streams: 12 lengths x 8 steps x {plain, escape-heavy}.  Per stream actual <= predicted <= actual + 4 bytes."""
    cdf, sizes, offsets, st = y_tables
    table = RX.cost_table(cdf, sizes)
    enc = oracle.Rans64Encoder(16, True, 4)
    enc.init_cdf_params(cdf, sizes, offsets)
    rng = np.random.default_rng(0)
    exact = above = 0
    most_escapes = 0.0
    for n in (1, 2, 3, 7, 33, 64, 100, 1000, 4096, 12288, 49152, 200000):
        sigma = np.exp(rng.uniform(np.log(0.05), np.log(300.0), n)).astype(np.float32)
        noise = rng.standard_normal(n).astype(np.float32)
        for spread in (1.0, 6.0):
            y = (noise * sigma * np.float32(spread)).astype(np.float32)
            for step in (0.0625, 0.25, 0.7, 1, 1.9, 4, 16, 64):
                sym, idx, _ = QX.quantize_index_q(y, sigma, [step], n, st, BOUND)
                costs = RX.symbol_costs(sym, idx, table, sizes, offsets, 4)
                pred = RX.stream_bound(costs.sum(), n)
                actual = len(enc.encode_with_indexes(sym, idx))
                value = sym - offsets[idx]
                most_escapes = max(most_escapes, float(((value < 0) | (value >= sizes[idx] - 2)).mean()) if n >= 1000 else 0.0)
                assert actual <= pred <= actual + 4, (n, spread, step, actual, pred)
                exact += pred == actual
                above += pred == actual + 4
    assert exact + above == 192
    assert most_escapes > 0.2   # the escape-heavy half does escape


def test_byte_bound_holds_on_other_inputs(oracle, y_tables):
    """Constant symbols at a row's cheapest entry, all-escape streams, a one-row stream: only actual <= predicted is promised."""
    cdf, sizes, offsets, st = y_tables
    table = RX.cost_table(cdf, sizes)
    enc = oracle.Rans64Encoder(16, True, 4)
    enc.init_cdf_params(cdf, sizes, offsets)
    rng = np.random.default_rng(1)
    cases = [(np.zeros(5000, np.int32), np.zeros(5000, np.int32)),                       # the cheapest symbol of the narrowest row
             (np.full(3000, 1 << 30, np.int32), np.full(3000, 63, np.int32)),            # 8-digit escapes only
             (np.full(3000, -(1 << 30), np.int32), np.full(3000, 5, np.int32)),
             (rng.integers(-40, 40, 20000).astype(np.int32), rng.integers(0, 64, 20000).astype(np.int32)),
             (np.array([7], np.int32), np.array([20], np.int32))]
    for sym, idx in cases:
        pred = RX.stream_bound(RX.symbol_costs(sym, idx, table, sizes, offsets, 4).sum(), sym.size)
        assert len(enc.encode_with_indexes(sym, idx)) <= pred


# ---------------------------------------------------------------- the cost table
def test_host_cost_table_is_the_restatement(y_tables):
    from cbench_basic_amd._lib import BasicHipInvalid
    from cbench_basic_amd.nn import kernels as K
    cdf, sizes, offsets, _ = y_tables
    got = K.rans_cost_table(cdf, sizes, 16)
    want = RX.cost_table(cdf, sizes, 16)
    assert got.shape == want.shape == cdf.shape and got.dtype == np.uint32
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1      # libm's log2 against NumPy's: one unit of 2^-16 bit
    for r in range(64):
        assert (got[r, sizes[r] - 1:] == 0).all() and (got[r, :sizes[r] - 1] > 0).all()
    # exact where log2 is: powers of two
    c = np.array([[0, 1, 3, 1 << 15, 1 << 16, 0]], dtype=np.int32)
    t = K.rans_cost_table(c, [5], 16)
    assert t[0].tolist() == [16 << 16, 15 << 16, int(np.rint((16 - np.log2((1 << 15) - 3)) * 65536)), 1 << 16, 0, 0]
    for bad in ([[0, 5, 5, 65536]], [[0, 9, 5, 65536]]):                          # a zero and a negative frequency inside the row
        with pytest.raises(BasicHipInvalid):
            K.rans_cost_table(np.array(bad, dtype=np.int32), [4], 16)
    K.rans_cost_table(np.array([[0, 5, 65536, 65536]], dtype=np.int32), [3], 16)   # ... but not beyond it


def test_symbol_costs_by_hand():
    # one row: offset -2, four table symbols (costs 10, 20, 30, 40) and the sentinel (cost 50), bypass precision 4
    table, sizes, offsets = np.array([[10, 20, 30, 40, 50, 0]], np.uint32), [6], [-2]
    u = 65536
    esc = lambda nb: 50 + 4 * (nb + 1 + nb // 15) * u
    sym = np.array([-2, 1, 2, 3, -3, -4, 2 + 8, 2 + (1 << 27), -(1 << 30)], np.int32)
    # value:          0  3  4=max (raw 0)  5 (raw 2)  -1 (raw 1)  -2 (raw 3)  12 (raw 16: 2 digits)  raw 2^28 + ..: 8 digits; raw 2^31 - 5: 8
    want = [10, 40, esc(0), esc(1), esc(1), esc(1), esc(2), esc(8), esc(8)]
    assert RX.symbol_costs(sym, np.zeros(9, np.int32), table, sizes, offsets, 4).tolist() == want
    assert RX.escape_digits(np.array([0, 1, 15, 16, 255, 256, 0xFFFFFFFF]), 4).tolist() == [0, 1, 1, 2, 2, 3, 8]
    assert RX.escape_digits(np.array([1, 0xFFFFFFFF]), 1).tolist() == [1, 32]


# ---------------------------------------------------------------- grid, select, refine
def test_first_grid():
    from cbench_basic_amd.utils.rate import first_grid
    g = first_grid(16)
    assert g.dtype == np.float32 and g.size == 16 and g[0] == 2.0 ** -4 and g[-1] == 64.0
    assert np.array_equal(g, RX.first_grid(16)) and (np.diff(g) > 0).all()
    assert np.array_equal(first_grid(11), np.float32(2.0) ** np.arange(-4, 7))     # whole exponents: exact powers of two
    assert np.array_equal(first_grid(5, (0.5, 8)), RX.first_grid(5, (0.5, 8)))
    assert first_grid(2, (1, 2)).tolist() == [1.0, 2.0]


def _bits_for_bytes(nbytes, per_seg):
    """A bit count whose bound is exactly `nbytes` for one stream of per_seg symbols."""
    words = nbytes // 4 - 2
    return (words << 21) - 4 * per_seg


def test_select_takes_the_first_fit():
    per = 1000
    cand = np.array([0.5, 1.0, 2.0, 4.0], np.float32)
    curve = lambda *b: [_bits_for_bytes(v, per) for v in b]
    bits = np.array([curve(400, 200, 300, 100),        # not monotone: 200 fits at k = 1 although k = 2 does not
                     curve(400, 300, 250, 240),        # nothing fits 200
                     curve(200, 100, 80, 40),          # everything fits
                     curve(204, 200, 196, 100)], np.int64)
    steps, choice, pred = RX.select(bits, 1, per, cand, [200, 200, 200, 200])
    assert choice.tolist() == [1, 3 | RX.NO_FIT, 0, 1] and steps.tolist() == [1.0, 4.0, 0.5, 1.0]
    assert pred.tolist() == [200, 240, 200, 200]
    # words already spent count against the budget; lanes add up, each with its own two flush words
    steps, choice, pred = RX.select(bits, 1, per, cand, [200] * 4, extra_words=[25, 0, 30, 1])
    assert choice.tolist() == [3, 3 | RX.NO_FIT, 2, 2] and pred.tolist() == [200, 240, 200, 200]     # e.g. row 2: 320, 220, 200
    steps, choice, pred = RX.select(bits, 2, per, cand, [500, 300])                                  # images (row 0, row 1), (row 2, row 3)
    assert choice.tolist() == [1, 1] and pred.tolist() == [500, 300] and steps.tolist() == [1.0, 1.0]
    # one grid per image
    steps, _, _ = RX.select(bits, 1, per, np.stack([cand, cand * 2, cand * 3, cand * 4]), [200] * 4)
    assert steps.tolist() == [1.0, 8.0, 1.5, 4.0]
    # the bound itself: one more unit of cost past a word boundary is one more word
    assert RX.stream_bound(_bits_for_bytes(200, per), per) == 200 and RX.stream_bound(_bits_for_bytes(200, per) + (1 << 21), per) == 204
    assert RX.stream_bound(0, 1) == 8


def test_refine_in_float32():
    from cbench_basic_amd.utils.rate import refine_t
    cand = np.array([0.5, 1.0, 2.0, 4.0], np.float32)
    out = RX.refine(cand, [2, 0, 3 | RX.NO_FIT], 3)
    assert out[0].tolist() == [1.25, 1.5, 1.75, 2.0]
    assert out[1].tolist() == [0.5] * 4 and out[2].tolist() == [4.0] * 4            # settled images repeat their step
    assert np.array_equal(refine_t(4), np.array([0.25, 0.5, 0.75, 1.0], np.float32))
    assert np.array_equal(refine_t(7), (np.arange(1, 8, dtype=np.float32) / np.float32(7)))
    # hi - lo of one ulp: every interior point rounds to lo or hi, never outside [lo, hi]
    lo = np.float32(1.7)
    hi = np.nextafter(lo, np.float32(2))
    out = RX.refine(np.array([lo, hi], np.float32), [1], 1)
    assert out[0, 1] == hi and out[0, 0] in (lo, hi)
    out = RX.refine(np.array([0.1, lo, hi, 60], np.float32), [2], 1)
    assert out[0, 3] == hi and all(v in (lo, hi) for v in out[0])
    # the clamp: 7 candidates, t[5] = 6/7 rounds so that lo + d * t stays <= hi; t[K - 1] is never used (the last entry is hi itself)
    rng = np.random.default_rng(3)
    for _ in range(200):
        a = np.sort(rng.uniform(0.0625, 64, 2).astype(np.float32))
        if a[0] == a[1]:
            continue
        g = RX.refine(np.array([a[0], a[1]] + [64.0] * 5, np.float32), [1], 1)[0]
        assert g[-1] == a[1] and (g >= a[0]).all() and (g <= a[1]).all() and (np.diff(g) >= 0).all()
    # a grid per image
    out = RX.refine(np.array([[1, 2, 3, 4], [1, 3, 5, 9]], np.float32), [1, 3], 2)
    assert out.tolist() == [[1.25, 1.5, 1.75, 2.0], [6.0, 7.0, 8.0, 9.0]]


# ---------------------------------------------------------------- refusals
def test_request_validation():
    from cbench_basic_amd.utils.rate import RateTarget, budgets_from, check_budgets, check_candidates, check_passes, first_grid
    assert budgets_from(1000, None, 3, 64, 64).tolist() == [1000]
    assert budgets_from(None, 0.5, 3, 64, 96).tolist() == [64 * 96 // 16]
    assert budgets_from(None, [0.5, 1.0, 0.3], 3, 64, 64).tolist() == [256, 512, int(np.floor(0.3 * 4096 / 8))]
    assert budgets_from([10, 20, 30], None, 3, 8, 8).dtype == np.int64
    for tb, bpp in ((None, None), (100, 1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            budgets_from(tb, bpp, 1, 64, 64)
    for bad in (0, -5, 1.5, float("nan"), float("inf"), [100, 200], [], [[1, 2, 3]], "x"):
        with pytest.raises(ValueError):
            budgets_from(bad, None, 3, 64, 64)
    for bad in (0.0, -1.0, float("nan"), 1e-6, [1.0, 2.0]):      # 1e-6 bpp of 64 x 64 is under one byte
        with pytest.raises(ValueError):
            budgets_from(None, bad, 3, 64, 64)
    assert check_budgets([5, 6], 2).tolist() == [5, 6]
    for bad in (1, 33, 0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            first_grid(bad)
    for bad in ((1, 1), (2, 1), (2 ** -5, 4), (1, 65), (float("nan"), 2), (1,), 3, (1, 1 + 2 ** -22)):
        with pytest.raises(ValueError):
            first_grid(16, bad)
    for bad in (0, 4, 1.0, True, None):
        with pytest.raises(ValueError):
            check_passes(bad)
    assert [check_passes(p) for p in (1, 2, 3)] == [1, 2, 3]
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0], [0.01, 1.0], [1.0, 65.0], [1.0, float("nan")], list(range(1, 34))):
        with pytest.raises(ValueError):
            check_candidates(bad)
    rt = RateTarget([100, 200], batch=2)
    assert rt.passes == 2 and rt.candidates.size == 16 and rt.budgets_for(2).tolist() == [100, 200]
    with pytest.raises(ValueError):
        rt.budgets_for(3)
    assert RateTarget(50).budgets_for(3).tolist() == [50, 50, 50]


def test_codec_refuses_before_any_launch():
    """On a codec that was never moved to a GPU nor given tables: every refusal comes from the host checks."""
    import torch
    from cbench_basic_amd.presets import hyperprior_codec, topogroup_ar_codec
    codec = hyperprior_codec().eval()
    x = torch.rand(3, 3, 64, 64)
    for kw in (dict(), dict(target_bytes=100, target_bpp=1.0), dict(target_bytes=0), dict(target_bytes=-1), dict(target_bpp=0.0),
               dict(target_bytes=[100, 200]), dict(target_bytes=100, candidates=1), dict(target_bytes=100, candidates=33),
               dict(target_bytes=100, passes=0), dict(target_bytes=100, passes=4), dict(target_bytes=100, step_range=(2.0, 1.0)),
               dict(target_bytes=100, step_range=(0.01, 1.0)), dict(target_bytes=100, step_range=(1.0, 100.0))):
        with pytest.raises(ValueError):
            codec.compress_to_rate(x, **kw)
    with pytest.raises(ValueError):
        codec.compress_to_rate(x[0], target_bytes=100)
    with pytest.raises(ValueError, match="two ways"):
        codec.entropy_coder.encode(x, qstep=1.0, rate_target=100)
    with pytest.raises(TypeError, match="rate_target"):
        topogroup_ar_codec().eval().compress_to_rate(x, target_bytes=100)
