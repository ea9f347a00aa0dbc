"""Direct tests of csrc/entropy.hip against NumPy, torch-CPU and fp64 references (never another kernel of the library):

  * the Gaussian group step (pgm_gauss_{encode,index,scatter}_group_dev), exact: scales on table entries, exactly between two, outside
    the table, negative, infinite and NaN; tables that are sorted, repeated, unsorted and of length 1; residuals on k + 1/2 of both
    signs and parities; outputs in sentinel-filled buffers; and more elements than one grid pass (256 * 8 workgroups of 256 threads);
  * the elementwise kernels on more than one grid pass, with a plane size that is no power of two, exact;
  * mse_per_image against fp64 on the shapes that reach its 4-stream loop, its remainder loop, its scalar tail and the unaligned
    fallback, within the rounding bound of the kernel's own summation depth;
  * the rate kernels (gauss_nll_per_image in its three modes, eb_nll_per_image) against an fp64 restatement of their formulas
    (include/basic_hip.h section 4), within a budget MEASURED from the formula's own fp32 error, which three wrong pairings exceed."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0x7FC0BEEF   # NaN payload of the guard bands
FRESH = 0x7FC00001   # what a view holds before the launch: a NaN as float, no symbol or table row as integer
BAND = 4096
U = 2.0 ** -24       # unit roundoff of fp32
ONE_PASS = 256 * 8 * 256


def _K():
    from cbench_basic_amd.nn import kernels as K
    return K


def _guarded(n, off=64):
    """(buffer, view of n int32 inside it): guard bands on both sides, the view filled with FRESH."""
    buf = torch.full((off + n + BAND,), GUARD, dtype=torch.int32, device="cuda")
    buf[off: off + n] = FRESH
    return buf, buf[off: off + n]


def _guards_intact(buf, n, off=64):
    h = buf.cpu()
    return bool((h[:off] == GUARD).all()) and bool((h[off + n:] == GUARD).all())


# ---------------------------------------------------------------------------------------------------------------- Gaussian group step
def _first_argmin(s, tab):
    """argmin_j |s - tab[j]| in float32, the FIRST minimum, an infinite or NaN distance never being one: row 0 for a scale of
    +/-inf or NaN (what torch.argmin gives on all-inf or all-NaN distances)."""
    with np.errstate(invalid="ignore"):
        d = np.abs(s.astype(np.float32)[:, None] - tab.astype(np.float32)[None, :])
        best, bd = np.zeros(len(s), dtype=np.int32), d[:, 0].copy()
        for j in range(1, d.shape[1]):
            m = d[:, j] < bd
            best[m], bd[m] = j, d[m, j]
    return best


def _group_inputs(rng, B, C, hw, elems, tab):
    """y [B, C, hw], params [B, 2C, hw] (channel 2c = mean, 2c + 1 = scale).  Scales come from the table's edges -- its entries, the
    exact midpoints, just beside the first entries, outside the table, negative, infinite, NaN --, every one of them at a listed
    element; half of the residuals lie on a rounding tie, the others are ordinary floats.  Means are finite."""
    uniq = np.unique(tab.astype(np.float64))
    pool = np.concatenate([tab.astype(np.float64), (uniq[:-1] + uniq[1:]) / 2, [uniq[0] - 0.25, uniq[0] - 100.0, uniq[-1] + 0.25, uniq[-1] + 1000.0],
                           [-0.5, -3.0, 0.0, np.inf, -np.inf, np.nan], uniq[:8] * (1 + 2.0 ** -20), uniq[:8] * (1 - 2.0 ** -20)]).astype(np.float32)
    scale = pool[rng.integers(0, len(pool), size=(B, C * hw))]
    listed = B * len(elems)
    assert len(pool) <= listed
    scale[:, elems] = pool[np.arange(listed) % len(pool)][rng.permutation(listed)].reshape(B, -1)
    scale = scale.reshape(B, C, hw)
    mu = np.where(rng.random((B, C, hw)) < 0.5, rng.integers(-40, 41, size=(B, C, hw)) / 4.0, rng.normal(size=(B, C, hw)) * 3).astype(np.float32)
    tie = rng.integers(-6, 6, size=(B, C, hw)) + 0.5   # -5.5 .. 5.5: both signs, k even and odd
    y = np.where((rng.random((B, C, hw)) < 0.5) & (mu * 4 == np.rint(mu * 4)), mu + tie, rng.normal(size=(B, C, hw)) * 4).astype(np.float32)
    params = np.stack([mu, scale], axis=2).reshape(B, 2 * C, hw)
    return y, np.ascontiguousarray(params)


def _check_group(rng, B, C, hw, elems, tab, per_image, out_base):
    from cbench_basic_amd import _lib
    K, L = _K(), _lib.lib()
    n, chw = len(elems), C * hw
    y, params = _group_inputs(rng, B, C, hw, elems, tab)
    # ---- NumPy float32 reference
    c, p = elems // hw, elems % hw
    mu, sg = params[:, 2 * c, p], params[:, 2 * c + 1, p]            # [B, n]
    want_idx = _first_argmin(sg.reshape(-1), tab).reshape(B, n)
    q = np.rint(y.reshape(B, chw)[:, elems] - mu)                    # float32 subtraction, round half to even
    want_sym = q.astype(np.int32)
    want_y = (q + mu).astype(np.float32)
    # ---- the kernels, every output a view into a sentinel-filled buffer
    d_y, d_par = torch.from_numpy(y).cuda(), torch.from_numpy(params).cuda()
    d_el, d_tab = torch.from_numpy(elems.astype(np.int32)).cuda(), torch.from_numpy(tab.astype(np.float32)).cuda()
    (bs, sym), (bi, idx), (bi1, idx1), (by, ybuf), (by2, ybuf2) = (_guarded(B * per_image), _guarded(B * per_image), _guarded(B * per_image),
                                                                  _guarded(B * chw), _guarded(B * chw))
    st = K._stream()
    _lib.check(L.basic_pgm_gauss_encode_group_dev(d_y.data_ptr(), d_par.data_ptr(), B, C, hw, d_el.data_ptr(), n, d_tab.data_ptr(), len(tab),
                                                  sym.data_ptr(), idx.data_ptr(), per_image, out_base, ybuf.data_ptr(), st))
    _lib.check(L.basic_pgm_gauss_index_group_dev(d_par.data_ptr(), B, C, hw, d_el.data_ptr(), n, d_tab.data_ptr(), len(tab), idx1.data_ptr(),
                                                 per_image, out_base, st))
    _lib.check(L.basic_pgm_gauss_scatter_group_dev(sym.data_ptr(), d_par.data_ptr(), B, C, hw, d_el.data_ptr(), n, per_image, out_base,
                                                   ybuf2.data_ptr(), st))
    torch.cuda.synchronize()
    for name, buf, m in (("symbols", bs, B * per_image), ("indexes", bi, B * per_image), ("indexes (index only)", bi1, B * per_image),
                         ("ybuf", by, B * chw), ("ybuf (scatter)", by2, B * chw)):
        assert _guards_intact(buf, m), f"the launch wrote outside {name}"
    # expected buffers: FRESH everywhere but [out_base, out_base + n) of every image / the listed elements
    exp_sym = np.full((B, per_image), FRESH, dtype=np.int32)
    exp_idx = exp_sym.copy()
    exp_sym[:, out_base: out_base + n], exp_idx[:, out_base: out_base + n] = want_sym, want_idx
    exp_y = np.full((B, chw), FRESH, dtype=np.int32)
    exp_y[:, elems] = want_y.view(np.int32)
    got_sym, got_idx, got_idx1 = (t.cpu().numpy().reshape(B, per_image) for t in (sym, idx, idx1))
    got_y, got_y2 = (t.cpu().numpy().reshape(B, chw) for t in (ybuf, ybuf2))
    bad = [int((a != b).sum()) for a, b in ((got_sym, exp_sym), (got_idx, exp_idx), (got_idx1, exp_idx), (got_y, exp_y), (got_y2, exp_y))]
    print(f"B={B} C={C} hw={hw} n={n} table of {len(tab)}: differing symbols {bad[0]}, indexes {bad[1]}, indexes (mode 1) {bad[2]}, "
          f"ybuf bits {bad[3]}, scattered ybuf bits {bad[4]}")
    assert bad == [0, 0, 0, 0, 0]
    return want_idx, sg


GROUP_TABLES = {"half-step": 0.5 * np.arange(1, 65), "repeated": np.array([0.5, 0.5, 1.0, 1.0, 1.0, 2.0, 2.0, 4.0]),
                "unsorted": np.array([2.0, 0.5, 4.0, 1.0, 1.0, 3.0, 0.25]), "single": np.array([1.5])}


@pytest.mark.parametrize("name", list(GROUP_TABLES))
def test_gauss_group_step_exact(name):
    """B = 3, C = 5, hw = 21, an ascending strict subset of the elements, per_image > n_elems and out_base > 0."""
    rng = np.random.default_rng(len(name))
    B, C, hw = 3, 5, 21
    elems = np.sort(rng.choice(C * hw, size=70, replace=False))
    tab = GROUP_TABLES[name]
    want_idx, sg = _check_group(rng, B, C, hw, elems, tab, per_image=len(elems) + 9, out_base=4)
    # the edges were there: a tie between two rows goes to the first of them, non-finite scales to row 0
    sg, want_idx = sg.reshape(-1), want_idx.reshape(-1)
    assert np.isnan(sg).any() and np.isposinf(sg).any() and np.isneginf(sg).any() and (sg[np.isfinite(sg)] < 0).any()
    assert (want_idx[~np.isfinite(sg)] == 0).all()
    assert np.isin(sg, tab.astype(np.float32)).any()
    if len(tab) > 1:
        d = np.abs(sg[np.isfinite(sg), None].astype(np.float64) - tab[None, :])
        assert ((d == d.min(1, keepdims=True)).sum(1) > 1).any(), "no scale with two nearest rows"


def test_gauss_group_step_more_than_one_grid_pass():
    B, C, hw = 3, 192, 1024
    assert B * C * hw > ONE_PASS
    _check_group(np.random.default_rng(5), B, C, hw, np.arange(C * hw), GROUP_TABLES["half-step"], per_image=C * hw + 5, out_base=2)


# ---------------------------------------------------------------------------------------- elementwise kernels beyond one grid pass
def test_elementwise_kernels_grid_stride_and_channel_wrap():
    """600,001 elements (one grid pass is 524,288) for gc_quantize_index and i32_to_f32; B = 3, C = 7, hw = 28,573 (no power of two) for
    the EntropyBottleneck kernels: exact against torch on the CPU.  Floats are multiples of 1/2 or 1/8 (rounding ties included), the
    integers include the int32 extremes."""
    K = _K()
    g = torch.Generator().manual_seed(3)
    n = 600_001
    assert n > ONE_PASS
    table = torch.exp(torch.linspace(math.log(0.11), math.log(256), 64))
    y = torch.randint(-40, 41, (n,), generator=g).float() / 2
    s = torch.randint(0, 2400, (n,), generator=g).float() / 8
    s[-64:] = table   # (entries hit exactly, in the second pass)
    sym, idx, yhat = K.gc_quantize_index(y.cuda(), s.cuda(), table.cuda())
    sb = torch.max(s, torch.tensor(0.11))
    want = torch.full((n,), 63, dtype=torch.int32)
    for t in table[:-1]:
        want -= (sb <= t).int()
    assert torch.equal(idx.cpu(), want) and torch.equal(sym.cpu(), torch.round(y).int()) and torch.equal(yhat.cpu(), torch.round(y))
    ints = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).int()
    ints[:4] = torch.tensor([2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, -(2 ** 24) - 1], dtype=torch.int32)
    ints[-4:] = torch.tensor([-2 ** 31, 2 ** 31 - 1, 0, -1], dtype=torch.int32)
    assert torch.equal(K.i32_to_f32(ints.cuda()).cpu(), ints.float())
    B, C, hw = 3, 7, 28_573
    assert B * C * hw > ONE_PASS
    z = torch.randint(-64, 65, (B, C, hw), generator=g).float() / 8
    med = torch.randint(-16, 17, (C,), generator=g).float() / 8
    m3 = med.reshape(1, C, 1)
    sym, idx, zhat = K.eb_quantize_index(z.cuda(), med.cuda())
    assert torch.equal(sym.cpu(), torch.round(z - m3).int())
    assert torch.equal(zhat.cpu(), torch.round(z - m3) + m3)
    assert torch.equal(idx.cpu(), torch.arange(C, dtype=torch.int32).reshape(1, C, 1).expand(B, C, hw))
    si = torch.randint(-2 ** 31, 2 ** 31, (B, C, hw), generator=g, dtype=torch.int64).int()
    si[0, 0, :2] = torch.tensor([2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    si[-1, -1, -2:] = torch.tensor([-2 ** 31, 2 ** 31 - 1], dtype=torch.int32)
    si[1] = torch.randint(-300, 301, (C, hw), generator=g).int()   # ordinary symbols
    assert torch.equal(K.eb_dequantize(si.cuda(), med.cuda()).cpu(), si.float() + m3)


# ------------------------------------------------------------------------------------------------------------------ mse_per_image
def _mse_depth(elems, aligned):
    """Roundings on the longest path from one squared difference to the sum, as the kernel adds (1024 threads; a thread walks four
    16-byte streams, then the float4s that are left, then the scalar tail; then the streams, the lanes and 10 LDS levels)."""
    if not aligned:
        return -(-elems // 1024) + 10
    n4 = elems // 4
    four = -(-(n4 - 3072) // 4096) if n4 > 3072 else 0       # iterations of the 4-stream loop (thread 0)
    rest = -(-(n4 - 4096 * four) // 1024) if n4 > 4096 * four else 0
    tail = 1 if elems % 4 else 0
    return four + rest + 4 + tail + 10


@pytest.mark.parametrize("B,elems,offset", [(3, 1, 0), (3, 3, 0), (3, 4099, 0), (2, 4 * (2 * 4096 + 1024 + 37) + 2, 0), (2, 5000, 1),
                                            (1, 3 * 512 * 768, 0)])
def test_mse_per_image_vs_fp64(B, elems, offset):
    """All terms are non-negative, so the relative error is bounded by (depth + 3) roundings (the difference, the square, the final
    division), doubled for FMA contraction.  4099 elements: images 1 and 2 start unaligned; offset 1: a view one float into its
    allocation; 37,014: the 4-stream loop twice, the remainder loop, the scalar tail."""
    K = _K()
    g = torch.Generator().manual_seed(elems)
    a = torch.rand(offset + B * elems, generator=g).cuda()[offset:].view(B, elems)
    b = torch.rand(offset + B * elems, generator=g).cuda()[offset:].view(B, elems)
    assert a.data_ptr() % 16 == 4 * offset and b.data_ptr() % 16 == 4 * offset
    got = K.mse_per_image(a, b).cpu().double()
    want = ((a.cpu().double() - b.cpu().double()) ** 2).mean(1)
    paths = set()
    for i in range(B):
        aligned = (a.data_ptr() + 4 * i * elems) % 16 == 0
        depth = _mse_depth(elems, aligned)
        bound = 2 * (depth + 3) * U
        rel = abs(float(got[i] - want[i])) / float(want[i])
        print(f"elems {elems} image {i}: {'aligned' if aligned else 'unaligned'}, depth {depth}, relative error {rel:.2e}, bound {bound:.2e}")
        assert rel <= bound
        paths.add(aligned)
    if elems == 4099:
        assert paths == {True, False}
    if offset:
        assert paths == {False}
    if elems == 4 * (2 * 4096 + 1024 + 37) + 2:
        assert _mse_depth(elems, True) == 2 + 2 + 4 + 1 + 10   # two 4-stream iterations, two of the remainder loop (1024 + 37 float4s)


# -------------------------------------------------------------------------------------------------------------------- rate kernels
SCALE_BOUND, LIK_BOUND = 0.11, 1e-9
SQRT2 = math.sqrt(2.0)


def _gauss_terms(q, par, mode, dtype, scale_bound=SCALE_BOUND, lik_bound=LIK_BOUND):
    """-log(max(P, bound)) per element [B, C, hw], evaluated in `dtype` by torch on the CPU, from the formulas of basic_hip.h section 4:
    mode 0: par = scales, zero mean, v = |q|, P = Phi((.5 - v) / s) - Phi((-.5 - v) / s) with Phi(t) = .5 erfc(-t / sqrt 2);
    mode 1: par = (mean, scale) pairs, P = cdf(q + .5) - cdf(q - .5), cdf(x) = .5 (1 + erf((x - mu) / (s sqrt 2)));
    mode 2: the same density at the rounded residual v = rint(q - mu): cdf0(v + .5) - cdf0(v - .5).
    s = max(scale, scale_bound) everywhere."""
    q, par = q.to(dtype), par.to(dtype)
    B, C, hw = q.shape
    half = torch.tensor(0.5, dtype=dtype)
    if mode == 0:
        s = torch.clamp(par, min=scale_bound)
        v = q.abs()
        phi = lambda t: half * torch.erfc(-t / SQRT2)
        p = phi((half - v) / s) - phi((-half - v) / s)
    else:
        pr = par.reshape(B, C, 2, hw)
        mu, s = pr[:, :, 0], torch.clamp(pr[:, :, 1], min=scale_bound)
        cdf = lambda x: half * (1 + torch.erf(x / (s * SQRT2)))
        if mode == 2:
            v = torch.round(q - mu)
            p = cdf(v + half) - cdf(v - half)
        else:
            p = cdf(q + half - mu) - cdf(q - half - mu)
    return -torch.log(torch.clamp(p, min=lik_bound))


def _gauss_body(mode, B, C, hw, seed):
    """Body inputs: s log-uniform in [0.05, 8] (a fifth of it below the scale bound), |q - mu| <= 2.5 max(s, bound)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.exp(torch.rand(B, C, hw, generator=g) * (math.log(8) - math.log(0.05)) + math.log(0.05))
    se = torch.clamp(s, min=SCALE_BOUND)
    u = torch.rand(B, C, hw, generator=g) * 2 - 1
    if mode == 0:
        return torch.trunc(u * 2.5 * se), s                                      # integers with |q| <= 2.5 s
    if mode == 1:
        q = torch.randint(-20, 21, (B, C, hw), generator=g).float()              # the quantised latent
        mu = q + u * 2.5 * se
    else:
        mu = torch.randn(B, C, hw, generator=g) * 3
        q = mu + u * 2.5 * se                                                    # the unquantised latent
    return q, torch.stack([mu, s], 2).reshape(B, 2 * C, hw)


def _sum_bound(elems, block=256, levels=8):
    """Relative rounding bound of a per-image sum of same-signed terms: a thread's chain, the LDS tree, 3 roundings, doubled."""
    return 2 * (-(-elems // block) + levels + 3) * U


_RATE_LINES = []


def _check_rate(name, got, t32, t64, mutants):
    """got [B] from the kernel; t32, t64 [B, ...] the per-element terms in fp32 / fp64; mutants: name -> fp64 terms of a wrong kernel.
    Per image: budget = 4 * sum |t32 - t64| (the formula's own fp32 error, times 4 for a device libm that differs from the host's by a
    few ulp) + the summation bound; the budget stays below 1e-4 of the value, the kernel within it, every mutant outside it."""
    B = got.shape[0]
    want = t64.reshape(B, -1).sum(1)
    budget = 4 * (t32.double() - t64).abs().reshape(B, -1).sum(1) + _sum_bound(t64[0].numel()) * t64.abs().reshape(B, -1).sum(1)
    dev = (got.cpu().double() - want).abs()
    line = (f"{name}: value {want.tolist()}, budget / value {[f'{v:.2e}' for v in (budget / want).tolist()]}, "
            f"kernel deviation / value {[f'{v:.2e}' for v in (dev / want).tolist()]}")
    for mname, tm in mutants.items():
        dm = (tm.reshape(B, -1).sum(1) - want).abs()
        line += f", {mname} / value {[f'{v:.2e}' for v in (dm / want).tolist()]}"
        assert bool((dm > budget).all()), f"{name}: the budget would let '{mname}' pass"
    print(line)
    _RATE_LINES.append(line)
    assert bool((budget < 1e-4 * want).all())
    assert bool((dev <= budget).all())


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,C,hw", [(3, 5, 21), (3, 7, 300)])
def test_gauss_nll_body_vs_fp64(mode, B, C, hw):
    K = _K()
    q, par = _gauss_body(mode, B, C, hw, 100 * mode + hw)
    arg = {0: False, 1: True, 2: "round_residual"}[mode]
    got = K.gauss_nll_per_image(q.cuda(), par.cuda(), arg, SCALE_BOUND, LIK_BOUND)
    t32, t64 = _gauss_terms(q, par, mode, torch.float32), _gauss_terms(q, par, mode, torch.float64)
    mutants = {"one position on": _gauss_terms(q, torch.roll(par, 1, dims=2), mode, torch.float64)}
    if mode:   # (mean, scale) pairs taken as (scale, mean)
        mutants["mean and scale swapped"] = _gauss_terms(q, par.reshape(B, C, 2, hw).flip(2).reshape(B, 2 * C, hw), mode, torch.float64)
    if mode == 1:   # (modes 0 and 2 take the density at an integer, and |q - mu| <= 2.5 s leaves the integer 0 below the scale bound, whose
        # probability is 1 to five digits with or without the bound: test_gauss_nll_tails sees their bound)
        mutants["no scale bound"] = _gauss_terms(q, par, mode, torch.float64, scale_bound=1e-30)
    _check_rate(f"gauss_nll mode {mode} ({B}, {C}, {hw})", got, t32, t64, mutants)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gauss_nll_tails(mode):
    """A few crafted elements per image: far in the tail the fp64 probability is below bound / 100, so the clamp decides in both
    precisions and the element costs -log(bound); the others have a probability above 0.01 (far above 100 x bound), where it does
    not.  Modes 0 and 2 also have two elements at 2.8e-6 that only the scale bound keeps off the clamp.  (The erf form loses all relative accuracy in the tail: such elements are kept out of the body cases.)"""
    K = _K()
    B, C, hw = 2, 3, 4
    s = torch.tensor([0.05, 0.11, 0.5, 1.0, 2.0, 8.0]).repeat(B * C * hw // 6).reshape(B, C, hw)
    se = torch.clamp(s, min=SCALE_BOUND)
    far = torch.zeros(B, C, hw, dtype=torch.bool)
    far[0, :, ::2] = True
    far[1, 1, :3] = True
    sign = torch.where(torch.arange(hw) % 2 == 0, 1.0, -1.0).reshape(1, 1, hw)
    mu = torch.zeros(B, C, hw) if mode == 0 else (torch.arange(B * C * hw).reshape(B, C, hw).float() % 5 - 2) * 0.3
    dist = torch.where(far, torch.ceil(40 * se) + 1, torch.zeros_like(se)) * sign   # whole numbers: 40 sigma or more away, or none
    q = mu + dist if mode == 2 else dist + torch.round(mu)
    edge = torch.zeros(B, C, hw, dtype=torch.bool)
    if mode != 1:   # the scale bound at work: s = 0.05 counts as 0.11, where the integer +/-1 has probability 2.8e-6 (without it: 7.6e-24, clamped)
        edge[1, 0, :2] = True
        s[1, 0, :2], q[1, 0, :2] = 0.05, mu[1, 0, :2] + torch.tensor([1.0, -1.0])
    par = s if mode == 0 else torch.stack([mu, s], 2).reshape(B, 2 * C, hw)
    arg = {0: False, 1: True, 2: "round_residual"}[mode]
    t64 = _gauss_terms(q, par, mode, torch.float64)
    p64 = torch.exp(-_gauss_terms(q, par, mode, torch.float64, lik_bound=1e-300))
    assert bool((p64[far] < LIK_BOUND / 100).all()) and bool((p64[~far & ~edge] > 0.01).all()) and bool((p64[edge] > 100 * LIK_BOUND).all())
    assert bool((t64[far] == -math.log(LIK_BOUND)).all())
    got = K.gauss_nll_per_image(q.cuda(), par.cuda(), arg, SCALE_BOUND, LIK_BOUND).cpu().double()
    t32 = _gauss_terms(q, par, mode, torch.float32)
    near64 = torch.where(far, torch.zeros_like(t64), t64).reshape(B, -1).sum(1)
    near_err = 4 * torch.where(far, torch.zeros_like(t64), (t32.double() - t64).abs()).reshape(B, -1).sum(1)
    want = far.reshape(B, -1).sum(1) * -math.log(LIK_BOUND) + near64
    tol = near_err + (_sum_bound(C * hw) + 2 * U) * want   # (2 U: the bound as a float, its logarithm)
    if mode == 2:   # the erf form takes 2.8e-6 as the difference of two values near 1, each good to a few ulp of 1: p within 2^-21
        tol[1] += float(-torch.log(1 - 2.0 ** -21 / p64[edge]).sum())
    print(f"gauss_nll tails mode {mode}: clamped {far.reshape(B, -1).sum(1).tolist()}, value {want.tolist()}, kernel {got.tolist()}, tolerance {tol.tolist()}")
    assert bool(((got - want).abs() <= tol).all())
    if mode != 1:
        unbounded = _gauss_terms(q, par, mode, torch.float64, scale_bound=1e-30).reshape(B, -1).sum(1)
        assert float((unbounded - want).abs()[1]) > 10 * float(tol[1]), "the tolerance would let a kernel without the scale bound pass"


def _eb_coef(C, seed, steep=1.0):
    """coef [C][58]: softplus(M0 [3x1]) b0 [3] tanh(f0) [3] | three times softplus(M [3x3], row-major) b [3] tanh(f) [3] |
    softplus(M4 [1x3]) b4 [1]."""
    g = torch.Generator().manual_seed(seed)
    sp = lambda *shape: torch.nn.functional.softplus(torch.randn(*shape, generator=g) * 0.3 - 0.5)
    parts = [sp(C, 3) * steep, torch.rand(C, 3, generator=g) - 0.5, torch.tanh(torch.randn(C, 3, generator=g))]
    for _ in range(3):
        parts += [sp(C, 9), torch.rand(C, 3, generator=g) - 0.5, torch.tanh(torch.randn(C, 3, generator=g))]
    parts += [sp(C, 3), torch.rand(C, 1, generator=g) - 0.5]
    coef = torch.cat(parts, 1).contiguous()
    assert coef.shape == (C, 58)
    return coef


def _eb_terms(z, coef, dtype, lik_bound=LIK_BOUND):
    """EntropyBottleneck likelihood per element [B, C, hw] in `dtype`: logits(v) through the 1-3-3-3-3-1 network of the element's
    channel (h = M h + b; h += f * tanh(h) after all layers but the last), P = |sigmoid(sg * upper) - sigmoid(sg * lower)| with
    lower / upper = logits(z -/+ .5), sg = -sign(lower + upper)."""
    z, k = z.to(dtype), coef.to(dtype)
    C = k.shape[0]

    def logits(v):   # [B, C, hw]
        h = k[:, 0:3].reshape(1, C, 3, 1) * v.unsqueeze(2) + k[:, 3:6].reshape(1, C, 3, 1)
        h = h + k[:, 6:9].reshape(1, C, 3, 1) * torch.tanh(h)
        o = 9
        for _ in range(3):
            m = k[:, o: o + 9].reshape(1, C, 3, 3, 1)
            h = (m * h.unsqueeze(2)).sum(3) + k[:, o + 9: o + 12].reshape(1, C, 3, 1)
            h = h + k[:, o + 12: o + 15].reshape(1, C, 3, 1) * torch.tanh(h)
            o += 15
        return (k[:, o: o + 3].reshape(1, C, 3, 1) * h).sum(2) + k[:, o + 3].reshape(1, C, 1)

    lower, upper = logits(z - 0.5), logits(z + 0.5)
    sg = -torch.sign(lower + upper)
    p = (torch.sigmoid(sg * upper) - torch.sigmoid(sg * lower)).abs()
    return -torch.log(torch.clamp(p, min=lik_bound))


@pytest.mark.parametrize("B,C,hw", [(3, 5, 21), (3, 7, 300)])
def test_eb_nll_body_vs_fp64(B, C, hw):
    K = _K()
    g = torch.Generator().manual_seed(hw)
    coef = _eb_coef(C, 11)
    z = torch.randint(-4, 5, (B, C, hw), generator=g).float()
    got = K.eb_nll_per_image(z.cuda(), coef.cuda(), LIK_BOUND)
    t32, t64 = _eb_terms(z, coef, torch.float32), _eb_terms(z, coef, torch.float64)
    mutants = {"next channel's network": _eb_terms(z, torch.roll(coef, 1, dims=0), torch.float64),
               "one position on": _eb_terms(torch.roll(z.reshape(B, -1), 1, dims=1).reshape(B, C, hw), coef, torch.float64)}
    _check_rate(f"eb_nll ({B}, {C}, {hw})", got, t32, t64, mutants)


def test_eb_nll_tails():
    """A steep first layer: at |z| = 3 the fp64 probability is below bound / 100 and the element costs -log(bound); at z = 0 it is
    above 0.1."""
    K = _K()
    B, C, hw = 2, 3, 4
    coef = _eb_coef(C, 12, steep=60.0)
    z = torch.zeros(B, C, hw)
    far = torch.zeros(B, C, hw, dtype=torch.bool)
    far[0, :, ::2] = True
    far[1, 2, 1:] = True
    z[far] = 3.0
    z[0, 1] *= -1
    t64 = _eb_terms(z, coef, torch.float64)
    p64 = torch.exp(-_eb_terms(z, coef, torch.float64, lik_bound=1e-300))
    assert bool((p64[far] < LIK_BOUND / 100).all()) and bool((p64[~far] > 0.1).all())
    got = K.eb_nll_per_image(z.cuda(), coef.cuda(), LIK_BOUND).cpu().double()
    t32 = _eb_terms(z, coef, torch.float32)
    near64 = torch.where(far, torch.zeros_like(t64), t64).reshape(B, -1).sum(1)
    near_err = 4 * torch.where(far, torch.zeros_like(t64), (t32.double() - t64).abs()).reshape(B, -1).sum(1)
    want = far.reshape(B, -1).sum(1) * -math.log(LIK_BOUND) + near64
    tol = near_err + (_sum_bound(C * hw) + 2 * U) * want
    print(f"eb_nll tails: clamped {far.reshape(B, -1).sum(1).tolist()}, value {want.tolist()}, kernel {got.tolist()}, tolerance {tol.tolist()}")
    assert bool(((got - want).abs() <= tol).all())
