"""GPU: every launch path of csrc/conv.hip against an fp64 CPU reference of the same layer, exactly where the data allow it.

Launch paths (basic_conv_forward_dev / choose_launches) and the PATHS cases below that reach them:

  path                                          selected by                                               cases
  conv_tap_mfma_kernel MT 1..6, 4 waves         ceil(cout / 32) accumulator tiles per launch              mt1_k3, mt2_k5, mt3_k4, mt5_k2, mt6_k5,
                                                                                                           mt4_k3_igdn
  conv_tap_mfma_kernel MT 4, 8 waves            plan_waves: GDN, MT 4 and more than 9 taps                mt4_k5_gdn_8w, table16_mt4
  runtime tap table (KH = 0)                    a tap grid other than 5x5 / 3x3 / 3x2 / 2x3 / 2x2         table16_mt1..6 (4x4), table1_mt1..6 (1x1),
                                                (the 7..9-tap table variant is unreachable: only 3x3       mt3_k4, tr_k3s2 phases (1x1, 1x2, 2x1)
                                                grids have 7..9 taps at k <= 5, stride <= 2)
  fused column phases (KWB > 0), MT 1..4        k5 s2 p2 transposed, even output width, 8-byte aligned    fused_mt1 .. fused_mt4
                                                output, no split-bf16 pack                                (2 launches instead of 4)
  four-phase fallback                           odd output width, output rows not 8-byte aligned, or      fourphase_op0 (odd width), fourphase_dbg512,
                                                BASIC_CONV_DEBUG bit 512                                  the misaligned out= runs of the guard tests
  bias-only phases (ntaps == 0)                 a phase no tap reaches (k1 s2 transposed)                 bias_only_k1s2
  32-channel slices over gridDim.y              cout >= 64, no GDN, fewer than 384 position blocks (or    slices_* (ragged last slice), test_chunks_and_slices
                                                bit 4; bit 8 forbids them)
  chunked cout > 192                            balanced chunks rounded to whole M-tiles                  test_chunks_and_slices (193, 200, 257, 400)
  conv5x5_cin4_gdn_persistent_kernel<true>      5x5 GDN conv, 128 channels, cin 1..3                      first_cin1, first_cin3
  conv5x5_cin4_gdn_persistent_kernel<false>     ... cin 4                                                 first_cin4
  deconv5s2_cout3_kernel                        k5 s2 p2 op1 transposed, cout <= 3, no GDN, input not     cout3_plain, cout3_plain_ragged (in_w % 4 != 0),
                                                16-byte aligned or in_w % 4 != 0                          guard runs at input offsets 1 and 2
  deconv5s2_cout3_dma_kernel<1>                 ... in_w % 4 == 0, 16-byte aligned input, in_h < 64       cout3_dma, cout3_dma_ragged
  deconv5s2_cout3_dma_kernel<2>                 ... and in_h >= 64 (two strips per lane)                  cout3_dma2, cout3_dma2_ragged
  conv_split_bf16_kernel<3,3,2> and <2,3,2>     fused IGDN launch, 97..128 channels, cin % 16 == 0 (the   split_* and SPLIT_CASES (both instantiations
                                                two row phases of one layer)                              run in every such layer)

Checks:
  * exact integers (|x| <= 15, |w| <= 7, |b| <= 64, every partial sum < 2^20): products and sums are exact in any order
    and in one bf16 piece, so linear and ReLU outputs equal the fp64 reference bit for bit, Leaky ReLU equals fp32 of the
    exact value times 0.01f, and GDN / IGDN with gamma = 0 and beta in {1/4, 1, 4, 16} per channel is the linear output
    times a power of two, within the one rsq / sqrt rounding (2^-21 relative);
  * randn data: |got - ref64| <= TAU * A element-wise, A = conv(|x|, |w|) + |b| in fp64 (GDN / IGDN with gamma = 0,
    beta = 1); with a real gamma, that bound propagated to first order through the normalisation;
  * guard bands: inputs as views into NaN-filled buffers at 64 / 1 / 2 floats offset, outputs as views into buffers whose
    bands hold a NaN of a fixed payload: every output element written, the bands bitwise unchanged;
  * the launch count of ConvPlan.launches() where the path changes it, and for split-bf16 a result that differs from the
    fp32 kernel's (BASIC_CONV_F32=1) on random data.
"""
import pytest
import torch

# the fp64 reference, the data, the bounds and the guard-band views: shared with test_gpu_conv_aspect.py
from conv_ref import (RMS_FLOOR, SPLIT_RMS_FACTOR, Case, _bound_a, _check_bound, _check_exact, _gdn_bound, _guarded_run,
                      _layer, _linear64, _out_offsets, _plan, _run, _seed, _set_env)

pytestmark = pytest.mark.gpu

# A representative layer per launch path; `launches` is ConvPlan.launches() under `debug` (BASIC_CONV_DEBUG).
PATHS = {
    "mt1_k3": Case(37, 20, 3, 1, 1, 0, False, "relu", 2, 7, 9, "", 1),
    "mt2_k5": Case(24, 50, 5, 2, 2, 0, False, "leaky", 1, 13, 11, "", 1),
    "mt3_k4": Case(40, 96, 4, 2, 1, 0, False, "none", 2, 9, 8, "8", 1),
    "mt4_k5_gdn_8w": Case(48, 128, 5, 2, 2, 0, False, "gdn", 2, 18, 24, "", 1),
    "mt4_k3_igdn": Case(64, 112, 3, 1, 1, 0, False, "igdn", 1, 10, 7, "", 1),
    "mt5_k2": Case(33, 150, 2, 1, 0, 0, False, "relu", 1, 8, 9, "8", 1),
    "mt6_k5": Case(72, 192, 5, 1, 2, 0, False, "gdn", 1, 9, 10, "", 1),
    "tr_k3s2": Case(24, 64, 3, 2, 1, 1, True, "relu", 2, 6, 5, "8", 4),
    "bias_only_k1s2": Case(24, 40, 1, 2, 0, 1, True, "leaky", 2, 5, 6, "", 4),
    "fused_mt1": Case(40, 30, 5, 2, 2, 1, True, "none", 2, 6, 7, "", 2),
    "fused_mt2": Case(36, 64, 5, 2, 2, 1, True, "relu", 1, 7, 5, "8", 2),
    "fused_mt3": Case(20, 90, 5, 2, 2, 1, True, "igdn", 1, 5, 6, "", 2),
    "fused_mt4_fp32": Case(72, 128, 5, 2, 2, 1, True, "igdn", 1, 6, 6, "", 2),   # cin % 16 != 0: no split pack
    "fourphase_op0": Case(40, 96, 5, 2, 2, 0, True, "igdn", 1, 6, 5, "", 4),     # odd output width
    "fourphase_dbg512": Case(48, 128, 5, 2, 2, 1, True, "leaky", 1, 5, 6, "520", 4),
    "slices_fwd_100": Case(40, 100, 3, 1, 1, 0, False, "leaky", 1, 6, 7, "4", 1),
    "slices_tr_70": Case(24, 70, 5, 2, 2, 1, True, "relu", 1, 5, 4, "4", 2),
    "slices_tr_190": Case(16, 190, 5, 2, 2, 1, True, "none", 1, 4, 3, "4", 2),
    "first_cin1": Case(1, 128, 5, 2, 2, 0, False, "gdn", 2, 24, 30, "", 1),
    "first_cin3": Case(3, 128, 5, 2, 2, 0, False, "gdn", 1, 40, 36, "", 1),
    "first_cin4": Case(4, 128, 5, 1, 2, 0, False, "gdn", 1, 21, 26, "", 1),
    "cout3_plain": Case(40, 3, 5, 2, 2, 1, True, "leaky", 2, 9, 13, "", 1),
    "cout3_dma": Case(24, 2, 5, 2, 2, 1, True, "relu", 1, 20, 16, "", 1),
    "cout3_dma2": Case(8, 1, 5, 2, 2, 1, True, "none", 1, 66, 12, "", 1),
    # ragged last channel stage, partial row and column tiles, every output channel
    "cout3_dma_ragged": Case(5, 3, 5, 2, 2, 1, True, "leaky", 1, 17, 68, "", 1),
    # ... odd height (a lane's second strip out of range), 18 workgroups (xcd_tile remaps 16 and passes 2 through)
    "cout3_dma2_ragged": Case(3, 3, 5, 2, 2, 1, True, "relu", 3, 65, 68, "", 1),
    "cout3_plain_ragged": Case(9, 2, 5, 2, 2, 1, True, "none", 1, 17, 66, "", 1),   # 2 x 2 tiles, ragged second stage
    "split_cin192": Case(192, 128, 5, 2, 2, 1, True, "igdn", 1, 8, 12, "", 2),
    "split_ragged": Case(48, 100, 5, 2, 2, 1, True, "igdn", 3, 3, 5, "", 2),
}
# runtime tap table (KH = 0) at every MT: 16 taps (k4 conv; MT 4 takes 8 waves) and 1 tap (k1 conv).  The table variant for
# 7..9 taps cannot be reached: with k <= 5 and stride <= 2 the only grid of 7..9 taps is 3x3, which is unrolled.
for _mt, _act in zip(range(1, 7), ("none", "relu", "leaky", "gdn", "none", "leaky")):
    PATHS[f"table16_mt{_mt}"] = Case(19 + _mt, 32 * _mt - 5, 4, 2, 1, 0, False, _act, 1, 9, 10, "8", 1)
    PATHS[f"table1_mt{_mt}"] = Case(30 - _mt, 32 * _mt - 3, 1, 1, 0, 0, False, _act, 2, 5, 6, "8", 1)
del _mt, _act
SPLIT_PATHS = ("split_cin192", "split_ragged")


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 2 + 3: every path, exact integers and the per-element fp64 bound


@pytest.mark.parametrize("name", list(PATHS))
def test_path_exact_integers(name, monkeypatch):
    c = PATHS[name]
    x, w, b, gamma, beta = _layer(c, True, _seed(name, "int"))
    plan = _plan(c, w, b, gamma, beta)
    _set_env(monkeypatch, c.debug)
    assert plan.launches(c.B, c.H, c.W) == c.launches
    got = _run(plan, x, monkeypatch, c.debug)
    _check_exact(c, got, _linear64(c, x, w, b), beta)


@pytest.mark.parametrize("name", list(PATHS))
def test_path_randn_bound(name, monkeypatch):
    c = PATHS[name]
    x, w, b, gamma, beta = _layer(c, False, _seed(name, "randn"))
    plan = _plan(c, w, b, gamma, beta)
    lin, A = _linear64(c, x, w, b), _bound_a(c, x, w, b)
    got = _run(plan, x, monkeypatch, c.debug)
    r = _check_bound(c, got, lin, A, name)
    if name in SPLIT_PATHS:
        got32 = _run(plan, x, monkeypatch, c.debug, f32=True)
        r32 = _check_bound(c, got32, lin, A, name + " fp32")
        assert not torch.equal(got, got32), "the split-bf16 path did not run"
        rms, rms32 = float(r.pow(2).mean().sqrt()), float(r32.pow(2).mean().sqrt())
        assert rms <= SPLIT_RMS_FACTOR * rms32 + RMS_FLOOR, (rms, rms32)


@pytest.mark.parametrize("name", [n for n, c in PATHS.items() if c.act in ("gdn", "igdn")])
def test_path_gdn_real_gamma(name, monkeypatch):
    c = PATHS[name]
    x, w, b, gamma, beta = _layer(c, False, _seed(name, "gamma"), gamma_kind="real")
    plan = _plan(c, w, b, gamma, beta)
    got = _run(plan, x, monkeypatch, c.debug)
    _gdn_bound(c, got, _linear64(c, x, w, b), _bound_a(c, x, w, b), gamma, beta)


# ---------------------------------------------------------------------------------------------------------------------
# 4: guard bands and alignment

GUARDED = ["mt1_k3", "mt4_k5_gdn_8w", "mt6_k5", "bias_only_k1s2", "fused_mt2", "fused_mt4_fp32", "slices_tr_70",
           "first_cin3", "first_cin4", "cout3_plain", "cout3_dma", "cout3_dma2", "cout3_dma_ragged", "cout3_dma2_ragged",
           "split_cin192", "split_ragged"]


@pytest.mark.parametrize("name", GUARDED)
def test_guard_bands_exact(name, monkeypatch):
    """Integer data through every input / output offset: bit for bit the exact result, bands untouched."""
    c = PATHS[name]
    x, w, b, gamma, beta = _layer(c, True, _seed(name, "int"))
    plan = _plan(c, w, b, gamma, beta)
    lin = _linear64(c, x, w, b)
    for in_off in (64, 1, 2):
        for out_off in _out_offsets(c):
            _check_exact(c, _guarded_run(plan, c, x, in_off, out_off, monkeypatch, c.debug), lin, beta)


@pytest.mark.parametrize("name", GUARDED)
def test_guard_bands_randn(name, monkeypatch):
    """randn data: aligned views give the plain run bit for bit; misaligned inputs (4-byte patch pieces, the plain
    cout <= 3 kernel) meet the fp64 bound, and the plain cout <= 3 kernel gives the LDS-DMA kernels' result bit for
    bit (the same FMA chain per output in all three kernels); a 4-byte misaligned output takes the four-phase
    fallback, which gives the BASIC_CONV_DEBUG=512 run bit for bit."""
    c = PATHS[name]
    x, w, b, gamma, beta = _layer(c, False, _seed(name, "randn"))
    plan = _plan(c, w, b, gamma, beta)
    lin, A = _linear64(c, x, w, b), _bound_a(c, x, w, b)
    plain = _run(plan, x, monkeypatch, c.debug)
    assert torch.equal(_guarded_run(plan, c, x, 64, 64, monkeypatch, c.debug), plain)
    for in_off in (1, 2):
        got = _guarded_run(plan, c, x, in_off, 64, monkeypatch, c.debug)
        _check_bound(c, got, lin, A, f"{name} in+{in_off}")
        if c.cout <= 3:   # the plain kernel: the same FMA chain per output as the LDS-DMA kernels
            assert torch.equal(got, plain), f"{name} in+{in_off}: the plain kernel's result differs from the aligned run's"
    if c.cout > 3:
        got = _guarded_run(plan, c, x, 64, 1, monkeypatch, c.debug)
        _check_bound(c, got, lin, A, f"{name} out+1")
        # the four-phase launches (no split-bf16 variant: the split kernel stores 8-byte pairs)
        dbg = str(int(c.debug or 0) | 512)
        fallback = _run(plan, x, monkeypatch, dbg, f32=True)
        assert torch.equal(got, fallback)
        if c.launches == 2:   # fused (or split-bf16) normally: the fallback sums in another order, so this proves it ran
            assert not torch.equal(plain, fallback)


# ---------------------------------------------------------------------------------------------------------------------
# 5: split-bf16 geometry matrix (k5 s2 p2 op1 transposed + IGDN: g_s layers)

# cin, cout, B, H, W, bias
SPLIT_CASES = [
    (16, 128, 1, 3, 5, True),
    (48, 97, 3, 1, 1, True),
    (112, 100, 1, 1, 7, True),
    (128, 127, 2, 5, 1, True),
    (144, 128, 1, 17, 9, True),
    (192, 97, 1, 8, 64, True),
    (192, 128, 1, 32, 48, True),   # the Kodak latent
    (16, 100, 257, 1, 1, True),    # a tile of 256 images plus one
    (48, 127, 257, 1, 1, True),
    (144, 97, 3, 17, 9, True),
    (128, 100, 3, 3, 5, False),
    (16, 97, 1, 8, 64, True),
    (192, 100, 1, 5, 1, False),
]


def _split_case(sc):
    cin, cout, B, H, W, _ = sc
    return Case(cin, cout, 5, 2, 2, 1, True, "igdn", B, H, W, "", 2)


def _split_id(sc):
    return "cin%d-cout%d-B%d-%dx%d%s" % (sc[:5] + ("" if sc[5] else "-nobias",))


@pytest.mark.parametrize("sc", SPLIT_CASES, ids=_split_id)
def test_split_geometry(sc, monkeypatch):
    c = _split_case(sc)
    # exact integers: bit for bit (times the power-of-two IGDN factor)
    x, w, b, gamma, beta = _layer(c, True, _seed(sc, "int"), bias=sc[5])
    plan = _plan(c, w, b, gamma, beta)
    _set_env(monkeypatch)
    assert plan.launches(c.B, c.H, c.W) == 2
    _check_exact(c, _run(plan, x, monkeypatch), _linear64(c, x, w, b), beta)
    # randn, gamma = 0, beta = 1: the split GEMM alone, per element within TAU * A, RMS within 1.5x the fp32 kernel's
    x, w, b, gamma, beta = _layer(c, False, _seed(sc, "randn"), bias=sc[5])
    plan = _plan(c, w, b, gamma, beta)
    lin, A = _linear64(c, x, w, b), _bound_a(c, x, w, b)
    got = _run(plan, x, monkeypatch)
    got32 = _run(plan, x, monkeypatch, f32=True)
    assert not torch.equal(got, got32), "the split-bf16 path did not run"
    r, r32 = _check_bound(c, got, lin, A, "split"), _check_bound(c, got32, lin, A, "fp32")
    rms, rms32 = float(r.pow(2).mean().sqrt()), float(r32.pow(2).mean().sqrt())
    assert rms <= SPLIT_RMS_FACTOR * rms32 + RMS_FLOOR, (rms, rms32)


@pytest.mark.parametrize("sc", [SPLIT_CASES[1], SPLIT_CASES[2], SPLIT_CASES[9]], ids=_split_id)
def test_split_batch_invariant_ragged(sc, monkeypatch):
    """Image 0 (and image 1) bit for bit the same whether its tile holds 1, 3 or 257 images."""
    c = _split_case(sc)
    Bmax = 257 if c.H * c.W == 1 else 3
    x, w, b, gamma, beta = _layer(c._replace(B=Bmax), False, _seed(sc, "batch"), gamma_kind="real")
    plan = _plan(c, w, b, gamma, beta)
    outs = [_run(plan, x[:n].contiguous(), monkeypatch) for n in sorted({1, 3, Bmax})]
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0])
    assert torch.equal(outs[1][1], outs[-1][1])
    assert torch.equal(outs[-1][-1], _run(plan, x[-1:].contiguous(), monkeypatch)[0])


def test_split_slimmable(monkeypatch):
    """A [192, 192, 5, 5] transposed weight at cin_active = cout_active = 128, gamma / beta given for the slice."""
    c = Case(128, 128, 5, 2, 2, 1, True, "igdn", 2, 6, 10, "", 2)
    g = torch.Generator().manual_seed(11)
    wi = torch.randint(-7, 8, (192, 192, 5, 5), generator=g).float()
    bi = torch.randint(-64, 65, (192,), generator=g).float()
    xi = torch.randint(-15, 16, (2, 128, 6, 10), generator=g).float()
    beta = torch.tensor([0.25, 1.0, 4.0, 16.0])[torch.randint(0, 4, (128,), generator=g)]
    plan = _plan(c, wi, bi, torch.zeros(128, 128), beta, cin_active=128, cout_active=128)
    _set_env(monkeypatch)
    assert plan.launches(2, 6, 10) == 2
    _check_exact(c, _run(plan, xi, monkeypatch), _linear64(c, xi, wi[:128, :128], bi[:128]), beta)
    x = torch.randn(2, 128, 6, 10, generator=g)
    w = torch.randn(192, 192, 5, 5, generator=g) * 0.02
    b = torch.randn(192, generator=g) * 0.1
    plan = _plan(c, w, b, torch.zeros(128, 128), torch.ones(128), cin_active=128, cout_active=128)
    lin, A = _linear64(c, x, w[:128, :128], b[:128]), _bound_a(c, x, w[:128, :128], b[:128])
    got, got32 = _run(plan, x, monkeypatch), _run(plan, x, monkeypatch, f32=True)
    assert not torch.equal(got, got32), "the split-bf16 path did not run"
    r, r32 = _check_bound(c, got, lin, A, "split"), _check_bound(c, got32, lin, A, "fp32")
    assert float(r.pow(2).mean().sqrt()) <= SPLIT_RMS_FACTOR * float(r32.pow(2).mean().sqrt()) + RMS_FLOOR


# ---------------------------------------------------------------------------------------------------------------------
# 6: output-channel chunks above 192 and 32-channel slices


def _expected_launches(c, slices):
    """ConvPlan.launches() restated: balanced chunks of whole M-tiles (or one 32-channel-slice family); a k5 s2 transposed
    conv runs its column phases fused (2 launches) where the chunk has <= 4 M-tiles and the output width is even."""
    if slices:
        mts = [1]
    else:
        n = -(-c.cout // 192)
        per = -(-(-(-c.cout // n)) // 32) * 32
        mts = [-(-min(per, c.cout - co0) // 32) for co0 in range(0, c.cout, per)]
    if not c.tr:
        return len(mts)
    ow = (c.W - 1) * c.s - 2 * c.p + c.k + c.op
    fuse = c.k == 5 and c.s == 2 and c.p == 2 and ow % 2 == 0
    return sum(2 if fuse and mt <= 4 else 4 for mt in mts)


CHUNK_SLICE = [
    # cout > 192: chunks (bit 8) against one slice family (bit 4)
    *[Case(cin, cout, 5, 2, 2, 0, False, act, 1, 9, 10, "", 0)
      for cin, cout, act in ((40, 193, "none"), (24, 200, "relu"), (36, 257, "leaky"), (20, 400, "none"))],
    *[Case(cin, cout, 5, 2, 2, 1, True, act, 1, 5, 4, "", 0)
      for cin, cout, act in ((40, 193, "relu"), (24, 200, "none"), (36, 257, "none"), (20, 400, "leaky"))],
    # 64 <= cout <= 192, not multiples of 32: a ragged last slice
    *[Case(cin, cout, 3, 1, 1, 0, False, "leaky", 2, 5, 6, "", 0) for cin, cout in ((30, 70), (16, 150), (40, 190))],
    *[Case(cin, cout, 5, 2, 2, 1, True, "none", 1, 4, 5, "", 0) for cin, cout in ((30, 100), (16, 150), (24, 190))],
]


@pytest.mark.parametrize("c", CHUNK_SLICE, ids=lambda c: f"{'tr' if c.tr else 'fwd'}-cin{c.cin}-cout{c.cout}-{c.act}")
def test_chunks_and_slices(c, monkeypatch):
    xi, wi, bi, _, _ = _layer(c, True, _seed(tuple(c), "int"))
    x, w, b, _, _ = _layer(c, False, _seed(tuple(c), "randn"))
    plan_i, plan = _plan(c, wi, bi, None, None), _plan(c, w, b, None, None)
    lin_i = _linear64(c, xi, wi, bi)
    lin, A = _linear64(c, x, w, b), _bound_a(c, x, w, b)
    for debug, slices in (("8", False), ("4", True)):
        _set_env(monkeypatch, debug)
        assert plan.launches(c.B, c.H, c.W) == _expected_launches(c, slices)
        _check_exact(c, _run(plan_i, xi, monkeypatch, debug), lin_i, None)
        _check_bound(c, _run(plan, x, monkeypatch, debug), lin, A, f"debug {debug}")
