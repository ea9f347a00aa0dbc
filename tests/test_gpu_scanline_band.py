"""The band encode schedule of the batched scan-line kernel (csrc/scanline.hip: the wavefront's W + s * (H - 1) steps, but an image's
rows share W // s + 1 column slots of one MFMA tile, so any batch and any height is served, in successive launches where one does
not hold the batch) against the per-step path of the same coder.  The schedule changes addressing, not arithmetic: symbols, table
rows, the coded latent (float bits) and the bytes must be EQUAL -- no tolerance anywhere -- and ScanlinePlan.last_kernel() must
say that the band ran."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0x7FC0BEEF   # NaN payload of the guard bands
BAND = 4096


def _coder(kind, C):
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import (GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder,
                                                                            TopoGroupDynamicMaskConv2dContextModel as Ctx)
    if kind.startswith("ctxmodel"):   # "ctxmodel", or "ctxmodel-k3" for a 3x3 context window
        ks = int(kind.split("-k")[1]) if "-k" in kind else 5
        c = Coder(in_channels=C, default_topo_group_method="scanline", topo_group_context_model=Ctx(in_channels=C, out_channels=2 * C, kernel_size=ks))
    else:   # "merger": layers that are not whole 32-row tiles
        c = Coder(in_channels=C, default_topo_group_method="scanline")
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for p in c.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.02))
    c = c.eval().cuda()
    c.update_state()
    return c


_CODERS = {}


def _shared_coder(kind, C):
    """One coder per configuration for the whole module (its weights are seeded: every test sees the same layers)."""
    if (kind, C) not in _CODERS:
        _CODERS[kind, C] = _coder(kind, C)
    c = _CODERS[kind, C]
    c.use_persistent_scanline = True
    c.scanline_encode_schedule = "auto"
    return c


def _inputs(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B, C, H, W, generator=g) * 3).cuda()
    prior = torch.stack([torch.randn(B, C, H, W, generator=g), torch.rand(B, C, H, W, generator=g) * 3 + 0.1], 2).reshape(B, 2 * C, H, W).cuda()
    return y, prior


def _plan_of(coder, C):
    """The coder's ScanlinePlan (built by a tiny raster call if need be)."""
    y, prior = _inputs(1, C, 2, 2, 5)
    coder.use_persistent_scanline = True
    coder.scanline_encode_schedule = "raster"
    coder._run_encode(y, prior)
    sl = coder._layers["scanline"][0]
    sl.check()
    coder.scanline_encode_schedule = "auto"
    return sl


def _check_band_equals_per_step(kind, B, H, W, seed):
    C = 192
    coder = _shared_coder(kind, C)
    y, prior = _inputs(B, C, H, W, seed)
    coder.use_persistent_scanline = False
    s0, i0, y0, plan = coder._run_encode(y, prior)
    data0 = coder.encode(y, prior=prior)
    coder.use_persistent_scanline = True
    coder.scanline_encode_schedule = "band"
    s1, i1, y1, _ = coder._run_encode(y, prior)   # (a call the band does not fit raises: no case here may)
    sl = coder._layers["scanline"][0]
    sl.check()
    assert sl.band_max(H, W) >= 1
    assert sl.last_kernel() == "band", sl.last_kernel()
    ms, mi = int((s0 != s1).sum()), int((i0 != i1).sum())
    my = int((y0.view(torch.int32) != y1.view(torch.int32)).sum())
    print(f"{kind} B={B} {H}x{W} seed {seed}: band_max {sl.band_max(H, W)}, symbol diffs {ms}, index diffs {mi}, ybuf bit diffs {my} of {s0.numel()}")
    assert ms == 0 and mi == 0 and my == 0
    data1 = coder.encode(y, prior=prior)
    assert sl.last_kernel() == "band", sl.last_kernel()
    sl.check()
    assert data1 == data0
    yhat = coder.decode(data1, prior=prior)
    sl.check()
    assert torch.equal(yhat.view(torch.int32), y1.view(torch.int32))


# 1x16x16: slots wrap three times; 1x9x4, 1x5x1: two slots, one slot; 1x1x6: fewer rows than slots; 6x16x16: one tile with holes;
# 7x16x16: a second tile with one image; 3x32x48, 8x32x48: B * H > 64; 1x70x24, 1x100x7: H > 64; 48x16x16: every tile a launch may
# hold; ctxmodel-k3: s = 3
@pytest.mark.parametrize("kind,B,H,W", [("ctxmodel", 1, 16, 16), ("ctxmodel", 1, 9, 4), ("ctxmodel", 1, 5, 1), ("ctxmodel", 1, 1, 6),
                                        ("ctxmodel", 1, 1, 1), ("ctxmodel", 6, 16, 16), ("ctxmodel", 7, 16, 16), ("ctxmodel", 3, 32, 48),
                                        ("ctxmodel", 8, 32, 48), ("ctxmodel", 1, 70, 24), ("ctxmodel", 1, 100, 7), ("ctxmodel", 48, 16, 16),
                                        ("ctxmodel-k3", 3, 16, 16)])
def test_band_encode_equals_per_step_path(kind, B, H, W):
    _check_band_equals_per_step(kind, B, H, W, B * 100 + H * 10 + W)


def test_band_more_than_one_launch():
    """Three images more than one launch holds: the call is cut into two launches over whole images."""
    sl = _plan_of(_shared_coder("ctxmodel", 192), 192)
    per_launch = sl.band_max(4, 4)
    assert per_launch >= 1
    _check_band_equals_per_step("ctxmodel", per_launch + 3, 4, 4, 4242)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_band_seeds(seed):
    """Five different inputs of a batch the wavefront refuses (B * H = 96), each coded once."""
    _check_band_equals_per_step("ctxmodel", 3, 32, 48, 9000 + seed)


@pytest.mark.parametrize("kind,C,B,H,W", [("merger", 32, 1, 5, 5), ("ctxmodel", 192, 1, 3, 130)])
def test_band_refused_on_the_host(kind, C, B, H, W):
    """Layers that are not whole 32-row tiles, or a latent so wide that an image's slots exceed one column tile (130 // 4 + 1 = 33):
    band_max says so and a forced call fails before any launch."""
    coder = _shared_coder(kind, C)
    sl = _plan_of(coder, C)
    before = sl.last_kernel()
    assert before in ("generic", "pipelined", "batched")
    assert sl.band_max(H, W) == 0
    y, prior = _inputs(B, C, H, W, 6)
    sl.set_encode_schedule("band")
    try:
        with pytest.raises((RuntimeError, ValueError), match="does not fit"):
            sl.encode(y, prior, coder._scale_table_dev)
    finally:
        sl.set_encode_schedule("auto")
    assert sl.last_kernel() == before   # no launch was made


@pytest.mark.parametrize("B,H,W", [(7, 16, 16), (None, 4, 4)])
def test_band_guard_bands(B, H, W):
    """sym, idx and ybuf as views into sentinel-filled buffers: the band's launches write all of each view and nothing else
    (B None: three images more than one launch holds)."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    C = 192
    coder = _shared_coder("ctxmodel", C)
    sl = _plan_of(coder, C)
    if B is None:
        B = sl.band_max(H, W) + 3
    y, prior = _inputs(B, C, H, W, 77 + B)
    coder.use_persistent_scanline = False
    s0, i0, y0, _ = coder._run_encode(y, prior)
    coder.use_persistent_scanline = True
    table = coder._scale_table_dev.to(device="cuda", dtype=torch.float32).contiguous()
    n = B * H * W * C
    off = 64
    bufs = [torch.full((off + n + BAND,), GUARD, dtype=torch.int32, device="cuda") for _ in range(3)]
    for b in bufs:
        b[off: off + n] = 0x7FC00001   # (a NaN as float, no symbol or table row as integer)
    sym, idx, ybuf = (b[off: off + n] for b in bufs)
    sl.set_encode_schedule("band")
    try:
        _lib.check(_lib.lib().basic_scanline_encode_dev(sl._h, y.data_ptr(), prior.data_ptr(), B, H, W, table.data_ptr(), table.numel(),
                                                        sym.data_ptr(), idx.data_ptr(), ybuf.data_ptr(), K._stream()))
        sl.check()
    finally:
        sl.set_encode_schedule("auto")
    assert sl.last_kernel() == "band"
    for name, b in zip(("sym", "idx", "ybuf"), bufs):
        h = b.cpu()
        assert bool((h[:off] == GUARD).all()) and bool((h[off + n:] == GUARD).all()), f"the launch wrote outside {name}"
    assert torch.equal(sym.view(B, -1), s0) and torch.equal(idx.view(B, -1), i0)
    assert torch.equal(ybuf.view(B, C, H, W), y0.view(torch.int32))


def test_band_leaves_auto_alone():
    """auto: one Kodak-shaped image still takes the wavefront; three of them (which the wavefront refuses) code the per-step
    path's integers and bytes whichever kernel auto picks."""
    C = 192
    coder = _shared_coder("ctxmodel", C)
    y, prior = _inputs(1, C, 32, 48, 31)
    coder._run_encode(y, prior)
    sl = coder._layers["scanline"][0]
    sl.check()
    assert sl.last_kernel() == "wavefront", sl.last_kernel()
    y, prior = _inputs(3, C, 32, 48, 32)
    coder.use_persistent_scanline = False
    s0, i0, y0, _ = coder._run_encode(y, prior)
    data0 = coder.encode(y, prior=prior)
    coder.use_persistent_scanline = True
    coder.scanline_encode_schedule = "auto"
    s1, i1, y1, _ = coder._run_encode(y, prior)
    sl.check()
    print("auto, 3x32x48:", sl.last_kernel())
    assert torch.equal(s0, s1) and torch.equal(i0, i1) and torch.equal(y0.view(torch.int32), y1.view(torch.int32))
    assert coder.encode(y, prior=prior) == data0


@pytest.mark.parametrize("level", [0, 7])
def test_band_codec_level(level):
    """BaSIC on five 256 x 256 images: the raster and the band schedule write the same bytes, which decompress to the same images."""
    from cbench_basic_amd.presets import basic_codec, seed_synthetic_weights
    codec = seed_synthetic_weights(basic_codec(), seed=0).eval().cuda()
    codec.update_state()
    codec.set_complex_level(level)
    yc = codec.entropy_coder.latent_node_entropy_coders["y"]
    x = torch.rand(5, 3, 256, 256, generator=torch.Generator().manual_seed(11)).cuda()
    yc.scanline_encode_schedule = "raster"
    raster = codec.compress(x)
    sl = yc._layers["scanline"][0]
    sl.check()
    assert sl.last_kernel() in ("generic", "pipelined", "batched")
    x_raster = codec.decompress(raster)
    yc.scanline_encode_schedule = "band"
    band = codec.compress(x)
    sl = yc._layers["scanline"][0]
    sl.check()
    assert sl.last_kernel() == "band", sl.last_kernel()
    assert band == raster
    x_band = codec.decompress(band)
    assert torch.equal(x_raster, x_band)
