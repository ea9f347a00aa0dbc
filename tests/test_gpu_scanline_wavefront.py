"""The wavefront encode schedule of the batched scan-line kernel (csrc/scanline.hip: a column of the MFMA tiles is one row of one
image, step t codes column position t - s * r of every row r, W + s * (H - 1) dependent steps instead of H * W) against the
per-step path of the same coder.  The schedule changes addressing, not arithmetic: symbols, table rows, the coded latent (float
bits) and the bytes must be EQUAL -- no tolerance anywhere -- and ScanlinePlan.last_kernel() must say that the wavefront ran."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0x7FC0BEEF   # NaN payload of the guard bands
BAND = 4096


def _coder(kind, C):
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import (GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder,
                                                                            TopoGroupDynamicMaskConv2dContextModel as Ctx)
    if kind.startswith("ctxmodel"):   # "ctxmodel", or "ctxmodel-k3" for a 3x3 context window (the masked-convolution plans stop at 5x5)
        ks = int(kind.split("-k")[1]) if "-k" in kind else 5
        c = Coder(in_channels=C, default_topo_group_method="scanline", topo_group_context_model=Ctx(in_channels=C, out_channels=2 * C, kernel_size=ks))
    elif kind == "merger":
        c = Coder(in_channels=C, default_topo_group_method="scanline")
    elif kind == "merger-expand":
        c = Coder(in_channels=C, default_topo_group_method="scanline", param_merger_expand_bottleneck=True)
    else:
        c = Coder(in_channels=C, use_joint_ar_model_impl=True)
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


def _check_wavefront_equals_per_step(kind, B, H, W, seed):
    C = 192
    coder = _shared_coder(kind, C)
    y, prior = _inputs(B, C, H, W, seed)
    coder.use_persistent_scanline = False
    s0, i0, y0, plan = coder._run_encode(y, prior)
    data0 = coder.encode(y, prior=prior)
    coder.use_persistent_scanline = True
    coder.scanline_encode_schedule = "wavefront"
    s1, i1, y1, _ = coder._run_encode(y, prior)   # (a call the wavefront does not fit raises: no case here may)
    sl = coder._layers["scanline"][0]
    sl.check()
    assert sl.wavefront_max(H, W) >= B
    assert sl.last_kernel() == "wavefront", sl.last_kernel()
    ms, mi = int((s0 != s1).sum()), int((i0 != i1).sum())
    my = int((y0.view(torch.int32) != y1.view(torch.int32)).sum())
    print(f"{kind} B={B} {H}x{W} seed {seed}: symbol diffs {ms}, index diffs {mi}, ybuf bit diffs {my} of {s0.numel()}")
    assert ms == 0 and mi == 0 and my == 0
    data1 = coder.encode(y, prior=prior)
    assert sl.last_kernel() == "wavefront", sl.last_kernel()
    sl.check()
    assert data1 == data0
    yhat = coder.decode(data1, prior=prior)
    sl.check()
    assert torch.equal(yhat.view(torch.int32), y1.view(torch.int32))


@pytest.mark.parametrize("kind,B,H,W", [("ctxmodel", 1, 32, 48), ("ctxmodel", 1, 48, 32), ("ctxmodel", 2, 32, 48), ("ctxmodel", 1, 16, 16),
                                        ("ctxmodel", 4, 16, 16), ("ctxmodel", 3, 5, 7), ("ctxmodel", 1, 7, 9), ("ctxmodel", 2, 3, 2),
                                        ("ctxmodel", 1, 5, 1), ("ctxmodel", 1, 1, 6), ("ctxmodel", 1, 1, 1), ("ctxmodel", 13, 4, 4),
                                        ("ctxmodel", 2, 32, 3), ("ctxmodel-k3", 1, 4, 3), ("ctxmodel-k3", 3, 16, 16)])
def test_wavefront_encode_equals_per_step_path(kind, B, H, W):
    _check_wavefront_equals_per_step(kind, B, H, W, B * 100 + H * 10 + W)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_wavefront_tile_boundary_seeds(seed):
    """Two column tiles: the first rows of image 1 read their causal rows from columns the OTHER tile's workgroups publish.  Five
    different inputs, each coded once."""
    _check_wavefront_equals_per_step("ctxmodel", 2, 32, 48, 9000 + seed)


@pytest.mark.parametrize("kind,C,B,H,W", [("ctxmodel", 192, 3, 32, 48), ("ctxmodel", 192, 65, 1, 4), ("merger", 32, 1, 5, 5)])
def test_wavefront_refused_on_the_host(kind, C, B, H, W):
    """B * H > 64, or layers that are not whole 32-row tiles: wavefront_max says so and a forced call fails before any launch."""
    coder = _shared_coder(kind, C)
    y, prior = _inputs(1, C, 2, 2, 5)
    coder.scanline_encode_schedule = "raster"
    coder._run_encode(y, prior)   # builds the plan
    sl = coder._layers["scanline"][0]
    sl.check()
    before = sl.last_kernel()
    assert before in ("generic", "pipelined", "batched")
    assert sl.wavefront_max(H, W) < B
    y, prior = _inputs(B, C, H, W, 6)
    sl.set_encode_schedule("wavefront")
    try:
        with pytest.raises((RuntimeError, ValueError), match="does not fit"):
            sl.encode(y, prior, coder._scale_table_dev)
    finally:
        sl.set_encode_schedule("auto")
    assert sl.last_kernel() == before   # no launch was made


@pytest.mark.parametrize("B,H,W", [(1, 32, 48), (13, 4, 4)])
def test_wavefront_guard_bands(B, H, W):
    """sym, idx and ybuf as views into sentinel-filled buffers: a wavefront launch writes all of each view and nothing else."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    C = 192
    coder = _shared_coder("ctxmodel", C)
    y, prior = _inputs(B, C, H, W, 77 + B)
    coder.use_persistent_scanline = False
    s0, i0, y0, _ = coder._run_encode(y, prior)
    coder.use_persistent_scanline = True
    coder.scanline_encode_schedule = "wavefront"
    coder._run_encode(y[:1, :, :2, :2].contiguous(), prior[:1, :, :2, :2].contiguous())   # builds the plan
    sl = coder._layers["scanline"][0]
    sl.check()
    table = coder._scale_table_dev.to(device="cuda", dtype=torch.float32).contiguous()
    n = B * H * W * C
    off = 64
    bufs = [torch.full((off + n + BAND,), GUARD, dtype=torch.int32, device="cuda") for _ in range(3)]
    for b in bufs:
        b[off: off + n] = 0x7FC00001   # (a NaN as float, no symbol or table row as integer)
    sym, idx, ybuf = (b[off: off + n] for b in bufs)
    sl.set_encode_schedule("wavefront")
    try:
        _lib.check(_lib.lib().basic_scanline_encode_dev(sl._h, y.data_ptr(), prior.data_ptr(), B, H, W, table.data_ptr(), table.numel(),
                                                        sym.data_ptr(), idx.data_ptr(), ybuf.data_ptr(), K._stream()))
        sl.check()
    finally:
        sl.set_encode_schedule("auto")
    assert sl.last_kernel() == "wavefront"
    for name, b in zip(("sym", "idx", "ybuf"), bufs):
        h = b.cpu()
        assert bool((h[:off] == GUARD).all()) and bool((h[off + n:] == GUARD).all()), f"the launch wrote outside {name}"
    assert torch.equal(sym.view(B, -1), s0) and torch.equal(idx.view(B, -1), i0)
    assert torch.equal(ybuf.view(B, C, H, W), y0.view(torch.int32))


@pytest.mark.parametrize("level", [0, 7])
def test_wavefront_codec_level(level):
    """BaSIC on one Kodak-shaped image: the raster and the wavefront schedule write the same bytes, which decompress to the same image."""
    from cbench_basic_amd.presets import basic_codec, seed_synthetic_weights
    codec = seed_synthetic_weights(basic_codec(), seed=0).eval().cuda()
    codec.update_state()
    codec.set_complex_level(level)
    yc = codec.entropy_coder.latent_node_entropy_coders["y"]
    x = torch.rand(1, 3, 512, 768, generator=torch.Generator().manual_seed(11)).cuda()
    yc.scanline_encode_schedule = "raster"
    raster = codec.compress(x)
    sl = yc._layers["scanline"][0]
    sl.check()
    assert sl.last_kernel() in ("generic", "pipelined", "batched")
    x_raster = codec.decompress(raster)
    yc.scanline_encode_schedule = "wavefront"
    wave = codec.compress(x)
    sl = yc._layers["scanline"][0]
    sl.check()
    assert sl.last_kernel() == "wavefront", sl.last_kernel()
    assert wave == raster
    x_wave = codec.decompress(wave)
    assert torch.equal(x_raster, x_wave)
