"""The band encode schedule of the batched scan-line kernel (csrc/scanline.hip: the wavefront's W + s * (H - 1) steps, but an image's
rows share W // s + 1 column slots of one MFMA tile, so any batch and any height is served, in successive launches where one does
not hold the batch) against the per-step path of the same coder.  The schedule changes addressing, not arithmetic: symbols, table
rows, the coded latent (float bits) and the bytes must be EQUAL -- no tolerance anywhere -- and ScanlinePlan.last_kernel() must
say that the band ran."""
import pytest
import torch

from scanline_cases import (_inputs, _plan_of, _shared_coder, check_codec_level, check_guard_bands, check_refused_on_the_host,
                            check_schedule_equals_per_step)

pytestmark = pytest.mark.gpu


def _check_band_equals_per_step(kind, B, H, W, seed):
    check_schedule_equals_per_step("band", kind, B, H, W, seed)


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
    check_refused_on_the_host("band", kind, C, B, H, W)


@pytest.mark.parametrize("B,H,W", [(7, 16, 16), (None, 4, 4)])
def test_band_guard_bands(B, H, W):
    """sym, idx and ybuf as views into sentinel-filled buffers: the band's launches write all of each view and nothing else
    (B None: three images more than one launch holds)."""
    if B is None:
        B = _plan_of(_shared_coder("ctxmodel", 192), 192).band_max(H, W) + 3
    check_guard_bands("band", B, H, W)


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
    check_codec_level("band", level, (5, 3, 256, 256))
