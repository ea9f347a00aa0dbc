"""The wavefront encode schedule of the batched scan-line kernel (csrc/scanline.hip: a column of the MFMA tiles is one row of one
image, step t codes column position t - s * r of every row r, W + s * (H - 1) dependent steps instead of H * W) against the
per-step path of the same coder.  The schedule changes addressing, not arithmetic: symbols, table rows, the coded latent (float
bits) and the bytes must be EQUAL -- no tolerance anywhere -- and ScanlinePlan.last_kernel() must say that the wavefront ran."""
import pytest

from scanline_cases import check_codec_level, check_guard_bands, check_refused_on_the_host, check_schedule_equals_per_step

pytestmark = pytest.mark.gpu


def _check_wavefront_equals_per_step(kind, B, H, W, seed):
    check_schedule_equals_per_step("wavefront", kind, B, H, W, seed)


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
    check_refused_on_the_host("wavefront", kind, C, B, H, W)


@pytest.mark.parametrize("B,H,W", [(1, 32, 48), (13, 4, 4)])
def test_wavefront_guard_bands(B, H, W):
    """sym, idx and ybuf as views into sentinel-filled buffers: a wavefront launch writes all of each view and nothing else."""
    check_guard_bands("wavefront", B, H, W)


@pytest.mark.parametrize("level", [0, 7])
def test_wavefront_codec_level(level):
    """BaSIC on one Kodak-shaped image: the raster and the wavefront schedule write the same bytes, which decompress to the same image."""
    check_codec_level("wavefront", level, (1, 3, 512, 768))
