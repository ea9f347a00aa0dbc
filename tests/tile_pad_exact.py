"""Edge-padded tiles (include/basic_hip.h section 8d; cbench_basic_amd/utils/tiling.py, ``pad_to``), restated in numpy from their
formulas.  No tests here; no torch, no device, no project code.

The padded tile.  A tile of ph x pw whose origin (y, x) lies inside an H x W picture:
``P[c, r, q] = picture[c, min(y + r, H - 1), min(x + q, W - 1)] / 255`` for r < ph, q < pw, the quotient the correctly rounded float32 one.
The clipped paste.  The top-left ph x pw of a reconstruction goes to (y, x) of a canvas of H x W; only the samples with y + r < H and
x + q < W are written, as ``quantise`` of the source; every other byte of the canvas keeps its value.
"""
import numpy as np


def ceil_to(v, m):
    return -(-v // m) * m


def coded_size(h, w, py, px):
    """The size at which a tile of valid h x w is coded under pad_to = (py, px)."""
    return ceil_to(h, py), ceil_to(w, px)


def padded_tile_u8(picture, y, x, ph, pw):
    """``picture``: uint8 [C, H, W] -> uint8 [C, ph, pw], rows and columns beyond the picture clamped to its last."""
    picture = np.asarray(picture)
    _, H, W = picture.shape
    assert 0 <= y < H and 0 <= x < W
    iy = np.minimum(np.arange(y, y + ph), H - 1)
    ix = np.minimum(np.arange(x, x + pw), W - 1)
    return picture[:, iy[:, None], ix[None, :]]


def padded_tile(picture, y, x, ph, pw):
    """The float32 padded tile: u / 255, one correctly rounded float32 division per sample."""
    return np.divide(padded_tile_u8(picture, y, x, ph, pw).astype(np.float32), np.float32(255), dtype=np.float32)


def quantise(v):
    """The 8-bit picture of section 8b: uint8(rint(min(max(v, 0), 1) * 255)), NaN -> 0."""
    v = np.asarray(v, dtype=np.float32)
    c = np.minimum(np.maximum(np.where(np.isnan(v), np.float32(0), v), np.float32(0)), np.float32(1))
    return np.rint(np.multiply(c, np.float32(255), dtype=np.float32)).astype(np.uint8)


def clipped_paste(canvas, source, y, x, ph, pw):
    """``canvas``: uint8 [C, H, W], written in place; ``source``: float32 [C, sh, sw] with sh x sw at least ph x pw."""
    _, H, W = canvas.shape
    assert 0 <= y < H and 0 <= x < W and source.shape[1] >= ph and source.shape[2] >= pw
    h, w = min(ph, H - y), min(pw, W - x)
    canvas[:, y:y + h, x:x + w] = quantise(source[:, :h, :w])
    return canvas
