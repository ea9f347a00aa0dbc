"""The blend of overlapped tiles (include/basic_hip.h section 8c), restated in numpy float32 operation by operation, and the source
tiles the tests feed it.  No tests here; no torch, no device.

The definition.  Steps ``s = t - o``.  Along an axis the samples ``[(i + 1) * s, (i + 1) * s + o)`` are covered by tiles i and i + 1; the
sample at distance d into that band is ``lerp(a, b, ramp[d])``, a from tile i and b from tile i + 1, with
``ramp[d] = float32((2 * d + 1) / (2.0 * o))`` (a double division, rounded once) and ``lerp(a, b, w) = a + w * (b - a)`` as one float32
subtract, one multiply and one add, each rounded.  In a band of both axes x goes first: the two tile rows are cross-faded along x,
then the two results along y.  ``blend`` below does exactly that for the whole picture: every tile row becomes a strip of the
picture's width (x), the strips become the picture (y).  numpy's float32 ufuncs round every operation and fuse nothing.
"""
import numpy as np

TIES = ((np.arange(255, dtype=np.float64) + 0.5) / 255).astype(np.float32)      # every rounding tie of the 8-bit quantiser
SPECIAL = np.concatenate([TIES, np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 2.0, 1.0, 1e30, -1e30], dtype=np.float32)])


def ramp(o):
    return np.array([np.float32((2 * d + 1) / (2.0 * o)) for d in range(o)], dtype=np.float32)


def lerp(a, b, w):
    a, b, w = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), np.asarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.subtract(b, a, dtype=np.float32)
        scaled = np.multiply(w, diff, dtype=np.float32)
        return np.add(a, scaled, dtype=np.float32)


def _fade(parts, step, o, total, axis):
    """``parts[i]`` covers [i * step, i * step + its length) of ``axis``: the whole axis of ``total`` samples, bands cross-faded."""
    shape = list(parts[0].shape)
    shape[axis] = total
    out = np.empty(shape, dtype=np.float32)
    w = ramp(o).reshape([-1 if k == axis else 1 for k in range(len(shape))]) if o else None

    def cut(a, lo, hi):
        return a[tuple(slice(lo, hi) if k == axis else slice(None) for k in range(len(shape)))]
    for i, part in enumerate(parts):
        lo = i * step + (o if i else 0)                                   # the part's own samples
        hi = (i + 1) * step if i + 1 < len(parts) else total
        cut(out, lo, hi)[...] = cut(part, lo - i * step, hi - i * step)
        if i and o:                                                       # the band it shares with part i - 1
            cut(out, i * step, i * step + o)[...] = lerp(cut(parts[i - 1], step, step + o), cut(part, 0, o), w)
    return out


def blend(grid, tiles):
    """``tiles[k]``: float32 [C, sh, sw] with sh x sw at least tile k's size -> the picture [C, H, W], float32."""
    strips = []
    for i in range(grid.rows):
        row = []
        for j in range(grid.cols):
            _, _, h, w = grid.tile_rect(i * grid.cols + j)
            row.append(np.asarray(tiles[i * grid.cols + j], dtype=np.float32)[:, :h, :w])
        strips.append(_fade(row, grid.sx, grid.ox, grid.W, axis=2))
    return _fade(strips, grid.sy, grid.oy, grid.H, axis=1)


def paste(grid, tiles):
    """The plain paste of abutting tiles (overlap 0), written independently of ``blend``."""
    assert grid.overlap == (0, 0)
    out = np.empty((np.asarray(tiles[0]).shape[0], grid.H, grid.W), dtype=np.float32)
    for k in range(len(grid)):
        y, x, h, w = grid.tile_rect(k)
        out[:, y:y + h, x:x + w] = np.asarray(tiles[k])[:, :h, :w]
    return out


def quantise(v):
    """The 8-bit picture of section 8b: uint8(rint(min(max(v, 0), 1) * 255)), NaN -> 0."""
    v = np.asarray(v, dtype=np.float32)
    c = np.minimum(np.maximum(np.where(np.isnan(v), np.float32(0), v), np.float32(0)), np.float32(1))
    return np.rint(np.multiply(c, np.float32(255), dtype=np.float32)).astype(np.uint8)


def band_mask(grid):
    """[H, W] bool: the samples that lie in a band of either axis."""
    m = np.zeros((grid.H, grid.W), dtype=bool)
    for i in range(1, grid.rows):
        m[i * grid.sy:i * grid.sy + grid.oy, :] = True
    for j in range(1, grid.cols):
        m[:, j * grid.sx:j * grid.sx + grid.ox] = True
    return m


def agree_mask(grid):
    """[H, W] bool: where all covering tiles are given one value, so that a lerp returns it exactly (a + w * 0): patches of 7 x 11."""
    yy, xx = np.meshgrid(np.arange(grid.H), np.arange(grid.W), indexing="ij")
    return ((yy // 7 + xx // 11) % 2) == 0


def _values(rng, n):
    """n samples as the paste test draws them: uniform in [-0.25, 1.25) with every rounding tie, NaN, +-inf, negatives and values
    above 1 scattered over them."""
    x = (rng.random(n, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
    k = min(SPECIAL.size, n)
    x[rng.permutation(n)[:k]] = SPECIAL[rng.permutation(SPECIAL.size)[:k]]
    return x


def sources(grid, C, pads=((5, 4), (0, 0), (3, 5), (1, 0)), seed=0):
    """The reconstructions of a grid's tiles: [(batch [n, C, sh, sw] float32, tile indices)] per group, group g padded by
    ``pads[g % len(pads)]`` so that sh x sw differs inside one table, plus the dict k -> [C, sh, sw] view the reference reads.
    Every tile has values of its own (``_values``), the padding included.  Where ``agree_mask`` holds, all covering tiles carry
    the value of one shared picture instead, and that picture has every rounding tie inside the agreeing bands, so ties reach the
    quantiser through a blend unchanged."""
    rng = np.random.default_rng(seed + 1000 * C + grid.H + grid.W)
    shared = _values(rng, C * grid.H * grid.W).reshape(C, grid.H, grid.W)
    agree = agree_mask(grid)
    spots = np.argwhere(agree & band_mask(grid))                       # (y, x) of agreeing band samples
    if len(spots):
        pick = spots[rng.permutation(len(spots))[:TIES.size]]
        shared[rng.integers(0, C, len(pick)), pick[:, 0], pick[:, 1]] = TIES[:len(pick)]
    batches, tiles = [], {}
    for n, g in enumerate(grid.groups()):
        ph, pw = pads[n % len(pads)]
        batch = _values(rng, len(g.indices) * C * (g.h + ph) * (g.w + pw)).reshape(len(g.indices), C, g.h + ph, g.w + pw)
        for t, k in enumerate(g.indices):
            y, x, h, w = grid.tile_rect(k)
            m = agree[y:y + h, x:x + w]
            batch[t, :, :h, :w][:, m] = shared[:, y:y + h, x:x + w][:, m]
            tiles[k] = batch[t]
        batches.append((batch, tuple(g.indices)))
    # NaN, +-inf and values beyond [0, 1] inside bands for certain, in one of the covering tiles each
    odd = np.argwhere(~agree & band_mask(grid))
    extra = SPECIAL[TIES.size:]
    for n, (y, x) in enumerate(odd[rng.permutation(len(odd))[:4 * extra.size]]):
        k = next(k for k in range(len(grid)) for ty, tx, h, w in [grid.tile_rect(k)] if ty <= y < ty + h and tx <= x < tx + w)
        ty, tx, _, _ = grid.tile_rect(k)
        tiles[k][n % C, y - ty, x - tx] = extra[n % extra.size]
    return batches, tiles


def ties_in_bands(grid, picture):
    """How many distinct rounding ties the float picture holds inside bands."""
    return int(np.isin(TIES, picture[:, band_mask(grid)]).sum())
