"""Tiled pictures: the geometry of a picture cut into independent tiles, and the container that holds the tiles' byte strings.

A picture of H x W is covered by ``rows x cols`` tiles of th x tw in row-major order, ``rows = ceil(H / th)``, ``cols = ceil(W / tw)``;
the tiles of the last row and column are as high and wide as the picture leaves them.  Tiles of one size form a regular grid -- a
*group* -- and a group is what one cut or paste kernel launch handles (include/basic_hip.h section 8c): the full tiles, the right
column, the bottom row, the corner; at most four.

Container, little-endian:  b"BTL1"  <B channels> <I H> <I W> <I th> <I tw> <I n>,  n x <I byte length>,  the n tile strings in
row-major order.  It states the picture's own size, which a tile's string does not (a decoder returns the synthesis transform's
size), and where each tile's string lies, which random access needs.  It says nothing about how the tiles' strings were written
(stream lanes, row streams, levels): that stays the coder's configuration.

Pure host code: no torch, no device.
"""
import struct
from typing import Iterator, List, NamedTuple, Sequence, Tuple

MAGIC = b"BTL1"
_HEAD = struct.Struct("<4sBIIIII")


class TileGroup(NamedTuple):
    """A regular grid of ny x nx tiles of h x w: tile (i, j) has its origin at (y0 + i * step_y, x0 + j * step_x) and is entry
    i * nx + j of ``indices``, the tiles' row-major numbers in the picture."""
    y0: int
    x0: int
    step_y: int
    step_x: int
    ny: int
    nx: int
    h: int
    w: int
    indices: Tuple[int, ...]


def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"{name} must be a positive integer, not {v!r}")
    return v


class TileGrid:
    """The tiles of an H x W picture cut into th x tw tiles (the edge tiles smaller)."""

    def __init__(self, H, W, th, tw):
        self.H, self.W = _positive_int("H", H), _positive_int("W", W)
        self.th, self.tw = _positive_int("th", th), _positive_int("tw", tw)
        self.rows, self.cols = -(-self.H // self.th), -(-self.W // self.tw)

    def __len__(self):
        return self.rows * self.cols

    def tile_rect(self, k):
        """(y, x, h, w) of tile k."""
        if not 0 <= k < len(self):
            raise IndexError(f"tile {k} of {len(self)}")
        i, j = divmod(k, self.cols)
        y, x = i * self.th, j * self.tw
        return y, x, min(self.th, self.H - y), min(self.tw, self.W - x)

    def _bands(self, n, size, total, lo=0, hi=None):
        """Index ranges [a, b) of one axis within [lo, hi) that hold tiles of one size: the full ones, then the smaller last one."""
        hi = n if hi is None else hi
        last = total - (n - 1) * size   # size of tile n - 1
        if last == size or hi < n:
            return [(lo, hi, size)] if hi > lo else []
        out = [(lo, n - 1, size)] if n - 1 > lo else []
        out.append((n - 1, n, last))
        return out

    def _groups(self, i0, i1, j0, j1) -> Iterator[TileGroup]:
        for a, b, h in self._bands(self.rows, self.th, self.H, i0, i1):
            for c, d, w in self._bands(self.cols, self.tw, self.W, j0, j1):
                yield TileGroup(a * self.th, c * self.tw, self.th, self.tw, b - a, d - c, h, w,
                                tuple(i * self.cols + j for i in range(a, b) for j in range(c, d)))

    def groups(self) -> List[TileGroup]:
        """The picture's tiles as at most four groups: full tiles, right column, bottom row, corner."""
        return list(self._groups(0, self.rows, 0, self.cols))

    def tiles_of_region(self, y0, x0, y1, x1) -> List[TileGroup]:
        """The groups (sub-grids) of the tiles that intersect the rectangle [y0, y1) x [x0, x1)."""
        if not (0 <= y0 < y1 <= self.H and 0 <= x0 < x1 <= self.W):
            raise ValueError(f"region {(y0, x0, y1, x1)} is empty or leaves the {self.H} x {self.W} picture")
        return list(self._groups(y0 // self.th, -(-y1 // self.th), x0 // self.tw, -(-x1 // self.tw)))


def split_group(group: TileGroup, max_batch=None) -> List[TileGroup]:
    """A group as sub-grids of at most ``max_batch`` tiles each (None / 0: the group itself).  Every chunk is again a regular grid,
    a x b tiles with a * b <= max_batch; of all such shapes the one that needs the fewest chunks is taken (a call costs more than
    its tiles do: profiles/tiled_coding.txt), whole rows of the grid where that is no worse."""
    if max_batch is not None and (isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 0):
        raise ValueError(f"max_batch must be a positive integer or None, not {max_batch!r}")
    g = group
    if not max_batch or g.ny * g.nx <= max_batch:
        return [g]
    best = None
    for a in range(1, min(g.ny, max_batch) + 1):
        b = min(g.nx, max_batch // a)
        count = -(-g.ny // a) * -(-g.nx // b)
        if best is None or (count, -b) < (best[0], -best[2]):
            best = (count, a, b)
    _, a, b = best
    out = []
    for i in range(0, g.ny, a):
        for j in range(0, g.nx, b):
            i1, j1 = min(i + a, g.ny), min(j + b, g.nx)
            out.append(g._replace(y0=g.y0 + i * g.step_y, x0=g.x0 + j * g.step_x, ny=i1 - i, nx=j1 - j,
                                  indices=tuple(g.indices[r * g.nx + c] for r in range(i, i1) for c in range(j, j1))))
    return out


def pack_tiled(channels, H, W, th, tw, strings: Sequence[bytes]) -> bytes:
    """The container of a picture's tile strings (row-major order)."""
    grid = TileGrid(H, W, th, tw)
    strings = [bytes(s) for s in strings]
    if len(strings) != len(grid):
        raise ValueError(f"{len(strings)} strings for {grid.rows} x {grid.cols} tiles")
    if not 1 <= channels <= 255:
        raise ValueError(f"channels must be in 1..255, not {channels!r}")
    if max(H, W, th, tw, len(strings), *[len(s) for s in strings]) >= 1 << 32:
        raise ValueError("a field of the container does not fit 32 bits")
    return b"".join([_HEAD.pack(MAGIC, channels, H, W, th, tw, len(strings)),
                     struct.pack("<%dI" % len(strings), *[len(s) for s in strings])] + strings)


def unpack_tiled(data):
    """(channels, H, W, th, tw, [tile strings]) of a container; ValueError for anything that is not exactly one."""
    data = bytes(data)
    if data[:4] != MAGIC:
        raise ValueError("not a tiled picture: wrong magic")
    if len(data) < _HEAD.size:
        raise ValueError("truncated tiled picture: head cut short")
    _, channels, H, W, th, tw, n = _HEAD.unpack_from(data)
    if min(channels, H, W, th, tw) < 1:
        raise ValueError("tiled picture: a dimension is zero")
    grid = TileGrid(H, W, th, tw)
    if n != len(grid):
        raise ValueError(f"tiled picture: {n} tiles stated, {grid.rows} x {grid.cols} expected")
    cur = _HEAD.size
    if cur + 4 * n > len(data):
        raise ValueError("truncated tiled picture: length table cut short")
    lens = struct.unpack_from("<%dI" % n, data, cur)
    cur += 4 * n
    if cur + sum(lens) > len(data):
        raise ValueError("truncated tiled picture: payload cut short")
    strings = []
    for L in lens:
        strings.append(data[cur:cur + L])
        cur += L
    if cur != len(data):
        raise ValueError(f"tiled picture: {len(data) - cur} bytes after the last tile")
    return channels, H, W, th, tw, strings
