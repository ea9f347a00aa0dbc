"""Tiled pictures: the geometry of a picture cut into independent tiles, and the container that holds the tiles' byte strings.

A picture of H x W is covered by ``rows x cols`` tiles of th x tw in row-major order, ``rows = ceil(H / th)``, ``cols = ceil(W / tw)``;
the tiles of the last row and column are as high and wide as the picture leaves them.  Tiles of one size form a regular grid -- a
*group* -- and a group is what one cut or paste kernel launch handles (include/basic_hip.h section 8c): the full tiles, the right
column, the bottom row, the corner; at most four.

Container, little-endian:  b"BTL1"  <B channels> <I H> <I W> <I th> <I tw> <I n>,  n x <I byte length>,  the n tile strings in
row-major order.  It states the picture's own size, which a tile's string does not (a decoder returns the synthesis transform's
size), and where each tile's string lies, which random access needs.  It says nothing about how the tiles' strings were written
(stream lanes, row streams, levels): that stays the coder's configuration.

Overlapped tiles (``overlap=(oy, ox)``, 0 <= 2 * oy <= th, 0 <= 2 * ox <= tw): the tiles' origins are ``sy = th - oy`` and ``sx = tw - ox``
apart, ``rows = max(1, ceil((H - oy) / sy))`` (columns likewise), tile (i, j) starts at (i * sy, j * sx) and is th x tw, cut off at
the picture's edge.  A sample is covered by at most two tiles per axis; the doubly covered samples of an axis are the bands
``[(i + 1) * s, (i + 1) * s + o)``, over which a decoder cross-fades the two reconstructions (include/basic_hip.h section 8c); a last
tile is always longer than the overlap.  Such a picture's container is  b"BTL2"  <B channels> <I H> <I W> <I th> <I tw> <I oy> <I ox>
<I n>,  then lengths and strings as above; with overlap (0, 0) the container is BTL1, byte for byte.

Edge-padded tiles (``pad_to=(py, px)``, th % py == 0 and tw % px == 0; default (1, 1), none): the grid is the same -- no tile is added
or moved, ``tile_rect`` stays the valid rectangle -- but an edge tile is CODED at ``coded_size(k)``, its valid h x w rounded up to
multiples of py x px (never more than th x tw), the extra rows and columns replicating the picture's last row and column:
``P_k[c, r, q] = image[c, min(y + r, H - 1), min(x + q, W - 1)]``.  A decoder crops every tile to its valid rectangle.  With
``pad_to=(th, tw)`` every tile of every picture is th x tw.  Such a picture's container is  b"BTL3"  <B channels> <I H> <I W> <I th>
<I tw> <I oy> <I ox> <I py> <I px> <I n>  (41 bytes), then lengths and strings as above; with pad_to (1, 1) the container is BTL1 / BTL2,
byte for byte.

Pure host code: no torch, no device.
"""
import struct
from typing import Iterator, List, NamedTuple, Sequence, Tuple

MAGIC = b"BTL1"
_HEAD = struct.Struct("<4sBIIIII")
MAGIC2 = b"BTL2"
_HEAD2 = struct.Struct("<4sBIIIIIII")
MAGIC3 = b"BTL3"
_HEAD3 = struct.Struct("<4sBIIIIIIIII")


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


def _overlap_pair(overlap):
    """``overlap`` -- an int or (oy, ox) -- as a pair of non-negative ints."""
    try:
        pair = (overlap, overlap) if isinstance(overlap, int) else tuple(overlap)
    except TypeError:
        pair = ()
    if len(pair) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in pair):
        raise ValueError(f"overlap is a non-negative integer or (oy, ox), not {overlap!r}")
    return pair


def _pad_pair(pad_to):
    """``pad_to`` -- an int or (py, px) -- as a pair of positive ints."""
    try:
        pair = (pad_to, pad_to) if isinstance(pad_to, int) else tuple(pad_to)
    except TypeError:
        pair = ()
    if len(pair) != 2 or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in pair):
        raise ValueError(f"pad_to is a positive integer or (py, px), not {pad_to!r}")
    return pair


class TileGrid:
    """The tiles of an H x W picture cut into th x tw tiles (the edge tiles smaller) whose neighbours share ``overlap = (oy, ox)``
    rows and columns (none by default); ``pad_to = (py, px)``: the edge tiles are coded at their size rounded up to multiples of
    py x px (``coded_size``), which changes no tile's place or valid rectangle."""

    def __init__(self, H, W, th, tw, overlap=(0, 0), pad_to=(1, 1)):
        self.H, self.W = _positive_int("H", H), _positive_int("W", W)
        self.th, self.tw = _positive_int("th", th), _positive_int("tw", tw)
        self.oy, self.ox = self.overlap = _overlap_pair(overlap)
        if 2 * self.oy > self.th or 2 * self.ox > self.tw:
            raise ValueError(f"an overlap of {self.overlap} is more than half a {self.th} x {self.tw} tile")
        self.py, self.px = self.pad_to = _pad_pair(pad_to)
        if self.th % self.py or self.tw % self.px:
            raise ValueError(f"pad_to {self.pad_to} does not divide a {self.th} x {self.tw} tile")
        self.sy, self.sx = self.th - self.oy, self.tw - self.ox   # the steps between the tiles' origins
        self.rows, self.cols = max(1, -(-(self.H - self.oy) // self.sy)), max(1, -(-(self.W - self.ox) // self.sx))

    def __len__(self):
        return self.rows * self.cols

    def tile_rect(self, k):
        """(y, x, h, w) of tile k."""
        if not 0 <= k < len(self):
            raise IndexError(f"tile {k} of {len(self)}")
        i, j = divmod(k, self.cols)
        y, x = i * self.sy, j * self.sx
        return y, x, min(self.th, self.H - y), min(self.tw, self.W - x)

    def coded_size(self, k):
        """(ph, pw) at which tile k is coded: its valid h x w rounded up to multiples of ``pad_to``; at most th x tw."""
        _, _, h, w = self.tile_rect(k)
        return -(-h // self.py) * self.py, -(-w // self.px) * self.px

    def _bands(self, n, size, step, total, lo=0, hi=None):
        """Index ranges [a, b) of one axis within [lo, hi) that hold tiles of one size: the full ones, then the smaller last one."""
        hi = n if hi is None else hi
        last = total - (n - 1) * step   # size of tile n - 1
        if last == size or hi < n:
            return [(lo, hi, size)] if hi > lo else []
        out = [(lo, n - 1, size)] if n - 1 > lo else []
        out.append((n - 1, n, last))
        return out

    def _groups(self, i0, i1, j0, j1) -> Iterator[TileGroup]:
        for a, b, h in self._bands(self.rows, self.th, self.sy, self.H, i0, i1):
            for c, d, w in self._bands(self.cols, self.tw, self.sx, self.W, j0, j1):
                yield TileGroup(a * self.sy, c * self.sx, self.sy, self.sx, b - a, d - c, h, w,
                                tuple(i * self.cols + j for i in range(a, b) for j in range(c, d)))

    def groups(self) -> List[TileGroup]:
        """The picture's tiles as at most four groups: full tiles, right column, bottom row, corner."""
        return list(self._groups(0, self.rows, 0, self.cols))

    def tiles_of_region(self, y0, x0, y1, x1) -> List[TileGroup]:
        """The groups (sub-grids) of the tiles that cover a sample of the rectangle [y0, y1) x [x0, x1): with an overlap, both
        tiles of every band the rectangle touches."""
        if not (0 <= y0 < y1 <= self.H and 0 <= x0 < x1 <= self.W):
            raise ValueError(f"region {(y0, x0, y1, x1)} is empty or leaves the {self.H} x {self.W} picture")
        # tile i of an axis covers [i * s, i * s + t): the first with i * s + t > lo, up to the last with i * s < hi
        return list(self._groups(max(0, (y0 - self.th) // self.sy + 1), min(self.rows, -(-y1 // self.sy)),
                                 max(0, (x0 - self.tw) // self.sx + 1), min(self.cols, -(-x1 // self.sx))))


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


class PooledTile(NamedTuple):
    """Tile ``index`` (row-major) of picture ``picture``, whose origin is (y0, x0)."""
    picture: int
    index: int
    y0: int
    x0: int


class TileChunk(NamedTuple):
    """Tiles of one coded size (h, w), of any pictures: what one pooled coding call takes."""
    h: int
    w: int
    tiles: Tuple[PooledTile, ...]


def pool_tiles(grids: Sequence[TileGrid], max_batch=None) -> List[TileChunk]:
    """The tiles of many pictures -- ``grids[p]`` is picture p's TileGrid -- as chunks of equally sized tiles: the full tiles of every
    picture are th x tw whatever the picture's size, and the edge tiles fall into a few more sizes.  The order is fixed: sizes in the
    order of their first appearance (pictures in order, a picture's tiles row-major), within a size picture-major and tile-major,
    cut into chunks of at most ``max_batch`` tiles (None / 0: one chunk per size).  So every tile of every picture is in exactly
    one chunk, and there are ``sum over the sizes of ceil(count / max_batch)`` chunks.  A tile's size is its ``coded_size``: the
    valid size for a grid without padding, and with ``pad_to`` the rounded one, so that the edge tiles of padded grids fall into fewer
    sizes -- with ``pad_to=(th, tw)`` into the one of the full tiles."""
    if max_batch is not None and (isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 0):
        raise ValueError(f"max_batch must be a positive integer or None, not {max_batch!r}")
    by_size = {}   # insertion-ordered: a size's first appearance
    for p, grid in enumerate(grids):
        for k in range(len(grid)):
            y, x, _, _ = grid.tile_rect(k)
            by_size.setdefault(grid.coded_size(k), []).append(PooledTile(p, k, y, x))
    out = []
    for (h, w), tiles in by_size.items():
        step = max_batch or len(tiles)
        out.extend(TileChunk(h, w, tuple(tiles[i:i + step])) for i in range(0, len(tiles), step))
    return out


def pack_tiled(channels, H, W, th, tw, strings: Sequence[bytes], overlap=(0, 0), pad_to=(1, 1)) -> bytes:
    """The container of a picture's tile strings (row-major order): BTL1, BTL2 when the tiles overlap, BTL3 when the edge tiles are
    padded (``pad_to`` other than (1, 1))."""
    grid = TileGrid(H, W, th, tw, overlap, pad_to)
    strings = [bytes(s) for s in strings]
    if len(strings) != len(grid):
        raise ValueError(f"{len(strings)} strings for {grid.rows} x {grid.cols} tiles")
    if not 1 <= channels <= 255:
        raise ValueError(f"channels must be in 1..255, not {channels!r}")
    if max(H, W, th, tw, len(strings), *[len(s) for s in strings]) >= 1 << 32:
        raise ValueError("a field of the container does not fit 32 bits")
    if grid.pad_to != (1, 1):
        head = _HEAD3.pack(MAGIC3, channels, H, W, th, tw, grid.oy, grid.ox, grid.py, grid.px, len(strings))
    elif grid.overlap == (0, 0):
        head = _HEAD.pack(MAGIC, channels, H, W, th, tw, len(strings))
    else:
        head = _HEAD2.pack(MAGIC2, channels, H, W, th, tw, grid.oy, grid.ox, len(strings))
    return b"".join([head,
                     struct.pack("<%dI" % len(strings), *[len(s) for s in strings])] + strings)


class TiledPicture(NamedTuple):
    """What a container states, and its tile strings in row-major order."""
    channels: int
    H: int
    W: int
    th: int
    tw: int
    overlap: Tuple[int, int]
    pad_to: Tuple[int, int]
    strings: List[bytes]


def unpack_tiled_full(data) -> TiledPicture:
    """A BTL1, BTL2 or BTL3 container as a TiledPicture; ValueError for anything that is not exactly one."""
    return _unpack(data, (MAGIC, MAGIC2, MAGIC3))


def unpack_tiled_any(data):
    """(channels, H, W, th, tw, (oy, ox), [tile strings]) of a BTL1 or BTL2 container; ValueError for anything that is not exactly one."""
    t = _unpack(data, (MAGIC, MAGIC2))
    return t.channels, t.H, t.W, t.th, t.tw, t.overlap, t.strings


def _unpack(data, magics) -> TiledPicture:
    data = bytes(data)
    if data[:4] not in magics:
        raise ValueError("not a tiled picture: wrong magic")
    head = {MAGIC: _HEAD, MAGIC2: _HEAD2, MAGIC3: _HEAD3}[data[:4]]
    if len(data) < head.size:
        raise ValueError("truncated tiled picture: head cut short")
    fields = head.unpack_from(data)
    channels, H, W, th, tw = fields[1:6]
    oy, ox = fields[6:8] if head is not _HEAD else (0, 0)
    py, px = fields[8:10] if head is _HEAD3 else (1, 1)
    n = fields[-1]
    if min(channels, H, W, th, tw) < 1:
        raise ValueError("tiled picture: a dimension is zero")
    if 2 * oy > th or 2 * ox > tw:
        raise ValueError(f"tiled picture: an overlap of {(oy, ox)} is more than half a {th} x {tw} tile")
    if min(py, px) < 1:
        raise ValueError("tiled picture: pad_to is zero")
    if th % py or tw % px:
        raise ValueError(f"tiled picture: pad_to {(py, px)} does not divide a {th} x {tw} tile")
    grid = TileGrid(H, W, th, tw, (oy, ox), (py, px))
    if n != len(grid):
        raise ValueError(f"tiled picture: {n} tiles stated, {grid.rows} x {grid.cols} expected")
    cur = head.size
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
    return TiledPicture(channels, H, W, th, tw, (oy, ox), (py, px), strings)


def unpack_tiled(data):
    """(channels, H, W, th, tw, [tile strings]) of a BTL1 container; ValueError for anything that is not exactly one."""
    if bytes(data[:4]) != MAGIC:
        raise ValueError("not a tiled picture: wrong magic")
    channels, H, W, th, tw, _, strings = unpack_tiled_any(data)
    return channels, H, W, th, tw, strings


# ---------------------------------------------------------------- BTQ1: tiles coded under a quantiser step (utils/qstep.py)
# b"BTQ1", the BTL3 head fields (channels, H, W, th, tw, oy, ox, py, px, n), n float32 LE steps (one per tile, row-major), n uint32
# lengths, the n tile strings.  Tile k's string is the inner stream of compress_q(P_k, step_k) -- encode(P_k, qstep=step_k) -- which
# does not hold its step: the container does.  A step per tile, so that a per-tile allocation needs no new format; a picture coded
# under one step carries it n times.
MAGIC_Q = b"BTQ1"
_HEAD_Q = _HEAD3
_STEP, _LEN = struct.Struct("<f"), struct.Struct("<I")


class TiledPictureQ(NamedTuple):
    """What a BTQ1 container states: the TiledPicture fields, and ``steps``, float32 [n], the quantiser step of every tile."""
    channels: int
    H: int
    W: int
    th: int
    tw: int
    overlap: Tuple[int, int]
    pad_to: Tuple[int, int]
    strings: List[bytes]
    steps: "object"


def pack_tiled_q(channels, H, W, th, tw, strings: Sequence[bytes], steps, overlap=(0, 0), pad_to=(1, 1)) -> bytes:
    """The BTQ1 container of a picture's tile strings (row-major order) coded under ``steps``: one step, or one per tile."""
    import numpy as np
    from .qstep import check_qsteps
    grid = TileGrid(H, W, th, tw, overlap, pad_to)
    strings = [bytes(s) for s in strings]
    if len(strings) != len(grid):
        raise ValueError(f"{len(strings)} strings for {grid.rows} x {grid.cols} tiles")
    steps = np.broadcast_to(check_qsteps(steps, len(grid)), (len(grid),))
    if not 1 <= channels <= 255:
        raise ValueError(f"channels must be in 1..255, not {channels!r}")
    if max(H, W, th, tw, len(strings), *[len(s) for s in strings]) >= 1 << 32:
        raise ValueError("a field of the container does not fit 32 bits")
    head = _HEAD_Q.pack(MAGIC_Q, channels, H, W, th, tw, grid.oy, grid.ox, grid.py, grid.px, len(strings))
    return b"".join([head, steps.astype("<f4").tobytes(),
                     struct.pack("<%dI" % len(strings), *[len(s) for s in strings])] + strings)


def unpack_tiled_q(data) -> TiledPictureQ:
    """A BTQ1 container as a TiledPictureQ; ValueError for anything that is not exactly one: a wrong magic, a short buffer, a tile
    count that is not the grid's, lengths that do not add up to the buffer, a step that is not finite or lies outside [2^-4, 2^6]."""
    import numpy as np
    from .qstep import check_qsteps
    data = bytes(data)
    if data[:4] != MAGIC_Q:
        raise ValueError("not a tiled picture with quantiser steps: wrong magic")
    if len(data) < _HEAD_Q.size:
        raise ValueError("truncated tiled picture: head cut short")
    _, channels, H, W, th, tw, oy, ox, py, px, n = _HEAD_Q.unpack_from(data)
    if min(channels, H, W, th, tw) < 1:
        raise ValueError("tiled picture: a dimension is zero")
    if 2 * oy > th or 2 * ox > tw:
        raise ValueError(f"tiled picture: an overlap of {(oy, ox)} is more than half a {th} x {tw} tile")
    if min(py, px) < 1:
        raise ValueError("tiled picture: pad_to is zero")
    if th % py or tw % px:
        raise ValueError(f"tiled picture: pad_to {(py, px)} does not divide a {th} x {tw} tile")
    grid = TileGrid(H, W, th, tw, (oy, ox), (py, px))
    if n != len(grid):
        raise ValueError(f"tiled picture: {n} tiles stated, {grid.rows} x {grid.cols} expected")
    cur = _HEAD_Q.size
    if cur + _STEP.size * n > len(data):
        raise ValueError("truncated tiled picture: step table cut short")
    steps = check_qsteps(np.frombuffer(data, dtype="<f4", count=n, offset=cur), n)
    cur += _STEP.size * n
    if cur + _LEN.size * n > len(data):
        raise ValueError("truncated tiled picture: length table cut short")
    lens = struct.unpack_from("<%dI" % n, data, cur)
    cur += _LEN.size * n
    if cur + sum(lens) > len(data):
        raise ValueError("truncated tiled picture: payload cut short")
    strings = []
    for L in lens:
        strings.append(data[cur:cur + L])
        cur += L
    if cur != len(data):
        raise ValueError(f"tiled picture: {len(data) - cur} bytes after the last tile")
    return TiledPictureQ(channels, H, W, th, tw, (oy, ox), (py, px), strings, np.broadcast_to(steps, (n,)).copy())


def tiled_q_framing_bytes(grid, stream_lanes=1, n_bodies=2, streams_per_body=None) -> int:
    """The exact number of bytes of a BTQ1 container that are not rANS payload: the head, a step and a length per tile, and per
    tile string the bodies' framing (utils/item_framing.py: a length in front of every body but the last, per body the header and
    one length per stream).  ``grid``: a TileGrid, or the number of tiles.  A tile string holds ``n_bodies`` CompressAI-style bodies,
    the last of ``stream_lanes`` streams (the y coder's) and the others of one; ``streams_per_body`` states every body's count."""
    from .item_framing import compressai_string_framing
    n = grid if isinstance(grid, int) and not isinstance(grid, bool) else len(grid)
    if n < 1:
        raise ValueError(f"a picture has at least one tile, not {n!r}")
    if streams_per_body is None:
        if isinstance(n_bodies, bool) or not isinstance(n_bodies, int) or n_bodies < 1:
            raise ValueError(f"n_bodies must be a positive integer, not {n_bodies!r}")
        streams_per_body = [1] * (n_bodies - 1) + [stream_lanes]
    return _HEAD_Q.size + n * (_STEP.size + _LEN.size + compressai_string_framing(streams_per_body))
