"""Item framing: the byte string of a batch of N images <-> the N byte strings of its images coded one at a time.

An image's rANS streams do not depend on the batch it is coded in (tests/test_gpu_codec.py, tests/test_gpu_ar_codecs.py); only the
framing around them does.  These functions move streams between the two framings without touching a payload byte, so N batch-1
items can be coded in ONE call and still yield exactly the N strings N calls would have written (and back, for decoding).  Pure host
functions over ``bytes``: no device, no tables.

  CompressAI-style bodies (compressai_coder.py ``write_body`` / ``read_body``):  ">III" (h, w, n), then per stream ">I" length + payload.
      n = S * B with S streams per item (1, or the y coder's stream_lanes); an item body is the same form with n = S.
  PGM bodies (pgm_coder.py ``_encode_impl``):  the optional shape head  B(len) <H batch> <H dims...>,  then
      batched form:  <I S*B> <S*B x I length> streams       (S streams per item: 1, stream_lanes, or H * stream_lanes with rows)
      item form:     the bare rANS stream (S = 1, ``batch_stream_mode="auto"``)  or  <I S> <S x I length> streams  (``item_tabled``)
  Whole-codec strings:  merge_bytes(bodies, num_segments=len(nodes)), split and merged node by node.
"""
import struct
from typing import Callable, Hashable, List, Optional, Sequence

from .bytes_ops import merge_bytes, split_merged_bytes


# ---------------------------------------------------------------- which items share a call
def coalesce_chunks(shapes: Sequence[Hashable], max_batch: Optional[int] = None) -> List[List[int]]:
    """Indices of the items that are coded together: items are grouped by ``shapes[i]`` (any hashable key), groups are ordered by
    first appearance, a group keeps the dataset order, and a chunk holds at most ``max_batch`` items (None / 0: the whole group)."""
    if max_batch is not None and int(max_batch) < 0:
        raise ValueError(f"max_batch must be a positive integer or None, not {max_batch!r}")
    groups = {}
    for i, key in enumerate(shapes):
        groups.setdefault(key, []).append(i)   # dicts keep insertion order: first appearance
    step = int(max_batch) if max_batch else None
    out = []
    for idx in groups.values():
        if step is None:
            out.append(idx)
        else:
            out.extend(idx[i:i + step] for i in range(0, len(idx), step))
    return out


# ---------------------------------------------------------------- CompressAI-style bodies
def _parse_compressai(body):
    body = bytes(body)
    if len(body) < 12:
        raise ValueError("truncated body: no (h, w, n) header")
    h, w, n = struct.unpack(">3I", body[:12])
    cur, streams = 12, []
    for _ in range(n):
        if cur + 4 > len(body):
            raise ValueError("truncated body: stream length missing")
        (L,) = struct.unpack(">I", body[cur:cur + 4])
        cur += 4
        if cur + L > len(body):
            raise ValueError("truncated body: stream shorter than its length")
        streams.append(body[cur:cur + L])
        cur += L
    if cur != len(body):
        raise ValueError(f"body holds {len(body) - cur} bytes after its last stream")
    return h, w, streams


def compressai_body_shape(body):
    """(h, w, n) of a body's header."""
    if len(body) < 12:
        raise ValueError("truncated body: no (h, w, n) header")
    return struct.unpack(">3I", bytes(body[:12]))


def _write_compressai(h, w, streams):
    parts = [struct.pack(">3I", h, w, len(streams))]
    for s in streams:
        parts.append(struct.pack(">I", len(s)))
        parts.append(s)
    return b"".join(parts)


def _check_streams_per_item(S):
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise ValueError(f"streams per item must be an integer >= 1, not {S!r}")
    return S


def split_compressai_body(body, streams_per_item=1) -> List[bytes]:
    """The batch-1 bodies of a body of n streams, ``streams_per_item`` consecutive streams each (lane streams: stream b * S + k is
    lane k of item b)."""
    S = _check_streams_per_item(streams_per_item)
    h, w, streams = _parse_compressai(body)
    if len(streams) % S:
        raise ValueError(f"{len(streams)} streams do not divide into items of {S}")
    return [_write_compressai(h, w, streams[i:i + S]) for i in range(0, len(streams), S)]


def merge_compressai_bodies(bodies, streams_per_item=1) -> bytes:
    """Inverse of split_compressai_body: batch-1 bodies of one (h, w) -> the body of the batch."""
    S = _check_streams_per_item(streams_per_item)
    bodies = list(bodies)
    if not bodies:
        raise ValueError("no bodies to merge")
    shape, streams = None, []
    for b in bodies:
        h, w, s = _parse_compressai(b)
        if len(s) != S:
            raise ValueError(f"an item body holds {'one stream' if S == 1 else '%d streams' % S}, not {len(s)}")
        if shape is None:
            shape = (h, w)
        elif shape != (h, w):
            raise ValueError(f"bodies of different shapes: {shape} and {(h, w)}")
        streams.extend(s)
    return _write_compressai(shape[0], shape[1], streams)


def compressai_body_framing(n_streams) -> int:
    """Bytes of a CompressAI-style body of ``n_streams`` streams that are not payload: the ">III" header and a ">I" length per stream
    (what ``_write_compressai`` writes around the streams)."""
    return struct.calcsize(">3I") + struct.calcsize(">I") * _check_streams_per_item(n_streams)


def compressai_string_framing(streams_per_body: Sequence[int], num_bytes_length=4) -> int:
    """Bytes that are not payload in a whole-codec string of CompressAI-style bodies, body k of ``streams_per_body[k]`` streams:
    merge_bytes(bodies, num_segments=len(bodies)) writes a length in front of every body but the last."""
    streams_per_body = list(streams_per_body)
    if not streams_per_body:
        raise ValueError("a codec string holds at least one body")
    return num_bytes_length * (len(streams_per_body) - 1) + sum(compressai_body_framing(s) for s in streams_per_body)


# ---------------------------------------------------------------- PGM bodies
def _pgm_head(body, has_head):
    """(batch, dims, offset of what follows) of the optional shape head."""
    if not has_head:
        return None, None, 0
    if len(body) < 1:
        raise ValueError("truncated body: no shape head")
    nd = body[0]
    if nd < 1 or len(body) < 1 + 2 * nd:
        raise ValueError("truncated body: shape head cut short")
    dims = struct.unpack("<%dH" % nd, body[1:1 + 2 * nd])
    return dims[0], tuple(dims[1:]), 1 + 2 * nd


def _write_pgm_head(batch, dims):
    return struct.pack("B", len(dims) + 1) + struct.pack("<H", batch) + b"".join(struct.pack("<H", d) for d in dims)


def pgm_body_shape(body, has_head=False):
    """The spatial dims a PGM body's head states, or None when the body carries no head."""
    return _pgm_head(bytes(body[:1 + 2 * 255]), has_head)[1]


def _parse_pgm_table(body, cur):
    """<I T> <T x I length> streams from ``cur`` to the end of the body -> list of T streams."""
    if cur + 4 > len(body):
        raise ValueError("truncated body: stream count missing")
    (total,) = struct.unpack("<I", body[cur:cur + 4])
    cur += 4
    if cur + 4 * total > len(body):
        raise ValueError("truncated body: stream length table cut short")
    lens = struct.unpack("<%dI" % total, body[cur:cur + 4 * total])
    cur += 4 * total
    streams = []
    for L in lens:
        if cur + L > len(body):
            raise ValueError("truncated body: stream shorter than its length")
        streams.append(body[cur:cur + L])
        cur += L
    if cur != len(body):
        raise ValueError(f"body holds {len(body) - cur} bytes after its last stream")
    return streams


def _write_pgm_table(streams):
    return b"".join([struct.pack("<I", len(streams)), struct.pack("<%dI" % len(streams), *[len(s) for s in streams])] + list(streams))


def split_pgm_body(body, n, has_head=False, item_tabled=False) -> List[bytes]:
    """The n item bodies of a PGM body that holds n images.  ``has_head``: the coder writes the shape head (no fixed input shape, no
    aligned prior); ``item_tabled``: what the coder's ``_per_image(1)`` says -- a batch of one is written with the stream table
    (explicit "per_image", lanes, rows) rather than as the bare stream ("auto")."""
    body, n = bytes(body), int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    batch, dims, cur = _pgm_head(body, has_head)
    if has_head and batch != n:
        raise ValueError(f"the shape head states a batch of {batch}, not {n}")
    if n == 1 and not item_tabled:   # a batch of one under "auto" is the bare stream: the item form already
        if len(body) == cur:
            raise ValueError("truncated body: no stream")
        return [body]
    streams = _parse_pgm_table(body, cur)
    if len(streams) == 0 or len(streams) % n:
        raise ValueError(f"{len(streams)} streams do not divide among {n} items")
    S = len(streams) // n
    if S != 1 and not item_tabled:
        raise ValueError(f"{S} streams per item need the tabled item form")
    head = _write_pgm_head(1, dims) if has_head else b""
    return [head + (_write_pgm_table(streams[i * S:(i + 1) * S]) if item_tabled else streams[i * S]) for i in range(n)]


def merge_pgm_bodies(bodies, has_head=False, item_tabled=False) -> bytes:
    """Inverse of split_pgm_body: item bodies -> the body ``_encode_impl`` writes for the batch of them."""
    bodies = [bytes(b) for b in bodies]
    if not bodies:
        raise ValueError("no bodies to merge")
    shape, streams, S = None, [], None
    for b in bodies:
        batch, dims, cur = _pgm_head(b, has_head)
        if has_head:
            if batch != 1:
                raise ValueError(f"an item body states a batch of 1, not {batch}")
            if shape is None:
                shape = dims
            elif shape != dims:
                raise ValueError(f"bodies of different shapes: {shape} and {dims}")
        if item_tabled:
            mine = _parse_pgm_table(b, cur)
            if not mine:
                raise ValueError("an item body holds at least one stream")
        else:
            if len(b) == cur:
                raise ValueError("truncated body: no stream")
            mine = [b[cur:]]
        if S is None:
            S = len(mine)
        elif S != len(mine):
            raise ValueError(f"bodies of {S} and of {len(mine)} streams")
        streams.extend(mine)
    if len(bodies) == 1:
        return bodies[0]
    return (_write_pgm_head(len(bodies), shape) if has_head else b"") + _write_pgm_table(streams)


# ---------------------------------------------------------------- whole-codec strings
def empty_split(body, n, **ctx) -> List[bytes]:
    """Splitter of a node that carries no bits (LossyDummyEntropyCoder)."""
    if len(body):
        raise ValueError("a node without bits has an empty body")
    return [b""] * int(n)


def empty_merge(bodies, **ctx) -> bytes:
    if any(len(b) for b in bodies):
        raise ValueError("a node without bits has an empty body")
    return b""


def split_codec_string(data, n, splitters: Sequence[Callable]) -> List[bytes]:
    """A codec's string of n images (merge_bytes over the nodes' bodies) -> its n item strings.  splitters[k](body, n) splits node k's
    body."""
    K = len(splitters)
    segs = split_merged_bytes(bytes(data), num_segments=K)
    per_node = [list(f(seg, n)) for f, seg in zip(splitters, segs)]
    for k, parts in enumerate(per_node):
        if len(parts) != n:
            raise ValueError(f"node {k}: {len(parts)} item bodies for {n} items")
    return [merge_bytes([per_node[k][i] for k in range(K)], num_segments=K) for i in range(n)]


def merge_codec_strings(strings, mergers: Sequence[Callable]) -> bytes:
    """Inverse of split_codec_string.  mergers[k](bodies) merges node k's item bodies."""
    K = len(mergers)
    segs = [split_merged_bytes(bytes(s), num_segments=K) for s in strings]
    return merge_bytes([f([sg[k] for sg in segs]) for k, f in enumerate(mergers)], num_segments=K)
