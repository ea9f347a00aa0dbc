"""The BTQ1 container of utils/tiling.py -- a tiled picture coded under quantiser steps -- without a GPU: the round trip, every
malformed container refused, the older readers refusing the new magic, the exact framing size against containers assembled from
synthetic tile strings (utils/item_framing.py), and the NumPy restatement of the group select on hand-made curves."""
import struct

import numpy as np
import pytest

import tiled_rate_exact as TX
from cbench_basic_amd.utils import item_framing as IF
from cbench_basic_amd.utils import tiling
from cbench_basic_amd.utils.bytes_ops import merge_bytes

GRIDS = [dict(H=200, W=136, th=64, tw=64),                                  # plain, ragged edges
         dict(H=192, W=192, th=64, tw=64, overlap=(16, 16)),                # overlapped
         dict(H=136, W=200, th=64, tw=64, pad_to=(64, 64)),                 # padded
         dict(H=100, W=90, th=64, tw=32, overlap=(8, 4), pad_to=(16, 8)),   # both
         dict(H=10, W=10, th=64, tw=64)]                                    # one tile


def _grid(g):
    return tiling.TileGrid(g["H"], g["W"], g["th"], g["tw"], g.get("overlap", (0, 0)), g.get("pad_to", (1, 1)))


def _strings(n, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes() for _ in range(n)]


@pytest.mark.parametrize("g", GRIDS)
def test_round_trip(g):
    grid = _grid(g)
    n = len(grid)
    strings = _strings(n)
    steps = np.exp2(np.random.default_rng(1).uniform(-4, 6, n)).astype(np.float32)
    steps[0], steps[-1] = 2.0 ** -4, 2.0 ** 6
    for given, want in ((steps, steps), (1.5, np.full(n, 1.5, np.float32)), ([0.25], np.full(n, 0.25, np.float32))):
        data = tiling.pack_tiled_q(3, g["H"], g["W"], g["th"], g["tw"], strings, given, overlap=grid.overlap, pad_to=grid.pad_to)
        assert data[:4] == b"BTQ1" == tiling.MAGIC_Q
        t = tiling.unpack_tiled_q(data)
        assert (t.channels, t.H, t.W, t.th, t.tw, t.overlap, t.pad_to) == (3, g["H"], g["W"], g["th"], g["tw"], grid.overlap, grid.pad_to)
        assert t.strings == strings and t.steps.dtype == np.float32 and np.array_equal(t.steps.view(np.int32), want.view(np.int32))
        assert tiling.unpack_tiled_q(memoryview(data)).strings == strings and tiling.unpack_tiled_q(bytearray(data)).strings == strings
    # the layout, field by field: the BTL3 head under the new magic, n float32 LE steps, n uint32 LE lengths, the strings
    data = tiling.pack_tiled_q(3, g["H"], g["W"], g["th"], g["tw"], strings, steps, overlap=grid.overlap, pad_to=grid.pad_to)
    head = struct.pack("<4sBIIIIIIIII", b"BTQ1", 3, g["H"], g["W"], g["th"], g["tw"], *grid.overlap, *grid.pad_to, n)
    assert data == head + steps.astype("<f4").tobytes() + struct.pack("<%dI" % n, *map(len, strings)) + b"".join(strings)
    btl3 = tiling.pack_tiled(3, g["H"], g["W"], g["th"], g["tw"], strings, overlap=grid.overlap, pad_to=(g["th"], g["tw"]))
    assert len(head) == 41 and btl3[:4] == b"BTL3" and len(btl3) == len(data) - 4 * n


def test_writer_refuses():
    g = GRIDS[0]
    n = len(_grid(g))
    ok = _strings(n)
    for steps in ([1.0] * (n - 1), [], float("nan"), float("inf"), 0.0, 2.0 ** -5, 65.0, [[1.0] * n], "x"):
        with pytest.raises(ValueError):
            tiling.pack_tiled_q(3, g["H"], g["W"], 64, 64, ok, steps)
    with pytest.raises(ValueError):
        tiling.pack_tiled_q(3, g["H"], g["W"], 64, 64, ok[:-1], 1.0)
    with pytest.raises(ValueError):
        tiling.pack_tiled_q(0, g["H"], g["W"], 64, 64, ok, 1.0)


@pytest.mark.parametrize("g", GRIDS[:4])
def test_reader_refuses_every_malformed_container(g):
    grid = _grid(g)
    n = len(grid)
    strings = [s + b"\x01" for s in _strings(n, 3)]          # no empty string: every cut removes something
    data = tiling.pack_tiled_q(3, g["H"], g["W"], g["th"], g["tw"], strings, 2.0, overlap=grid.overlap, pad_to=grid.pad_to)
    o_steps, o_lens, o_body = 41, 41 + 4 * n, 41 + 8 * n
    # truncated at each field: inside the magic, the head, the step table, the length table, the payload; and one byte short
    for cut in (0, 3, 4, 20, 40, o_steps, o_steps + 2, o_lens - 1, o_lens, o_lens + 3, o_body - 1, o_body, o_body + 1, len(data) - 1):
        with pytest.raises(ValueError):
            tiling.unpack_tiled_q(data[:cut])
    with pytest.raises(ValueError, match="after the last tile"):
        tiling.unpack_tiled_q(data + b"\x00")
    # a step that is not finite, or outside [2^-4, 2^6] -- in the first, a middle and the last slot
    for slot in sorted({0, n // 2, n - 1}):
        for bad in (float("nan"), float("inf"), -1.0, 0.0, 2.0 ** -5, 64.5):
            broken = bytearray(data)
            struct.pack_into("<f", broken, o_steps + 4 * slot, bad)
            with pytest.raises(ValueError, match="quantiser step"):
                tiling.unpack_tiled_q(bytes(broken))
    # a wrong n; lengths that do not add up (one more, one less); a zero dimension; an overlap and a padding the grid refuses
    for off, value in ((37, n + 1), (37, max(n - 1, 0)), (5, 0), (13, 0), (21, g["th"]), (29, 0), (29, g["th"] - 1 if g["th"] > 2 else 3)):
        broken = bytearray(data)
        struct.pack_into("<I", broken, off, value)
        with pytest.raises(ValueError):
            tiling.unpack_tiled_q(bytes(broken))
    for delta in (1, -1):
        broken = bytearray(data)
        struct.pack_into("<I", broken, o_lens, len(strings[0]) + delta)
        with pytest.raises(ValueError):
            tiling.unpack_tiled_q(bytes(broken))
    for magic in (b"BTL1", b"BTL2", b"BTL3", b"BTL4", b"BQS1", b"btq1"):
        with pytest.raises(ValueError, match="magic"):
            tiling.unpack_tiled_q(magic + data[4:])


def test_the_older_readers_still_refuse_the_new_magic():
    g = GRIDS[0]
    data = tiling.pack_tiled_q(3, g["H"], g["W"], 64, 64, _strings(len(_grid(g))), 1.0)
    for reader in (tiling.unpack_tiled, tiling.unpack_tiled_any, tiling.unpack_tiled_full):
        with pytest.raises(ValueError, match="magic"):
            reader(data)
    # and what they read is what it was: a step-less container is not a BTQ1 one
    plain = tiling.pack_tiled(3, g["H"], g["W"], 64, 64, _strings(len(_grid(g))))
    assert plain[:4] == b"BTL1" and tiling.unpack_tiled_full(plain).strings == _strings(len(_grid(g)))
    with pytest.raises(ValueError, match="magic"):
        tiling.unpack_tiled_q(plain)


def _tile_string(rng, h, w, streams_per_body):
    """A codec string of CompressAI-style bodies with random payloads -> (string, payload bytes)."""
    bodies, payload = [], 0
    for S in streams_per_body:
        streams = [rng.integers(0, 256, 4 * int(rng.integers(2, 30)), dtype=np.uint8).tobytes() for _ in range(S)]
        payload += sum(map(len, streams))
        bodies.append(IF._write_compressai(h, w, streams))
    return merge_bytes(bodies, num_segments=len(bodies)), payload


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("g", GRIDS)
def test_framing_bytes_are_exact(g, lanes):
    grid = _grid(g)
    rng = np.random.default_rng(lanes)
    made = [_tile_string(rng, 4, 4, [1, lanes]) for _ in range(len(grid))]
    data = tiling.pack_tiled_q(3, g["H"], g["W"], g["th"], g["tw"], [s for s, _ in made], 1.0, overlap=grid.overlap, pad_to=grid.pad_to)
    want = len(data) - sum(p for _, p in made)
    assert tiling.tiled_q_framing_bytes(grid, lanes) == want == tiling.tiled_q_framing_bytes(len(grid), stream_lanes=lanes, n_bodies=2)
    assert tiling.tiled_q_framing_bytes(grid, streams_per_body=[1, lanes]) == want
    # the strings split back into item bodies of the stated stream counts: the framing counted is the framing written
    for s, _ in made:
        assert IF.split_codec_string(s, 1, [lambda b, n: IF.split_compressai_body(b, 1), lambda b, n: IF.split_compressai_body(b, lanes)]) == [s]
    # by hand: 41 + n (4 + 4 + 4 + 12 + 4 + 12 + 4 lanes)
    assert want == 41 + len(grid) * (8 + 4 + 24 + 4 * (1 + lanes))
    # three bodies, the middle one of two streams
    made3 = [_tile_string(rng, 4, 4, [1, 2, lanes]) for _ in range(len(grid))]
    data3 = tiling.pack_tiled_q(3, g["H"], g["W"], g["th"], g["tw"], [s for s, _ in made3], 1.0, overlap=grid.overlap, pad_to=grid.pad_to)
    assert tiling.tiled_q_framing_bytes(grid, streams_per_body=[1, 2, lanes]) == len(data3) - sum(p for _, p in made3)
    assert tiling.tiled_q_framing_bytes(grid, lanes, n_bodies=1) == 41 + len(grid) * (8 + 12 + 4 * lanes)
    for bad in (dict(grid=0), dict(grid=grid, stream_lanes=0), dict(grid=grid, n_bodies=0), dict(grid=grid, streams_per_body=[])):
        with pytest.raises(ValueError):
            tiling.tiled_q_framing_bytes(**bad)


def test_item_framing_sizes():
    assert IF.compressai_body_framing(1) == len(IF._write_compressai(2, 2, [b""])) == 16
    assert IF.compressai_body_framing(4) == len(IF._write_compressai(2, 2, [b""] * 4)) == 28
    assert IF.compressai_string_framing([1, 4]) == len(merge_bytes([IF._write_compressai(2, 2, [b""]), IF._write_compressai(2, 2, [b""] * 4)],
                                                                   num_segments=2))


# ---- the restatement of the group select, on curves made by hand
def _bits_for(nbytes, per):
    """Curve entries whose stream bound is exactly ``nbytes`` (a multiple of 4, >= 8) for a stream of ``per`` symbols."""
    return ((nbytes // 4 - 2) << 21) - 4 * per


def test_group_select_by_hand():
    per = [1000, 10, 1000]                       # tile 1 is a small edge tile
    # tile 0: 400 / 200 / 100 bytes at the three candidates; tile 1: 40 / 80 / 16 (not monotone); tile 2, in no group
    bits = np.array([[_bits_for(v, per[t]) for v in row] for t, row in enumerate([[400, 200, 100], [40, 80, 16], [8, 8, 8]])], np.int64)
    cand = np.array([0.5, 1.0, 2.0], np.float32)
    extra = [3, 1, 0]                              # 12 and 4 bytes already spent
    run = lambda budget: TX.select_groups(bits, [0, 1, 2], 1, per, extra, [[1, 0]], cand, [budget])
    steps, choice, pred, ts, tp = run(296)         # candidate 1 predicts 200 + 80 + 16 = 296: fits exactly
    assert (steps[0], choice[0], pred[0]) == (1.0, 1, 296) and ts.tolist() == [1.0, 1.0, 1.0] and tp.tolist() == [212, 84, 0]
    steps, choice, pred, ts, tp = run(295)         # one byte less: the next candidate in order
    assert (steps[0], choice[0], pred[0]) == (2.0, 2, 132) and tp.tolist() == [112, 20, 0]
    steps, choice, pred, ts, tp = run(131)         # nothing fits: the largest step, flagged
    assert (steps[0], choice[0], pred[0]) == (2.0, 2 | TX.NO_FIT, 132) and ts.tolist() == [2.0, 2.0, 1.0]
    assert run(456)[1][0] == 0 and run(455)[1][0] == 1
    # two lanes: tile 0 owns rows 0 and 1, tile 1 rows 1 and 2
    s2 = TX.select_groups(bits, [0, 1], 2, [10, 10], None, [[0], [1]], np.stack([cand, cand * 2]), [10 ** 6, 0])
    assert s2[1].tolist() == [0, 2 | TX.NO_FIT] and s2[0].tolist() == [0.5, 4.0]
    assert s2[2][0] == TX.tile_pred(bits.tolist(), 0, 2, 10, 0, 0)
