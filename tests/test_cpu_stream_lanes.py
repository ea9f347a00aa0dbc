"""Lane streams of the scan-line y-coder (stream_lanes = K, INTEGRATION.md "Lane streams"), the parts that need no GPU: what the
constructor accepts, the body's framing parser, the lane permutation as plain NumPy (test_gpu_scanline_lanes.py reuses it), and
the size cap of test_gpu_scanline_lanes.py's size test confirmed with the CPU rANS oracle alone."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from scanline_exact import C, TABLE, exact_case

# (B, H, W) of test_gpu_scanline_lanes.py's stream test, and its lane counts
LANE_CASES = [(1, 5, 6), (2, 7, 9), (3, 5, 7), (33, 2, 6)]
LANE_COUNTS = (2, 3, 12)
SIZE_CAP_PER_STREAM = 16   # bytes: 4 of length field, at most 8 of flushed 64-bit state, 4 of word rounding


def lane_permutation_numpy(positions, channels, lanes):
    """The format's statement of a lane: lane k of an image holds, position after position, channels [k L, (k + 1) L) of the coding
    order (element p * C + c).  -> int64 [lanes, positions * L]: row k = the coding-order element numbers of lane k."""
    L = channels // lanes
    rows = []
    for k in range(lanes):
        rows.append([p * channels + c for p in range(positions) for c in range(k * L, (k + 1) * L)])
    return np.asarray(rows, dtype=np.int64)


def oracle_encoder(ans_params, precision=16, bypass=True, bypass_precision=4):
    from oracle.rans_oracle import Rans64Encoder
    enc = Rans64Encoder(precision, bypass, bypass_precision)
    enc.init_params(*ans_params)
    return enc


def oracle_lane_streams(enc, sym, idx, positions, channels, lanes):
    """[B][K] bytes: what the CPU rANS oracle writes for every lane of every image of sym / idx int32 [B, positions * channels]."""
    perm = lane_permutation_numpy(positions, channels, lanes)
    return [[enc.encode_with_indexes(np.ascontiguousarray(sym[b][perm[k]]), np.ascontiguousarray(idx[b][perm[k]])) for k in range(lanes)]
            for b in range(sym.shape[0])]


def exact_ans_params():
    """The rANS tables of the exact coder (scanline_exact.install: the 0.5-step scale table), as update_state builds them."""
    import torch
    from cbench_basic_amd.modules.prior_model.prior_coder.torch_ans import gaussian_ans_params
    return gaussian_ans_params(torch.from_numpy(TABLE.copy()), 16, 0.11)


def _coder(**kw):
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder
    kw.setdefault("in_channels", 192)
    kw.setdefault("default_topo_group_method", "scanline")
    return Coder(**kw)


@pytest.mark.parametrize("lanes", [1, 2, 3, 4, 6, 12])
def test_constructor_accepts_the_lane_counts_of_192_channels(lanes):
    assert _coder(stream_lanes=lanes).stream_lanes == lanes


def test_default_is_one_lane_and_joint_ar_is_served():
    assert _coder().stream_lanes == 1
    assert _coder(use_joint_ar_model_impl=True, default_topo_group_method="none", stream_lanes=3).stream_lanes == 3


@pytest.mark.parametrize("kw", [dict(stream_lanes=5), dict(stream_lanes=24), dict(stream_lanes=0), dict(stream_lanes=-3), dict(stream_lanes=2.0),
                                dict(stream_lanes=8),   # 192 / 8 = 24: not a multiple of 16
                                dict(stream_lanes=2, in_channels=48),   # lanes of 24
                                dict(stream_lanes=3, default_topo_group_method="checkerboard"),
                                dict(stream_lanes=3, default_topo_group_method="none"),
                                dict(stream_lanes=3, channel_groups=2),
                                dict(stream_lanes=3, batch_stream_mode="reference")])
def test_constructor_refuses(kw):
    with pytest.raises(ValueError):
        _coder(**kw)


def test_one_lane_is_allowed_everywhere():
    """K = 1 is the reference's format: no configuration that was valid before is refused."""
    assert _coder(default_topo_group_method="checkerboard", stream_lanes=1).stream_lanes == 1
    assert _coder(channel_groups=2, stream_lanes=1).stream_lanes == 1
    assert _coder(batch_stream_mode="reference", stream_lanes=1).stream_lanes == 1


def test_a_call_with_a_pgm_is_refused_before_anything_runs():
    import torch
    c = _coder(stream_lanes=3)
    pgm = torch.zeros(1, 1, 2, 2, dtype=torch.long)
    with pytest.raises(ValueError, match="pgm"):
        c._encode_impl(torch.zeros(1, 192, 2, 2), pgm=pgm)
    with pytest.raises(ValueError, match="pgm"):
        c._decode_impl(b"\0" * 64, pgm=pgm)


def test_framing_parser():
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import parse_stream_lengths
    streams = [b"\1" * 8, b"\2" * 12, b"\3" * 8, b"\4" * 16, b"\5" * 8, b"\6" * 20]
    body = struct.pack("<I", 6) + b"".join(struct.pack("<I", len(s)) for s in streams) + b"".join(streams)
    lens, payload = parse_stream_lengths(body, 6)
    assert lens.dtype == np.int64 and lens.tolist() == [8, 12, 8, 16, 8, 20] and payload == 4 + 4 * 6
    at = payload
    for s, n in zip(streams, lens):
        assert body[at: at + n] == s
        at += int(n)
    assert at == len(body)
    lens, payload = parse_stream_lengths(memoryview(body), 6)   # the decoder reads through the buffer protocol
    assert lens.tolist() == [8, 12, 8, 16, 8, 20]
    for wrong in (1, 2, 3, 5, 7, 12):   # B * K is configuration: a body of another count is another coder's
        with pytest.raises(ValueError, match="streams"):
            parse_stream_lengths(body, wrong)
    with pytest.raises(ValueError):
        parse_stream_lengths(b"", 6)
    with pytest.raises(ValueError):
        parse_stream_lengths(body[:3], 6)
    with pytest.raises(ValueError):
        parse_stream_lengths(body[:4 + 4 * 6 - 1], 6)   # the length fields are cut short


@pytest.mark.parametrize("P,K", [(1, 1), (6, 1), (6, 2), (6, 3), (5, 12), (7, 4), (3, 6)])
def test_lane_permutation(P, K):
    """The statement of a lane that the GPU tests hold the pack kernel and the streams against: it is the [P][K][L] -> [K][P][L]
    transposition, a permutation, every lane keeps the coding order, K = 1 is the identity."""
    want = lane_permutation_numpy(P, C, K)
    got = np.arange(P * C, dtype=np.int64).reshape(P, K, C // K).transpose(1, 0, 2).reshape(-1)
    assert want.shape == (K, P * C // K) and np.array_equal(got.reshape(K, -1), want)
    assert np.array_equal(np.sort(got), np.arange(P * C))
    assert all(bool((np.diff(row) > 0).all()) for row in want)   # a lane is a subsequence of the K = 1 order
    if K == 1:
        assert np.array_equal(got, np.arange(P * C))
    L = C // K
    for k in range(K):
        ch = want[k] % C
        assert ch.min() == k * L and ch.max() == (k + 1) * L - 1


def test_size_cap_holds_for_the_oracle():
    """The size test's cap, confirmed on the CPU with the oracle alone: on every case and lane count of the GPU test, the K-lane
    body -- <I B K> <B K x I length> streams -- is at most 16 bytes per lane stream longer than the K = 1 body of the same call (one
    bare stream at batch 1, <I B> <B x I length> streams above)."""
    enc = oracle_encoder(exact_ans_params())
    worst = 0.0
    for B, H, W in LANE_CASES:
        _, _, ref = exact_case(5, B, H, W, 1000 * B + 10 * H + W)
        one = oracle_lane_streams(enc, ref["sym"], ref["idx"], H * W, C, 1)
        body1 = len(one[0][0]) if B == 1 else 4 + 4 * B + sum(len(s[0]) for s in one)
        for K in LANE_COUNTS:
            lanes = oracle_lane_streams(enc, ref["sym"], ref["idx"], H * W, C, K)
            bodyk = 4 + 4 * B * K + sum(len(s) for img in lanes for s in img)
            extra = (bodyk - body1) / (B * K)
            worst = max(worst, extra)
            print(f"B={B} {H}x{W} K={K}: K = 1 body {body1} bytes, lane body {bodyk}, {extra:.2f} extra bytes per lane stream")
            assert bodyk - body1 <= SIZE_CAP_PER_STREAM * B * K
    print(f"worst: {worst:.2f} bytes per lane stream")


def test_new_entries_are_declared_with_prototypes():
    """Every entry the lane format adds to include/basic_hip.h has a ctypes prototype (and, when the library is built, is exported);
    the entries they generalise are still there with their signatures."""
    from cbench_basic_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "basic_hip.h")).read()
    new = ["basic_scanline_decode_lanes_dev", "basic_scanline_choose_lanes", "basic_rans_decode_batch_lanes_dev", "basic_lanes_pack_dev"]
    for name in new + ["basic_scanline_decode_dev", "basic_scanline_choose", "basic_rans_decode_batch_strided_dev"]:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._SIGNATURES, name
    assert len(_lib._SIGNATURES["basic_scanline_decode_lanes_dev"][1]) == len(_lib._SIGNATURES["basic_scanline_decode_dev"][1]) + 1
    assert len(_lib._SIGNATURES["basic_scanline_choose_lanes"][1]) == len(_lib._SIGNATURES["basic_scanline_choose"][1]) + 1
    assert len(_lib._SIGNATURES["basic_rans_decode_batch_lanes_dev"][1]) == len(_lib._SIGNATURES["basic_rans_decode_batch_strided_dev"][1]) + 1
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(lib, name) for name in new)
