"""Row streams of the scan-line y-coder (stream_rows = True, INTEGRATION.md "Row streams"), the parts that need no GPU: what the
constructor accepts, the row / lane permutation as plain NumPy (test_gpu_scanline_rows.py reuses it), the prototypes of the new
entries, and the size cap of the format confirmed with the CPU rANS oracle alone on every case of the GPU test."""
import ctypes
import os
import re

import numpy as np
import pytest

from scanline_exact import C, exact_case
from test_cpu_stream_lanes import SIZE_CAP_PER_STREAM, exact_ans_params, oracle_encoder

# (window, B, H, W) and lane count of test_gpu_scanline_rows.py's stream test: the wavefront decode cases, then the raster readers'
WAVEFRONT_CASES = [(5, 2, 7, 9), (5, 1, 16, 16), (3, 1, 4, 3), (5, 2, 3, 2), (5, 1, 1, 6), (5, 9, 7, 4), (5, 1, 33, 5)]
WAVEFRONT_CASES_K3 = [(5, 2, 7, 9), (5, 1, 5, 6)]
RASTER_CASES = [(5, 1, 5, 6), (5, 2, 7, 9), (5, 3, 5, 7), (5, 33, 2, 6)]
ROW_CASES = [(c, 1) for c in WAVEFRONT_CASES] + [(c, 3) for c in WAVEFRONT_CASES_K3] + [(c, k) for c in RASTER_CASES for k in (1, 3)]


def row_permutation_numpy(height, width, channels, lanes):
    """The format's statement of a stream: stream (r, k) of an image holds, position after position of row r, channels [k L, (k + 1) L)
    of the coding order (element p * C + c).  -> int64 [height * lanes, width * L]: row r * lanes + k = the coding-order element
    numbers of stream (r, k)."""
    L = channels // lanes
    rows = []
    for r in range(height):
        for k in range(lanes):
            rows.append([p * channels + c for p in range(r * width, (r + 1) * width) for c in range(k * L, (k + 1) * L)])
    return np.asarray(rows, dtype=np.int64)


def oracle_row_streams(enc, sym, idx, height, width, channels, lanes):
    """[B][H * K] bytes: what the CPU rANS oracle writes for every (row, lane) stream of every image of sym / idx int32 [B, H * W * C]."""
    perm = row_permutation_numpy(height, width, channels, lanes)
    return [[enc.encode_with_indexes(np.ascontiguousarray(sym[b][row]), np.ascontiguousarray(idx[b][row])) for row in perm]
            for b in range(sym.shape[0])]


def case_of(ks, B, H, W):
    return exact_case(ks, B, H, W, 1000 * B + 10 * H + W)


def _coder(**kw):
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder
    kw.setdefault("in_channels", 192)
    kw.setdefault("default_topo_group_method", "scanline")
    return Coder(**kw)


def test_constructor_accepts():
    assert _coder().stream_rows is False
    assert _coder(stream_rows=True).stream_rows is True
    assert _coder(stream_rows=True, stream_lanes=3).stream_rows is True
    assert _coder(stream_rows=True, batch_stream_mode="per_image").stream_rows is True
    assert _coder(use_joint_ar_model_impl=True, default_topo_group_method="none", stream_rows=True).stream_rows is True
    c = _coder(stream_rows=True)
    assert c._per_image(1) and c._per_image(5)   # the per-image framing at every batch size


@pytest.mark.parametrize("kw", [dict(default_topo_group_method="checkerboard"), dict(default_topo_group_method="none"), dict(channel_groups=2),
                                dict(batch_stream_mode="reference")])
def test_constructor_refuses_and_false_is_allowed_everywhere(kw):
    with pytest.raises(ValueError, match="stream_rows"):
        _coder(stream_rows=True, **kw)
    assert _coder(stream_rows=False, **kw).stream_rows is False   # no configuration that was valid before is refused


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 2.0])
def test_constructor_wants_a_bool(bad):
    with pytest.raises(ValueError, match="stream_rows"):
        _coder(stream_rows=bad)


def test_a_call_with_a_pgm_is_refused_before_anything_runs():
    import torch
    c = _coder(stream_rows=True)
    pgm = torch.zeros(1, 1, 2, 2, dtype=torch.long)
    with pytest.raises(ValueError, match="pgm"):
        c._encode_impl(torch.zeros(1, 192, 2, 2), pgm=pgm)
    with pytest.raises(ValueError, match="pgm"):
        c._decode_impl(b"\0" * 64, pgm=pgm)
    with pytest.raises(ValueError, match="pgm"):
        c.encode(torch.zeros(1, 192, 2, 2), pgm=pgm)
    with pytest.raises(ValueError, match="pgm"):
        c.decode(b"\0" * 64, pgm=pgm)


@pytest.mark.parametrize("B,H,W,K", [(1, 1, 1, 1), (1, 3, 4, 1), (2, 3, 4, 3), (3, 2, 5, 12), (1, 5, 1, 2), (2, 1, 6, 4)])
def test_row_lane_permutation(B, H, W, K):
    """The statement of a stream that the GPU tests hold the streams against is the lane pack with batch := B * H and positions := W,
    reshape(B H, W, K, L).transpose(0, 2, 1, 3): a permutation, every stream a subsequence of the coding order; K = 1 moves nothing."""
    L = C // K
    n = H * W * C
    want = row_permutation_numpy(H, W, C, K)
    assert want.shape == (H * K, W * L)
    elems = np.arange(B * n, dtype=np.int64)
    got = elems.reshape(B * H, W, K, L).transpose(0, 2, 1, 3).reshape(B, H * K, W * L)
    for b in range(B):
        assert np.array_equal(got[b], b * n + want)
    assert np.array_equal(np.sort(got.reshape(-1)), elems)
    assert all(bool((np.diff(row) > 0).all()) for row in want)   # a stream keeps the coding order
    if K == 1:
        assert np.array_equal(got.reshape(-1), elems)
    for r in range(H):
        for k in range(K):
            row = want[r * K + k]
            assert (row // C).min() == r * W and (row // C).max() == (r + 1) * W - 1
            assert (row % C).min() == k * L and (row % C).max() == (k + 1) * L - 1


def test_new_entries_are_declared_with_prototypes():
    from cbench_basic_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "basic_hip.h")).read()
    new = ["basic_scanline_decode_rows_dev", "basic_scanline_choose_rows", "basic_rans_decode_batch_streams_dev"]
    for name in new + ["basic_scanline_decode_lanes_dev", "basic_scanline_choose_lanes", "basic_rans_decode_batch_lanes_dev"]:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._SIGNATURES, name
    sig = _lib._SIGNATURES
    assert sig["basic_scanline_decode_rows_dev"] == sig["basic_scanline_decode_lanes_dev"]   # the lanes entry's argument list
    assert len(sig["basic_scanline_choose_rows"][1]) == len(sig["basic_scanline_choose_lanes"][1]) + 1
    assert len(sig["basic_rans_decode_batch_streams_dev"][1]) == len(sig["basic_rans_decode_batch_lanes_dev"][1]) + 2   # base and stride
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(lib, name) for name in new)


def test_size_cap_holds_for_the_oracle():
    """The format's size cap, with the oracle alone: on every case and lane count of the GPU test the row-stream body --
    <I B H K> <B H K x I length> streams -- is at most 16 bytes per stream longer than the K = 1, rows-off body of the same call (one
    bare stream at batch 1, <I B> <B x I length> streams above): 4 of length field, at most 8 of flushed state, 4 of word rounding."""
    enc = oracle_encoder(exact_ans_params())   # (the tables come from the scale table alone: the same for both windows)
    worst = 0.0
    for (ks, B, H, W), K in ROW_CASES:
        _, _, ref = case_of(ks, B, H, W)
        one = [enc.encode_with_indexes(np.ascontiguousarray(ref["sym"][b]), np.ascontiguousarray(ref["idx"][b])) for b in range(B)]
        body1 = len(one[0]) if B == 1 else 4 + 4 * B + sum(len(s) for s in one)
        rows = oracle_row_streams(enc, ref["sym"], ref["idx"], H, W, C, K)
        n = B * H * K
        assert sum(len(img) for img in rows) == n
        bodyr = 4 + 4 * n + sum(len(s) for img in rows for s in img)
        extra = (bodyr - body1) / n
        worst = max(worst, extra)
        print(f"k={ks} B={B} {H}x{W} K={K}: plain body {body1} bytes, row-stream body {bodyr}, {extra:.2f} extra bytes per stream")
        assert bodyr - body1 <= SIZE_CAP_PER_STREAM * n
    print(f"worst: {worst:.2f} bytes per stream")
