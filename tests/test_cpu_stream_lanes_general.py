"""Lane streams for every y coder (stream_lanes = K, INTEGRATION.md "Lane streams"), the parts that need no GPU: the lane rule as
plain NumPy (test_gpu_stream_lanes_general.py holds the pack kernel and the streams against it), what the constructors and the
calls refuse, the S-streams-per-item framing of CompressAI bodies, and the C entries the format adds."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from test_cpu_stream_lanes import lane_permutation_numpy


def lane_index_lists(bases, lanes):
    """The format's statement of a lane: the image's coding order is cut into steps [bases[g], bases[g + 1]); lane k of a step is the
    k-th of ``lanes`` equal contiguous parts of it, and stream k carries, step after step, lane k's part.  -> int64 [lanes, n / lanes]:
    row k = the coding-order element numbers of stream k.  ValueError when a step does not divide."""
    bases = [int(b) for b in bases]
    rows = [[] for _ in range(lanes)]
    for g in range(len(bases) - 1):
        n_g = bases[g + 1] - bases[g]
        if n_g % lanes:
            raise ValueError(f"step {g} of {n_g} elements does not divide into {lanes} lanes")
        part = n_g // lanes
        for k in range(lanes):
            rows[k].extend(range(bases[g] + k * part, bases[g] + (k + 1) * part))
    return np.asarray(rows, dtype=np.int64).reshape(lanes, -1)


def plan_bases(method, channel_groups, channels, h, w):
    """Group bases of a default plan, from the topo-group ids alone (pgm_coder._GroupPlan's rule: group g = the elements c * HW + p
    with id g, ascending)."""
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import default_topo_groups
    topo = default_topo_groups(method, channel_groups, h, w)
    full = np.repeat(topo, channels // topo.shape[0], axis=0).reshape(-1)
    counts = [int((full == g).sum()) for g in range(int(topo.max()) + 1)]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@pytest.mark.parametrize("bases,K", [((0, 6, 16, 18), 2), ((0, 192), 1), ((0, 192), 64), (tuple(range(0, 1201, 4)), 4), ((0, 0, 8, 8, 12), 4)])
def test_lane_rule(bases, K):
    rows = lane_index_lists(bases, K)
    n = bases[-1]
    assert rows.shape == (K, n // K)
    assert np.array_equal(np.sort(rows.reshape(-1)), np.arange(n))          # a permutation of the image
    assert all(bool((np.diff(r) > 0).all()) for r in rows)                  # a lane is a subsequence of the K = 1 order
    if K == 1:
        assert np.array_equal(rows[0], np.arange(n))
    # every step contributes equally to every stream, in step order
    at = 0
    for g in range(len(bases) - 1):
        part = (bases[g + 1] - bases[g]) // K
        for k in range(K):
            assert rows[k][at: at + part].tolist() == list(range(bases[g] + k * part, bases[g] + (k + 1) * part))
        at += part


def test_lane_rule_small_example_and_errors():
    assert lane_index_lists((0, 6, 16, 18), 2).tolist() == [[0, 1, 2, 6, 7, 8, 9, 10, 16], [3, 4, 5, 11, 12, 13, 14, 15, 17]]
    with pytest.raises(ValueError):
        lane_index_lists((0, 6, 16, 18), 4)
    with pytest.raises(ValueError):
        lane_index_lists((0, 192), 5)


@pytest.mark.parametrize("P,K", [(1, 1), (6, 2), (5, 12), (7, 4)])
def test_scanline_lanes_are_the_same_rule(P, K):
    """Step = position, list = channels: the general rule restates the scan-line coder's lanes."""
    C = 192
    assert np.array_equal(lane_index_lists(np.arange(P + 1) * C, K), lane_permutation_numpy(P, C, K))


@pytest.mark.parametrize("method,K", [("checkerboard", 2), ("checkerboard", 4), ("raster2x2", 4), ("none", 64)])
def test_spatial_groups_with_k_dividing_c_are_channel_lanes(method, K):
    """Spatial-only groups and K | C: lane k is channels [k L, (k + 1) L) of every step -- the scan-line picture."""
    C, H, W = 192, 4, 6
    bases = plan_bases(method, 1, C, H, W)
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import default_topo_groups
    topo = default_topo_groups(method, 1, H, W).reshape(-1)
    order = np.concatenate([np.nonzero(np.repeat(topo[None], C, 0).reshape(-1) == g)[0] for g in range(int(topo.max()) + 1)])
    rows = lane_index_lists(bases, K)
    L = C // K
    for k in range(K):
        ch = order[rows[k]] // (H * W)
        assert ch.min() == k * L and ch.max() == (k + 1) * L - 1


def _pgm_coder(**kw):
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder
    kw.setdefault("in_channels", 192)
    return Coder(**kw)


def _gc_coder(**kw):
    from cbench_basic_amd.modules.prior_model.prior_coder.compressai_coder import CompressAIGaussianConditionalCoder
    return CompressAIGaussianConditionalCoder(**kw)


@pytest.mark.parametrize("method,G", [("checkerboard", 1), ("raster2x2", 1), ("channelwise", 4), ("elic", 1), ("none", 1), ("zigzag", 1),
                                      ("channelwise-g10", 1), ("checkerboard", 2)])
@pytest.mark.parametrize("K", [1, 2, 4, 16, 64, 256])
def test_every_method_takes_lanes(method, G, K):
    c = _pgm_coder(default_topo_group_method=method, channel_groups=G, stream_lanes=K)
    assert c.stream_lanes == K
    assert c._per_image(1) == (K > 1)      # lanes use the tabled per-image framing at every batch size
    assert c.can_split_items


@pytest.mark.parametrize("K", [1, 2, 3, 16, 64, 256])
def test_gaussian_conditional_takes_lanes(K):
    c = _gc_coder(stream_lanes=K)
    assert c.stream_lanes == K and _gc_coder().stream_lanes == 1


@pytest.mark.parametrize("bad", [0, -1, 257, 1000, 2.0, "4", None, True])
def test_lane_count_must_be_an_integer_in_range(bad):
    with pytest.raises(ValueError, match="stream_lanes"):
        _gc_coder(stream_lanes=bad)
    with pytest.raises(ValueError, match="stream_lanes"):
        _pgm_coder(default_topo_group_method="checkerboard", stream_lanes=bad)
    with pytest.raises(ValueError, match="stream_lanes"):
        _pgm_coder(default_topo_group_method="scanline", stream_lanes=bad)


@pytest.mark.parametrize("method,G", [("checkerboard", 1), ("none", 1), ("elic", 1), ("channelwise", 4), ("raster2x2", 1)])
@pytest.mark.parametrize("K", [3, 6, 12, 24, 96, 255])
def test_other_methods_take_powers_of_two_only(method, G, K):
    """Outside the scan-line schedule a lane count that is no power of two stays refused at construction (3 lanes on a checkerboard
    coder were refused before this format reached it, test_cpu_stream_lanes.py)."""
    with pytest.raises(ValueError, match="stream_lanes"):
        _pgm_coder(default_topo_group_method=method, channel_groups=G, stream_lanes=K)


def test_scanline_rules_are_unchanged():
    for kw in (dict(stream_lanes=8), dict(stream_lanes=5), dict(stream_lanes=24), dict(stream_lanes=3, channel_groups=2),
               dict(stream_lanes=2, in_channels=48)):
        with pytest.raises(ValueError, match="stream_lanes"):
            _pgm_coder(default_topo_group_method="scanline", **kw)
    for K in (1, 2, 3, 4, 6, 12):
        assert _pgm_coder(default_topo_group_method="scanline", stream_lanes=K).stream_lanes == K


@pytest.mark.parametrize("method", ["checkerboard", "none", "elic", "scanline"])
def test_reference_stream_mode_cannot_hold_lanes(method):
    with pytest.raises(ValueError, match="reference"):
        _pgm_coder(default_topo_group_method=method, batch_stream_mode="reference", stream_lanes=2)
    assert _pgm_coder(default_topo_group_method=method, batch_stream_mode="reference", stream_lanes=1).stream_lanes == 1


def test_a_call_with_a_pgm_or_per_sample_plans_is_refused_before_anything_runs():
    import torch
    c = _pgm_coder(default_topo_group_method="checkerboard", stream_lanes=2)
    for pgm in (torch.zeros(1, 1, 2, 2, dtype=torch.long), torch.zeros(3, 1, 2, 2, dtype=torch.long)):   # one map; a map per sample
        with pytest.raises(ValueError, match="pgm"):
            c._encode_impl(torch.zeros(pgm.shape[0], 192, 2, 2), pgm=pgm)
        with pytest.raises(ValueError, match="pgm"):
            c._decode_impl(b"\0" * 64, pgm=pgm)
        with pytest.raises(ValueError, match="pgm"):
            c.encode(torch.zeros(pgm.shape[0], 192, 2, 2), pgm=pgm)


def test_a_step_that_does_not_divide_is_refused_per_call():
    import torch
    # checkerboard at 3 x 3: steps of 5 * 192 = 960 and 4 * 192 = 768 elements
    c = _pgm_coder(default_topo_group_method="checkerboard", stream_lanes=256)
    assert plan_bases("checkerboard", 1, 192, 3, 3).tolist() == [0, 960, 1728]
    with pytest.raises(ValueError, match="does not divide"):
        c._encode_impl(torch.zeros(1, 192, 3, 3))
    head = struct.pack("B", 3) + struct.pack("<3H", 1, 3, 3)
    with pytest.raises(ValueError, match="does not divide"):
        c._decode_impl(head + b"\0" * 64)
    c._check_lanes_steps(4, 4)                 # 8 * 192 = 1536 = 6 * 256: this shape divides
    c = _pgm_coder(default_topo_group_method="checkerboard", stream_lanes=128)
    with pytest.raises(ValueError, match="does not divide"):
        c._check_lanes_steps(3, 3)
    c._check_lanes_steps(4, 4)
    # elic: 16-channel groups x checkerboard halves: 16 * 8 = 128 elements in the smallest step at 4 x 4
    c = _pgm_coder(default_topo_group_method="elic", stream_lanes=4)
    c._check_lanes_steps(4, 4)
    c = _pgm_coder(default_topo_group_method="elic", stream_lanes=32)      # 16 channels x 5 or 4 positions at 3 x 3
    with pytest.raises(ValueError, match="does not divide"):
        c._check_lanes_steps(3, 3)
    # GaussianConditional: the whole image is one step
    g = _gc_coder(stream_lanes=64)
    assert g._lane_length(192 * 4 * 4) == 48 and g._lane_length(192) == 3
    with pytest.raises(ValueError, match="does not divide"):
        g._lane_length(192 * 4 * 4 + 32)
    with pytest.raises(ValueError, match="does not divide"):
        _gc_coder(stream_lanes=5)._lane_length(192)


def test_a_body_of_another_stream_count_is_refused():
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import parse_stream_lengths
    streams = [bytes([i + 1]) * 8 for i in range(8)]
    body = struct.pack("<I", 8) + b"".join(struct.pack("<I", len(s)) for s in streams) + b"".join(streams)
    assert parse_stream_lengths(body, 8)[0].tolist() == [8] * 8      # B * K = 2 * 4
    for wrong in (2, 4, 6, 16):
        with pytest.raises(ValueError, match="streams"):
            parse_stream_lengths(body, wrong)


# ---------------------------------------------------------------- item framing
def _cai_body(h, w, streams):
    return struct.pack(">3I", h, w, len(streams)) + b"".join(struct.pack(">I", len(s)) + s for s in streams)


@pytest.mark.parametrize("S", [1, 2, 4, 64])
@pytest.mark.parametrize("n", [1, 3])
def test_compressai_item_framing_with_s_streams_per_item(S, n):
    from cbench_basic_amd.utils import item_framing as F
    rng = np.random.default_rng(10 * S + n)
    streams = [rng.integers(0, 256, 4 * int(rng.integers(2, 9)), dtype=np.uint8).tobytes() for _ in range(n * S)]
    body = _cai_body(5, 7, streams)
    parts = F.split_compressai_body(body, S)
    assert len(parts) == n
    for i, p in enumerate(parts):
        assert p == _cai_body(5, 7, streams[i * S:(i + 1) * S])      # an item body: the same form with S streams, lane order kept
    assert F.merge_compressai_bodies(parts, S) == body                # split then merge is the identity
    assert F.split_compressai_body(F.merge_compressai_bodies(parts, S), S) == parts
    if S == 1:   # the one-stream form is what the functions did before they took S
        assert F.split_compressai_body(body) == parts == [_cai_body(5, 7, [s]) for s in streams]
        assert F.merge_compressai_bodies(parts) == body
    else:
        with pytest.raises(ValueError):      # an item of S streams is not an item of one
            F.merge_compressai_bodies(parts)
        with pytest.raises(ValueError):
            F.merge_compressai_bodies(parts, S + 1)
    if (n * S) % (S + 1):
        with pytest.raises(ValueError):
            F.split_compressai_body(body, S + 1)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            F.split_compressai_body(body, bad)
        with pytest.raises(ValueError):
            F.merge_compressai_bodies(parts, bad)
    with pytest.raises(ValueError):
        F.merge_compressai_bodies(parts + [_cai_body(5, 8, streams[:S])], S)    # another (h, w)


@pytest.mark.parametrize("K", [1, 4])
def test_coder_item_framing_follows_its_lanes(K):
    c = _gc_coder(stream_lanes=K)
    streams = [bytes([i + 1]) * (8 + 4 * i) for i in range(3 * K)]
    body = _cai_body(4, 4, streams)
    parts = c.split_items(body, 3)
    assert parts == [_cai_body(4, 4, streams[i * K:(i + 1) * K]) for i in range(3)]
    assert c.merge_items(parts) == body
    assert [c.item_shape(p) for p in parts] == [(4, 4)] * 3
    with pytest.raises(ValueError):
        c.split_items(body, 2)
    with pytest.raises(ValueError):
        c.item_shape(_cai_body(4, 4, streams[: K + 1]))
    # the z coder beside it keeps one stream per item
    from cbench_basic_amd.modules.prior_model.prior_coder.compressai_coder import CompressAIEntropyBottleneckPriorCoder
    z = CompressAIEntropyBottleneckPriorCoder(entropy_bottleneck_channels=8)
    assert z.stream_lanes == 1 and len(z.split_items(body, 3 * K)) == 3 * K


def test_pgm_item_framing_holds_k_streams_per_item():
    c = _pgm_coder(default_topo_group_method="checkerboard", stream_lanes=4)
    streams = [bytes([i + 1]) * (8 + 4 * i) for i in range(12)]
    table = lambda ss: struct.pack("<I", len(ss)) + struct.pack("<%dI" % len(ss), *[len(s) for s in ss]) + b"".join(ss)
    body = table(streams)
    parts = c.split_items(body, 3, has_prior=True)
    assert parts == [table(streams[i * 4:(i + 1) * 4]) for i in range(3)]
    assert c.merge_items(parts, has_prior=True) == body


def test_presets_pass_the_lanes_to_the_y_coder():
    from cbench_basic_amd.presets import hyperprior_codec, topogroup_ar_codec
    for build in (hyperprior_codec, lambda **kw: topogroup_ar_codec("checkerboard", **kw), lambda **kw: topogroup_ar_codec("elic", **kw)):
        assert build().entropy_coder.latent_node_entropy_coders["y"].stream_lanes == 1
        codec = build(stream_lanes=4)
        assert codec.entropy_coder.latent_node_entropy_coders["y"].stream_lanes == 4
        assert getattr(codec.entropy_coder.latent_node_entropy_coders["z"], "stream_lanes", 1) == 1   # the z body keeps the reference's format
    with pytest.raises(ValueError):
        hyperprior_codec(stream_lanes=0)


def test_tool_takes_lanes_for_every_codec(monkeypatch, capsys):
    """--stream-lanes is no longer tied to --codec basic: the argument check passes for all three codecs (the run itself then stops
    where a machine without a GPU stops any run), and a count outside [1, 256] is an argument error."""
    import importlib.util
    import sys
    import torch
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "run_benchmark.py")
    spec = importlib.util.spec_from_file_location("run_benchmark_tool_lanes", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for codec in ("hyperprior", "topogroup", "basic"):
        monkeypatch.setattr(sys, "argv", ["run_benchmark.py", "--codec", codec, "--stream-lanes", "4", "--coalesce", "3", "--out", "unused"])
        with pytest.raises(SystemExit) as e:
            tool.main()
        assert e.value.code != 2 and "MI355X" in str(e.value.code)
    monkeypatch.setattr(sys, "argv", ["run_benchmark.py", "--stream-lanes", "257", "--out", "unused"])
    with pytest.raises(SystemExit) as e:
        tool.main()
    assert e.value.code == 2 and "--stream-lanes" in capsys.readouterr().err


def test_new_entries_are_declared_with_prototypes():
    from cbench_basic_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "basic_hip.h")).read()
    new = ["basic_group_lanes_pack_dev", "basic_hp_session_set_stream_lanes"]
    for name in new + ["basic_lanes_pack_dev", "basic_hp_decoded_shape", "basic_hp_session_set_rans_waves"]:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._SIGNATURES, name
    assert len(_lib._SIGNATURES["basic_group_lanes_pack_dev"][1]) == 10
    assert _lib._SIGNATURES["basic_hp_session_set_stream_lanes"] == _lib._SIGNATURES["basic_hp_session_set_rans_waves"]
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(lib, name) for name in new)
