"""Lane streams for every y coder (stream_lanes = K > 1, INTEGRATION.md "Lane streams") on the GPU: the pack kernel against the
NumPy statement of the lane rule (test_cpu_stream_lanes_general.lane_index_lists), and for the GaussianConditional coder, the fused
hyperprior session, the topo-group coders and the harness: stream (b, k) is byte for byte what the CPU rANS oracle writes for that
slice of the K = 1 symbols and indexes on the coder's own tables, the decoder gives the K = 1 latent exactly, K = 1 writes today's
bytes, and an item's lanes do not depend on the batch it is coded in."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest
import torch

from test_cpu_stream_lanes_general import lane_index_lists, plan_bases

pytestmark = pytest.mark.gpu


def _cai_streams(body):
    from cbench_basic_amd.utils.item_framing import _parse_compressai
    return _parse_compressai(body)


def _cai_body(h, w, streams):
    return struct.pack(">3I", h, w, len(streams)) + b"".join(struct.pack(">I", len(s)) + s for s in streams)


def _pgm_streams(body, nstreams):
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import parse_stream_lengths
    lens, at = parse_stream_lengths(body, nstreams)
    out = []
    for n in lens:
        out.append(bytes(body[at: at + int(n)]))
        at += int(n)
    assert at == len(body)
    return out


# ---------------------------------------------------------------- 1. the pack kernel
PACK_CASES = [("unequal", (0, 6, 16, 18), 2), ("one-group", (0, 192), 1), ("one-group", (0, 192), 64),
              ("300x4", tuple(range(0, 1201, 4)), 4), ("empty-groups", (0, 0, 8, 8, 12, 12), 4),
              ("checkerboard", None, 2), ("checkerboard", None, 4), ("checkerboard", None, 64), ("checkerboard", None, 1)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,bases,K", PACK_CASES)
def test_pack_kernel_is_the_lane_rule(name, bases, K, B):
    from cbench_basic_amd.nn import kernels
    if bases is None:
        bases = plan_bases("checkerboard", 1, 192, 4, 4)
        assert bases.tolist() == [0, 1536, 3072]
    bases = np.asarray(bases, dtype=np.int64)
    n = int(bases[-1])
    rng = np.random.default_rng(n + 7 * K + B)
    sym = rng.integers(-1000, 1000, (B, n)).astype(np.int32)
    idx = rng.integers(0, 64, (B, n)).astype(np.int32)
    rows = lane_index_lists(bases, K)
    so, io = kernels.group_lanes_pack(torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(bases).cuda(), K)
    assert so.shape == io.shape == (B * K, n // K) and so.dtype == io.dtype == torch.int32
    so, io = so.cpu().numpy(), io.cpu().numpy()
    for b in range(B):
        for k in range(K):
            assert np.array_equal(so[b * K + k], sym[b][rows[k]]), (name, b, k)
            assert np.array_equal(io[b * K + k], idx[b][rows[k]]), (name, b, k)
    if K == 1:
        assert np.array_equal(so, sym) and np.array_equal(io, idx)      # a copy


def test_pack_entry_refuses_bad_arguments():
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels
    L = _lib.lib()
    a = torch.zeros((1, 192), dtype=torch.int32, device="cuda")
    b, c, d = torch.zeros_like(a), torch.zeros_like(a), torch.zeros_like(a)
    bases = torch.tensor([0, 192], dtype=torch.int64, device="cuda")
    st = kernels._stream()
    for lanes in (0, -1, 257, 5):      # outside [1, 256]; 5 does not divide 192
        with pytest.raises(ValueError):
            _lib.check(L.basic_group_lanes_pack_dev(a.data_ptr(), b.data_ptr(), 1, 192, bases.data_ptr(), 1, lanes, c.data_ptr(), d.data_ptr(), st))
    with pytest.raises(ValueError):    # in place
        _lib.check(L.basic_group_lanes_pack_dev(a.data_ptr(), b.data_ptr(), 1, 192, bases.data_ptr(), 1, 2, a.data_ptr(), d.data_ptr(), st))
    with pytest.raises(ValueError):
        _lib.check(L.basic_group_lanes_pack_dev(a.data_ptr(), b.data_ptr(), 1, 192, None, 1, 2, c.data_ptr(), d.data_ptr(), st))
    with pytest.raises(ValueError):
        kernels.group_lanes_pack(a, b, bases, 5)
    _lib.check(L.basic_group_lanes_pack_dev(a.data_ptr(), b.data_ptr(), 1, 192, bases.data_ptr(), 1, 2, c.data_ptr(), d.data_ptr(), st))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. the GaussianConditional coder alone
@pytest.fixture(scope="module")
def gc():
    """One coder per lane count, each constructed with stream_lanes=K as a user would, and the oracle encoder on their (common) host
    tables."""
    from cbench_basic_amd.modules.prior_model.prior_coder.compressai_coder import CompressAIGaussianConditionalCoder
    from oracle.rans_oracle import Rans64Encoder
    coders = {}
    for K in (1, 2, 3, 16, 64):
        c = CompressAIGaussianConditionalCoder(stream_lanes=K).eval().cuda()
        c.update_state()
        coders[K] = c
    enc = Rans64Encoder(16, True, 4)
    enc.init_cdf_params(*coders[1]._cdf_host)
    for c in coders.values():
        assert all(np.array_equal(a, b) for a, b in zip(c._cdf_host, coders[1]._cdf_host))
    return coders, enc


def _gc_input(shape, seed, heavy=False):
    g = torch.Generator().manual_seed(seed)
    if heavy:   # scales at the table's floor and latents far outside every table row: bypass symbols everywhere
        y = torch.randn(shape, generator=g) * 3000
        scales = torch.full(shape, 0.05)
    else:
        scales = torch.rand(shape, generator=g) * 4 + 0.05
        y = torch.randn(shape, generator=g) * scales
    return y.cuda(), scales.cuda()


GC_CASES = [((2, 192, 1, 1), 64, False), ((3, 192, 4, 4), 2, False), ((3, 192, 4, 4), 3, False), ((3, 192, 4, 4), 16, False),
            ((3, 192, 4, 4), 64, False), ((3, 192, 4, 4), 16, True), ((2, 192, 1, 1), 64, True)]


@pytest.mark.parametrize("shape,K,heavy", GC_CASES)
def test_gaussian_conditional_lanes(gc, shape, K, heavy):
    from cbench_basic_amd.nn import kernels
    coders, enc = gc
    c1, ck = coders[1], coders[K]
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    per = n // K
    y, scales = _gc_input(shape, 11 * K + n + int(heavy), heavy)
    # the K = 1 symbols and indexes, and the K = 1 body: today's bytes (one oracle stream per image)
    c1._ready()
    sym, idx, _ = kernels.gc_quantize_index(y, scales, c1._scale_table_dev, c1.scale_bound)
    sym, idx = sym.reshape(B, n).cpu().numpy(), idx.reshape(B, n).cpu().numpy()
    body1 = c1.encode(y, prior=scales)
    assert body1 == _cai_body(shape[2], shape[3], [enc.encode_with_indexes(sym[b], idx[b]) for b in range(B)])
    yhat1 = c1.decode(body1, prior=scales)
    assert torch.equal(yhat1, torch.round(y))
    # K lanes: stream b * K + k = the oracle's bytes for symbols [k n / K, (k + 1) n / K) of image b
    body = ck.encode(y, prior=scales)
    h, w, streams = _cai_streams(body)
    assert (h, w) == tuple(shape[2:]) and len(streams) == B * K
    rows = lane_index_lists((0, n), K)
    for b in range(B):
        for k in range(K):
            assert rows[k].tolist() == list(range(k * per, (k + 1) * per))
            want = enc.encode_with_indexes(np.ascontiguousarray(sym[b][rows[k]]), np.ascontiguousarray(idx[b][rows[k]]))
            assert streams[b * K + k] == want, (b, k)
    if heavy and per >= 64:   # more words than the reference-sized slot of a lane holds: the guaranteed slot per lane was taken
        assert max(len(s) for s in streams) > 4 * (per + 2)      # (a lane of 3 symbols fits the per + 2 words of its slot whatever they are)
    assert torch.equal(ck.decode(body, prior=scales), yhat1)
    assert ck.encode(y, prior=scales, lazy=True).result() == body
    # an item's lanes do not depend on its batch; the item framing moves them without touching a byte
    items = [ck.encode(y[b:b + 1], prior=scales[b:b + 1]) for b in range(B)]
    for b in range(B):
        assert items[b] == _cai_body(h, w, streams[b * K:(b + 1) * K]), b
        assert torch.equal(ck.decode(items[b], prior=scales[b:b + 1]), yhat1[b:b + 1])
    assert ck.split_items(body, B) == items and ck.merge_items(items) == body


def test_gaussian_conditional_lane_errors(gc):
    coders, _ = gc
    y, scales = _gc_input((2, 192, 4, 4), 3)
    with pytest.raises(ValueError, match="does not divide"):
        coders[64].encode(y[:, :191].contiguous(), prior=scales[:, :191].contiguous())     # 191 * 16 symbols
    body16 = coders[16].encode(y, prior=scales)
    for K in (2, 3, 64):      # a body of another stream count than B * K
        with pytest.raises(ValueError, match="streams"):
            coders[K].decode(body16, prior=scales)
    with pytest.raises(ValueError, match="streams"):
        coders[16].decode(body16, prior=scales[:1])


# ---------------------------------------------------------------- 3. the hyperprior codec: fused session and module path
@pytest.fixture(scope="module")
def hp():
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    out = {}
    for K in (1, 4, 16):
        c = seed_synthetic_weights(hyperprior_codec(stream_lanes=K), seed=0).eval().cuda()
        c.update_state()
        out[K] = c
    return out


def _decoded_shape(codec, data):
    from cbench_basic_amd import _lib
    sess = codec.entropy_coder._fused_session({}, None)
    assert sess is not None
    buf = np.frombuffer(data, dtype=np.uint8)
    b, c, h, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().basic_hp_decoded_shape(sess._h, buf.ctypes.data, buf.size, ctypes.byref(b), ctypes.byref(c), ctypes.byref(h), ctypes.byref(w)))
    return b.value, c.value, h.value, w.value


@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("shape", [(1, 3, 64, 64), (3, 3, 64, 64), (1, 3, 77, 131), (3, 3, 77, 131)])
def test_hyperprior_fused_equals_module_path_with_lanes(hp, shape, K):
    from cbench_basic_amd.utils.bytes_ops import split_merged_bytes
    c1, ck = hp[1], hp[K]
    ec = ck.entropy_coder
    B = shape[0]
    torch.manual_seed(sum(shape) + K)
    x = torch.rand(*shape)
    ref1 = c1.compress(x.cuda())
    xhat1 = c1.decompress(ref1)
    ec.use_fused_session = False
    try:
        ref = ck.compress(x.cuda())
        xref = ck.decompress(ref)
    finally:
        ec.use_fused_session = True
    assert ec._fused_session({}, None) is not None
    before = ec.profiler.count["encode_fused"]
    for inp in (x.cuda(), x):
        assert ck.compress(inp) == ref, (shape, K, inp.device)
    assert ec.profiler.count["encode_fused"] == before + 2
    xhat = ck.decompress(ref)
    assert torch.equal(xhat, xref) and torch.equal(xhat, xhat1)       # bit-equal to K = 1
    assert _decoded_shape(ck, ref) == tuple(xhat.shape) and xhat.shape[0] == B      # batch = streams of the y body / K
    # the z body is the K = 1 z body; the y body holds B * K streams whose concatenated payload codes the K = 1 symbols
    z1, y1 = split_merged_bytes(ref1, num_segments=2)
    zk, yk = split_merged_bytes(ref, num_segments=2)
    assert zk == z1
    h, w, streams = _cai_streams(yk)
    assert len(streams) == B * K and (h, w) == _cai_streams(y1)[:2]
    # 12 bytes per extra stream at most: 4 of length prefix, 8 of flushed state (word rounding and the split's own loss aside: <= 16)
    assert len(yk) - len(y1) <= 16 * B * (K - 1)
    # batch-1 items keep their lanes
    if B > 1:
        for b in range(B):
            _, yb = split_merged_bytes(ck.compress(x[b:b + 1].cuda()), num_segments=2)
            assert _cai_streams(yb)[2] == streams[b * K:(b + 1) * K], b
    # a session of another lane count refuses the stream
    with pytest.raises(ValueError):
        c1.decompress(ref)
    with pytest.raises(ValueError):
        _decoded_shape(c1, ref)


@pytest.mark.parametrize("K", [4, 16])
def test_hyperprior_lanes_reach_the_overflow_retry(K):
    """Latents far outside the tables make every symbol a bypass symbol: a lane's reference-sized slot (n / K + 2 words) overflows
    and the session re-encodes with the guaranteed slot per lane; the bytes still equal the module path's."""
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    from cbench_basic_amd.utils.bytes_ops import split_merged_bytes
    c = seed_synthetic_weights(hyperprior_codec(N=32, M=48, stream_lanes=K), seed=1).eval()
    with torch.no_grad():
        c.entropy_coder.latent_inference_modules["x_y"].model[6].weight.mul_(4000.0)
    c = c.cuda()
    c.update_state()
    torch.manual_seed(2)
    x = torch.rand(2, 3, 64, 64).cuda()
    c.entropy_coder.use_fused_session = False
    ref = c.compress(x)
    xref = c.decompress(ref)
    c.entropy_coder.use_fused_session = True
    data = c.compress(x)
    assert data == ref
    _, _, streams = _cai_streams(split_merged_bytes(data, num_segments=2)[1])
    per = 48 * 4 * 4 // K
    assert len(streams) == 2 * K and max(len(s) for s in streams) > 4 * (per + 2)     # no reference-sized slot holds it: the retry ran
    assert torch.equal(c.decompress(data), xref)


def test_session_lane_count_is_checked():
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    c = seed_synthetic_weights(hyperprior_codec(N=32, M=48), seed=1).eval().cuda()
    c.update_state()
    sess = c.entropy_coder._fused_session({}, None)
    for bad in (0, -2, 257):
        with pytest.raises(ValueError):
            sess.set_stream_lanes(bad)
    sess.set_stream_lanes(5)          # 48 * 4 * 4 = 768 symbols do not divide into 5 lanes
    try:
        with pytest.raises(ValueError):
            sess.encode(torch.rand(1, 3, 64, 64).cuda())
    finally:
        sess.set_stream_lanes(1)
    data = c.compress(torch.rand(1, 3, 64, 64).cuda())
    assert c.decompress(data).shape == (1, 3, 64, 64)


# ---------------------------------------------------------------- 4. the topo-group coders
TOPO = [("checkerboard", 1), ("raster2x2", 1), ("channelwise", 4), ("elic", 1)]


@pytest.fixture(scope="module")
def topo_coders():
    """(method, K) -> coder, all of one method with the same seeded weights; built with stream_lanes=K as a user would."""
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder
    out = {}
    for method, G in TOPO:
        sd = None
        for K in (1, 2, 4, 128):
            c = Coder(in_channels=192, channel_groups=G, default_topo_group_method=method, stream_lanes=K).eval()
            if sd is None:
                g = torch.Generator().manual_seed(5)
                with torch.no_grad():
                    for p in c.parameters():
                        p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.02))
                sd = {k: v.clone() for k, v in c.state_dict().items()}
            else:
                c.load_state_dict(sd)
            c = c.cuda()
            c.update_state()
            out[(method, K)] = c
    return out


def _topo_input(B, H, W, seed):
    C = 192
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, C, H, W, generator=g) * 2
    prior = torch.stack([torch.randn(B, C, H, W, generator=g), torch.rand(B, C, H, W, generator=g) * 3 + 0.1], 2).reshape(B, 2 * C, H, W)
    return y.cuda(), prior.cuda()


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("H,W", [(4, 4), (4, 6)])
@pytest.mark.parametrize("method,G", TOPO)
def test_topo_group_lanes(topo_coders, method, G, H, W, K):
    from oracle.rans_oracle import Rans64Encoder
    c1, ck = topo_coders[(method, 1)], topo_coders[(method, K)]
    B = 2
    y, prior = _topo_input(B, H, W, 100 * H + W)
    enc = Rans64Encoder(16, True, 4)
    enc.init_params(*c1._ans_params)
    # the K = 1 arrays in coding order, the K = 1 body (today's bytes) and latent
    sym, idx, ybuf, plan = c1._run_encode(y, prior)
    n = plan.per_image
    sym, idx = sym.reshape(B, n).cpu().numpy(), idx.reshape(B, n).cpu().numpy()
    bases = plan_bases(method, c1.channel_groups, 192, H, W)
    assert bases.tolist() == [g["base"] for g in plan.groups] + [n]
    body1 = c1.encode(y, prior=prior)
    assert _pgm_streams(body1, B) == [enc.encode_with_indexes(sym[b], idx[b]) for b in range(B)]
    yhat1 = c1.decode(body1, prior=prior)
    assert torch.equal(yhat1, ybuf)
    rows = lane_index_lists(bases, K)
    want = [enc.encode_with_indexes(np.ascontiguousarray(sym[b][rows[k]]), np.ascontiguousarray(idx[b][rows[k]])) for b in range(B) for k in range(K)]
    saved = (ck.GRAPH_MIN_GROUPS, getattr(ck, "use_hip_graphs", True))
    try:
        for path in ("eager", "graph"):
            ck.use_hip_graphs = path == "graph"
            ck.GRAPH_MIN_GROUPS = 1 if path == "graph" else saved[0]
            body = ck.encode(y, prior=prior)
            assert _pgm_streams(body, B * K) == want, path
            for _ in range(2 if path == "graph" else 1):      # capture, then replay
                assert torch.equal(ck.decode(body, prior=prior), yhat1), path
            if path == "graph":
                assert any(k[0] == "dec" and k[1] == B and k[6] == K for k in ck._graphs) and any(k[0] == "enc" for k in ck._graphs)
            else:
                assert not ck._graphs or all(k[1:4] != (B, H, W) for k in ck._graphs if k[0] == "dec")
    finally:
        ck.GRAPH_MIN_GROUPS, ck.use_hip_graphs = saved
    # an item's lanes do not depend on its batch (tabled item form, K streams)
    items = [ck.encode(y[b:b + 1], prior=prior[b:b + 1]) for b in range(B)]
    for b in range(B):
        assert _pgm_streams(items[b], K) == want[b * K:(b + 1) * K]
    assert ck.split_items(body, B, has_prior=True) == items and ck.merge_items(items, has_prior=True) == body
    # a body of another stream count
    with pytest.raises(ValueError, match="streams"):
        ck.decode(body1, prior=prior)


@pytest.mark.parametrize("method,G", TOPO)
def test_topo_group_non_dividing_lanes_raise(topo_coders, method, G):
    """128 lanes at 3 x 3: every method has a step there that is no multiple of 128 (checkerboard 5 * 192, raster2x2 1 * 192, channel-wise
    g4 9 * 48, elic 5 * 16)."""
    c128 = topo_coders[(method, 128)]
    y, prior = _topo_input(1, 3, 3, 1)
    with pytest.raises(ValueError, match="does not divide"):
        c128.encode(y, prior=prior)
    with pytest.raises(ValueError, match="does not divide"):
        c128.decode(struct.pack("<I", 128) + struct.pack("<128I", *[8] * 128) + b"\0" * 1024, prior=prior)
    with pytest.raises(ValueError, match="pgm"):
        topo_coders[(method, 2)].encode(y, prior=prior, pgm=torch.zeros(1, c128.channel_groups, 3, 3, dtype=torch.long))


# ---------------------------------------------------------------- 5. the harness
def _run_tool(monkeypatch, capsys, argv):
    import importlib.util
    import sys
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "run_benchmark.py")
    spec = importlib.util.spec_from_file_location("run_benchmark_tool_lanes_gpu", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["run_benchmark.py"] + argv)
    capsys.readouterr()
    tool.main()
    out = capsys.readouterr().out
    return json.loads(out[out.rindex("\n{") + 1 if "\n{" in out else out.index("{"):])      # the metrics are the last thing printed


@pytest.mark.parametrize("kind", ["hyperprior", "checkerboard"])
def test_harness_coalesce_with_lanes(kind, tmp_path, monkeypatch, capsys):
    """--coalesce 3 --stream-lanes 4 over 6 small items: the tool's pass measures what the one-call-per-item pass measures, and the
    per-item strings of the coalesced calls are those of 6 separate calls."""
    from cbench_basic_amd import presets
    from cbench_basic_amd.data import RandomImageDataset, batched
    codec_args = ["--codec", "hyperprior"] if kind == "hyperprior" else ["--codec", "topogroup", "--method", "checkerboard"]
    common = codec_args + ["--synthetic", "6", "--size", "64", "--stream-lanes", "4"]
    seq = _run_tool(monkeypatch, capsys, common + ["--out", str(tmp_path / "seq")])
    co = _run_tool(monkeypatch, capsys, common + ["--coalesce", "3", "--out", str(tmp_path / "co")])
    ends = ("compressed_length", "compression_ratio", "original_length", "psnr")
    keys = [k for k in seq if k.endswith(ends)]
    assert len(keys) == 4 and list(seq) == list(co)
    for k in keys:
        assert abs(seq[k] - co[k]) <= 1e-9 * max(1.0, abs(seq[k])), (k, seq[k], co[k])
    # the strings themselves
    build = (lambda **kw: presets.hyperprior_codec(**kw)) if kind == "hyperprior" else (lambda **kw: presets.topogroup_ar_codec(method="checkerboard", **kw))
    codec = presets.seed_synthetic_weights(build(stream_lanes=4), seed=0).eval().cuda()
    codec.update_state()
    items = list(batched(RandomImageDataset(num=6, size=(3, 64, 64)), 1))
    want = [codec.compress(x.cuda()) for x in items]
    got = codec.compress_items(items, max_batch=3)
    assert codec.last_items_calls == 2 and got == want
    xhat = codec.decompress_items(want, max_batch=3)
    assert codec.last_items_calls == 2
    for a, s in zip(xhat, want):
        assert torch.equal(a, codec.decompress(s))
    # and they are not the K = 1 strings: 4 streams in every item's y body, same reconstruction
    plain = build().eval()
    plain.load_state_dict(codec.state_dict())      # the SAME weights (seed_synthetic_weights leaves the y coder's biases to the global generator)
    plain = plain.cuda()
    plain.update_state()
    one = plain.compress(items[0].cuda())
    assert one != want[0] and 0 < len(want[0]) - len(one) <= 16 * 3 + 8
    assert torch.equal(plain.decompress(one), xhat[0])
