"""The quantiser step of the hyperprior y coder from the coder up (INTEGRATION.md "Quantiser step"): the GaussianConditional coder's
bytes are those of the CPU rANS oracle fed the NumPy restatement's symbols and indexes (tests/qstep_exact.py) on the coder's own host
tables, with and without lane streams; a coarser step writes fewer bytes; and through the codec the fused session and the
module-by-module path write the same bytes and decode the same picture, for float32 and uint8 input, per-image steps, and a session
that has had steps and lost them."""
import struct

import numpy as np
import pytest
import torch

import qstep_exact as QX

pytestmark = pytest.mark.gpu


def _cai_body(h, w, streams):
    return struct.pack(">3I", h, w, len(streams)) + b"".join(struct.pack(">I", len(s)) + s for s in streams)


# ---------------------------------------------------------------- the coder alone
@pytest.fixture(scope="module")
def gc():
    from cbench_basic_amd.modules.prior_model.prior_coder.compressai_coder import CompressAIGaussianConditionalCoder
    from oracle.rans_oracle import Rans64Encoder
    coders = {}
    for K in (1, 4):
        c = CompressAIGaussianConditionalCoder(stream_lanes=K).eval().cuda()
        c.update_state()
        c._ready()
        coders[K] = c
    enc = Rans64Encoder(16, True, 4)
    enc.init_cdf_params(*coders[1]._cdf_host)
    return coders, enc


@pytest.mark.parametrize("shape,K,steps", [((3, 8, 5, 7), 1, (0.5, 1.0, 3.0)), ((3, 8, 4, 4), 4, (0.5, 1.0, 3.0)), ((3, 8, 5, 7), 1, (0.7,)),
                                           ((2, 8, 4, 4), 4, 2.0)])
def test_coder_bytes_are_the_oracles_on_the_restated_symbols(gc, shape, K, steps):
    coders, enc = gc
    c = coders[K]
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    g = torch.Generator().manual_seed(n + K)
    scales = torch.exp(torch.rand(shape, generator=g) * 6 - 2.5)            # 0.08 .. 33: below the bound too
    y = torch.randn(shape, generator=g) * scales
    y[:, 0, 0, :2] = torch.tensor([0.75, 1.25])
    y[:, 1, 0, :2] = torch.tensor([4.5, -4.5])
    table = c.scale_table.cpu().numpy()
    sym, idx, yhat = QX.quantize_index_q(y.numpy(), scales.numpy(), steps, n, table, c.scale_bound)
    sym, idx = sym.reshape(B * K, n // K), idx.reshape(B * K, n // K)       # lane k of image b: a contiguous run
    want = _cai_body(shape[2], shape[3], [enc.encode_with_indexes(np.ascontiguousarray(sym[i]), np.ascontiguousarray(idx[i])) for i in range(B * K)])
    body = c.encode(y.cuda(), prior=scales.cuda(), qstep=steps)
    assert body == want
    assert c.encode(y.cuda(), prior=scales.cuda(), qstep=steps, lazy=True).result() == want
    dec = c.decode(body, prior=scales.cuda(), qstep=steps)
    assert QX.same_reconstruction(dec.cpu().numpy(), yhat, sym)             # the encoder's yhat (signed zero: see qstep_exact)
    fwd = c(y.cuda(), prior=scales.cuda(), qstep=steps)
    assert np.array_equal(fwd.cpu().numpy().reshape(-1).view(np.int32), yhat.view(np.int32))
    assert torch.equal(dec, fwd)
    # the rate estimate follows the step: the fp64 value of the restated symbols under scale / step, in nats per image
    t64 = QX.nll_terms_q(sym.reshape(shape).astype(np.float32), scales.numpy(), steps, c.scale_bound, 1e-9, torch.float64)
    est = float(c.get_raw_cache("metric_dict")["prior_entropy"])
    assert abs(est - float(t64.reshape(B, -1).sum(1).mean())) <= 1e-4 * est      # (the bound test_gpu_entropy_kernels keeps its budgets under)
    # None is today's call, untouched; step 1 writes its bytes
    assert c.encode(y.cuda(), prior=scales.cuda(), qstep=1.0) == c.encode(y.cuda(), prior=scales.cuda()) == c.encode(y.cuda(), prior=scales.cuda(), qstep=None)


def test_coder_refuses_bad_steps_and_two_knobs(gc):
    c = gc[0][1]
    y = torch.randn(2, 8, 4, 4).cuda()
    s = torch.ones_like(y)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -5, 100.0, [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            c.encode(y, prior=s, qstep=bad)
        with pytest.raises(ValueError):
            c(y, prior=s, qstep=bad)
    body = c.encode(y, prior=s, qstep=[1.0, 2.0])
    with pytest.raises(ValueError):
        c.decode(body, prior=s, qstep=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="two rate knobs"):
        c.encode(y, prior=s, qstep=2.0, channel_gains=torch.ones(8).cuda())


def test_a_coarser_step_writes_fewer_bytes(gc):
    """y iid N(0, 8), sigma = 8 everywhere, 192 * 16 * 16 = 49,152 symbols: sigma / step stays between 2 and 16, well inside the table,
    where doubling the step takes about one bit off every symbol (about 6 kB here).  Derived, not measured; only the order is asserted."""
    c = gc[0][1]
    g = torch.Generator().manual_seed(8)
    y = (torch.randn(1, 192, 16, 16, generator=g) * 8).cuda()
    s = torch.full_like(y, 8.0)
    lens = {d: len(c.encode(y, prior=s, qstep=d)) for d in (4.0, 2.0, 1.0, 0.5)}
    print("bytes per step:", lens)
    assert lens[4.0] < lens[2.0] < lens[1.0] < lens[0.5]


# ---------------------------------------------------------------- the codec
@pytest.fixture(scope="module")
def codec():
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    c = seed_synthetic_weights(hyperprior_codec(), seed=0).eval().cuda()
    c.update_state()
    return c


def _x(shape, dtype, order):
    torch.manual_seed(sum(shape))
    if dtype == torch.float32:
        return torch.rand(*shape)
    x = torch.randint(0, 256, shape, dtype=torch.uint8)
    return x if order == "chw" else x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # the same picture, [B][H][W][C] memory


def _header(n):
    return 8 + 4 * n


@pytest.mark.parametrize("dtype,order", [(torch.float32, "chw"), (torch.uint8, "chw"), (torch.uint8, "hwc")], ids=["f32", "u8-chw", "u8-hwc"])
@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 72, 88)])
def test_fused_and_module_paths_agree_under_a_step(codec, shape, dtype, order):
    ec = codec.entropy_coder
    B = shape[0]
    x = _x(shape, dtype, order)
    plain = codec.compress(x)
    for qstep in (1.0, 2.0, [0.5, 3.0][:B]):
        n = 1 if isinstance(qstep, float) else len(qstep)
        try:
            ec.use_fused_session = False
            ref = codec.compress_q(x.cuda(), qstep)
            xref = codec.decompress_q(ref)
            uref = codec.decompress_q(ref, output_dtype=torch.uint8)
        finally:
            ec.use_fused_session = True
        assert ec._fused_session({}, None) is not None
        before = ec.profiler.count["encode_fused"], ec.profiler.count["decode_fused"]
        for inp in (x.cuda(), x):                                         # device and host input
            assert codec.compress_q(inp, qstep) == ref, (qstep, inp.device)
        xhat = codec.decompress_q(ref)
        uhat = codec.decompress_q(ref, output_dtype=torch.uint8)
        assert (ec.profiler.count["encode_fused"], ec.profiler.count["decode_fused"]) == (before[0] + 2, before[1] + 2)   # the step keeps the call on its path
        # (the graph returns g_s's own size, a multiple of 16: 80 x 96 for a 72 x 88 picture, as decompress() does)
        assert xhat.shape == xref.shape == codec.decompress(plain).shape and float((xhat - xref).abs().max()) <= 1e-4
        assert uhat.dtype == torch.uint8 and torch.equal(uhat, uref)
        # the container: magic, count, steps, then exactly what encode(x, qstep=) returned
        assert ref[:4] == b"BQS1" and struct.unpack("<I", ref[4:8])[0] == n
        assert ref[8:_header(n)] == np.asarray(qstep, "<f4").reshape(-1).tobytes()
        assert ref[_header(n):] == ec.encode(x.cuda(), qstep=qstep)
        if qstep == 1.0:
            assert ref[_header(1):] == plain                                # step 1 is today's codec, byte for byte
        else:
            assert ref[_header(n):] != plain
        assert codec.compress(x) == plain                                    # steps set and cleared: compress() writes its bytes again


def test_per_image_steps_are_the_per_image_calls(codec):
    """A step vector codes image b as the batch-1 call with step b does: the bodies agree image by image, on both paths."""
    from cbench_basic_amd.utils.item_framing import _parse_compressai
    from cbench_basic_amd.utils.bytes_ops import split_merged_bytes
    ec = codec.entropy_coder
    torch.manual_seed(3)
    x = torch.rand(3, 3, 64, 64).cuda()
    steps = [0.5, 1.0, 3.0]
    for fused in (True, False):
        try:
            ec.use_fused_session = fused
            both = codec.compress_q(x, steps)[_header(3):]
            singles = [codec.compress_q(x[b:b + 1], steps[b])[_header(1):] for b in range(3)]
            xhat = codec.decompress_q(codec.compress_q(x, steps))
            alone = [codec.decompress_q(codec.compress_q(x[b:b + 1], steps[b])) for b in range(3)]
        finally:
            ec.use_fused_session = True
        zb, yb = split_merged_bytes(both, num_segments=2)
        (zh, zw, zs), (yh, yw, ys) = _parse_compressai(zb), _parse_compressai(yb)
        assert len(zs) == len(ys) == 3
        for b in range(3):
            z1, y1 = split_merged_bytes(singles[b], num_segments=2)
            assert _parse_compressai(z1) == (zh, zw, [zs[b]]) and _parse_compressai(y1) == (yh, yw, [ys[b]]), (fused, b)
            assert float((xhat[b:b + 1] - alone[b]).abs().max()) <= 1e-4


def test_lane_streams_keep_working_under_a_step():
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    c = seed_synthetic_weights(hyperprior_codec(stream_lanes=4), seed=0).eval().cuda()
    c.update_state()
    ec = c.entropy_coder
    torch.manual_seed(4)
    x = torch.rand(2, 3, 64, 64).cuda()
    try:
        ec.use_fused_session = False
        ref = c.compress_q(x, [0.7, 2.0])
        xref = c.decompress_q(ref)
    finally:
        ec.use_fused_session = True
    assert c.compress_q(x, [0.7, 2.0]) == ref
    assert float((c.decompress_q(ref) - xref).abs().max()) <= 1e-4
    assert c.compress_q(x, 1.0)[_header(1):] == c.compress(x)


def test_refusals_before_any_launch(codec):
    ec = codec.entropy_coder
    x = torch.rand(2, 3, 64, 64).cuda()
    good = codec.compress_q(x, [1.0, 2.0])
    plain = codec.compress(x)
    for bad in (0.0, -2.0, float("nan"), float("inf"), 2.0 ** -5, 65.0, [1.0, 2.0, 3.0], []):
        with pytest.raises(ValueError):
            codec.compress_q(x, bad)
        with pytest.raises(ValueError):
            ec.encode(x, qstep=bad)
    inner = good[_header(2):]
    for data in (b"", b"BQS1", b"BQS2" + good[4:], good[:11], inner,
                 b"BQS1" + struct.pack("<I3f", 3, 1.0, 2.0, 3.0) + inner,             # three steps for a batch of two
                 b"BQS1" + struct.pack("<If", 1, 0.0) + inner, b"BQS1" + struct.pack("<If", 1, float("nan")) + inner):
        for fused in (True, False):
            try:
                ec.use_fused_session = fused
                with pytest.raises(ValueError):
                    codec.decompress_q(data)
            finally:
                ec.use_fused_session = True
    with pytest.raises(ValueError):
        ec.decode(inner, qstep=[1.0, 2.0, 3.0])
    # the session itself: values on the host, the count against the call's batch
    sess = ec._fused_session({}, None)
    for bad in (0.0, float("nan"), float("inf"), 128.0):
        with pytest.raises(ValueError):
            sess.set_qsteps(bad)
    sess.set_qsteps([1.0, 2.0, 3.0])
    try:
        with pytest.raises(ValueError):
            sess.encode(x)
        with pytest.raises(ValueError):
            sess.decode(inner)
    finally:
        sess.set_qsteps(None)
    assert codec.compress_q(x, [1.0, 2.0]) == good and codec.compress(x) == plain      # none of the refusals left a step behind


def test_a_pgm_y_coder_refuses_the_step():
    from cbench_basic_amd.presets import topogroup_ar_codec
    c = topogroup_ar_codec("checkerboard", N=32, M=48).eval().cuda()
    c.update_state()
    x = torch.rand(1, 3, 64, 64).cuda()
    with pytest.raises(TypeError, match="quantizer_params"):
        c.compress_q(x, 2.0)
    with pytest.raises(TypeError, match="quantizer_params"):
        c.entropy_coder.encode(x, qstep=2.0)
    data = c.compress(x)
    with pytest.raises(TypeError, match="quantizer_params"):
        c.entropy_coder.decode(data, qstep=2.0)
    assert c.compress(x) == data
