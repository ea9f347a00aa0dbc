"""Lane streams of the scan-line y-coder (stream_lanes = K > 1, INTEGRATION.md "Lane streams"): an image's channels are cut into K
lanes of C / K, each its own rANS64 stream; the persistent decode launch runs K decoder wavefronts per image, the per-step path
steps K streams per image, the encoder codes B * K contiguous streams.  Only the framing changes, so everything here is exact:

  * every lane stream equals, byte for byte, what the CPU rANS oracle writes for that lane of scanline_exact.py's reference
    symbols and table rows (never another path of the library), and decodes to the reference's float bits;
  * which path wrote the bytes and which one reads them is free, and an image's streams do not depend on the batch around it;
  * the new C entries write all of their outputs and nothing else (guard bands);
  * what the format does not offer is refused on the host, before any launch;
  * a decode call whose decoder wavefronts do not fit beside the compute workgroups goes to the per-step path, and decodes.

The coders are scanline_cases._coder("ctxmodel", 192)'s configuration, one per lane count and built with stream_lanes=K as a user
builds them, with scanline_exact's layers installed."""
import math
import struct

import numpy as np
import pytest
import torch

from scanline_cases import BAND, GUARD, _coder, _plan_of
from scanline_exact import C, exact_case, exact_params, install
from test_cpu_stream_lanes import (LANE_COUNTS, SIZE_CAP_PER_STREAM, lane_permutation_numpy, oracle_encoder, oracle_lane_streams)
from test_gpu_scanline_exact import _Forced, _bits

pytestmark = pytest.mark.gpu

_STATE = {}


def _exact_coder(lanes):
    """One coder per lane count for the whole run, constructed with stream_lanes=lanes (K = 1: scanline_cases._coder itself, built
    without the argument), every parameter overwritten with the exact layers of the 5 x 5 window."""
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import (GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder,
                                                                            TopoGroupDynamicMaskConv2dContextModel as Ctx)
    if ("coder", lanes) not in _STATE:
        if lanes == 1:
            c = _coder("ctxmodel", C)
        else:
            c = Coder(in_channels=C, default_topo_group_method="scanline", topo_group_context_model=Ctx(in_channels=C, out_channels=2 * C, kernel_size=5),
                      stream_lanes=lanes).eval().cuda()
        install(c, exact_params(5))
        c.update_state()
        assert c.stream_lanes == lanes
        _STATE["coder", lanes] = c
    c = _STATE["coder", lanes]
    c.use_persistent_scanline = True
    c.scanline_encode_schedule = "auto"
    c.persistent_scanline_max_batch = type(c).persistent_scanline_max_batch
    return c


def _oracle(coder):
    if "oracle" not in _STATE:
        _STATE["oracle"] = oracle_encoder(coder._ans_params, coder.freq_precision, coder.use_bypass_coding, coder.bypass_precision)
    return _STATE["oracle"]


def _case(B, H, W):
    yn, pn, ref = exact_case(5, B, H, W, 1000 * B + 10 * H + W)
    return torch.from_numpy(yn.copy()).cuda(), torch.from_numpy(pn.copy()).cuda(), ref


def _split(body, nstreams):
    """<I n> <n x I length> streams -> the n streams; asserts the count and that the body holds nothing else."""
    (n,) = struct.unpack("<I", body[:4])
    assert n == nstreams, f"the body holds {n} streams, not {nstreams}"
    lens = struct.unpack("<%dI" % n, body[4: 4 + 4 * n])
    at, out = 4 + 4 * n, []
    for ln in lens:
        out.append(bytes(body[at: at + ln]))
        at += ln
    assert at == len(body)
    return out


def _check_kernel(coder, path):
    if path != "per-step":
        sl = coder._layers["scanline"][0]
        sl.check()
        assert sl.last_kernel() == path, sl.last_kernel()


_RASTER = [(1, 5, 6), (2, 7, 9)]
PATH_CASES = {"per-step": _RASTER, "generic": _RASTER, "pipelined": _RASTER, "batched": [(3, 5, 7), (33, 2, 6)]}


# K = 2: a 64-chunk and a 32-tail per lane; K = 3: whole 64-chunks (the spelled-out path); K = 12: 16-symbol chunks (the generic path)
@pytest.mark.parametrize("lanes", LANE_COUNTS)
@pytest.mark.parametrize("path", list(PATH_CASES))
def test_lane_streams_are_the_oracles(path, lanes):
    """1. (and 9.)  Every lane stream is the CPU rANS oracle's for that lane of the NumPy reference; the decoder returns the
    reference's bits; both directions ran the forced kernel; the body is at most 16 bytes per lane stream longer than the K = 1
    body of the same call (4 of length field, at most 8 of flushed state, 4 of word rounding: test_cpu_stream_lanes.py confirms the
    cap with the oracle alone)."""
    for B, H, W in PATH_CASES[path]:
        y, prior, ref = _case(B, H, W)
        coder = _exact_coder(lanes)
        want = oracle_lane_streams(_oracle(coder), ref["sym"], ref["idx"], H * W, C, lanes)
        with _Forced(coder, path):
            data = coder.encode(y, prior=prior)
            _check_kernel(coder, path)
            got = _split(data, B * lanes)
            bad = [s for s in range(B * lanes) if got[s] != want[s // lanes][s % lanes]]
            print(f"B={B} {H}x{W} K={lanes} [{path}]: {len(data)} bytes, {len(bad)} of {B * lanes} lane streams differ from the oracle's")
            assert not bad, bad[:8]
            yhat = coder.decode(data, prior=prior)
            _check_kernel(coder, path)
            md = int((_bits(yhat) != ref["ybuf"].view(np.int32)).sum())
            print(f"B={B} {H}x{W} K={lanes} [{path}]: decoded ybuf bit diffs {md}")
            assert md == 0
        one = _exact_coder(1).encode(y, prior=prior)
        print(f"B={B} {H}x{W} K={lanes} [{path}]: K = 1 body {len(one)} bytes, {(len(data) - len(one)) / (B * lanes):.2f} extra bytes per lane stream")
        assert len(data) - len(one) <= SIZE_CAP_PER_STREAM * B * lanes


def test_encoder_and_decoder_need_not_agree_on_a_path():
    """2. Bytes of the per-step path at K = 3 decode through the batched and the pipelined kernel to the reference's bits, and theirs
    through the per-step path; all three write the same bytes."""
    for B, H, W, kernel in [(3, 5, 7, "batched"), (2, 7, 9, "pipelined")]:
        y, prior, ref = _case(B, H, W)
        coder = _exact_coder(3)
        with _Forced(coder, "per-step"):
            slow = coder.encode(y, prior=prior)
        with _Forced(coder, kernel):
            fast = coder.encode(y, prior=prior)
            _check_kernel(coder, kernel)
            back = coder.decode(slow, prior=prior)
            _check_kernel(coder, kernel)
        assert fast == slow
        assert np.array_equal(_bits(back), ref["ybuf"].view(np.int32))
        with _Forced(coder, "per-step"):
            back = coder.decode(fast, prior=prior)
        assert np.array_equal(_bits(back), ref["ybuf"].view(np.int32))


@pytest.mark.parametrize("lanes", [3, 12])
def test_batch_invariance(lanes):
    """3. Image b's K streams in a call of five images are the streams of that image coded alone."""
    B, H, W = 5, 3, 4
    y, prior, _ = _case(B, H, W)
    coder = _exact_coder(lanes)
    together = _split(coder.encode(y, prior=prior), B * lanes)
    for b in range(B):
        alone = _split(coder.encode(y[b: b + 1].contiguous(), prior=prior[b: b + 1].contiguous()), lanes)
        assert alone == together[b * lanes: (b + 1) * lanes], f"image {b}"


def _lane_words(coder, sym, idx, B, P, lanes):
    """Device words and offsets of the B * lanes lane streams of sym / idx [B, P * C] (pack, then the batched encoder)."""
    from cbench_basic_amd.nn import kernels as K
    ps, pi = K.lanes_pack(sym, idx, B, P, C, lanes)
    words, woff = coder._tables.encode_batch_end(coder._tables.encode_batch_begin(ps.reshape(-1), pi.reshape(-1), P * C // lanes))
    assert len(woff) == B * lanes + 1
    return torch.from_numpy(words[: int(woff[-1])].view(np.int32).copy()).cuda(), torch.from_numpy(woff.astype(np.int64)).cuda()


@pytest.mark.parametrize("kernel", ["generic", "pipelined", "batched"])
@pytest.mark.parametrize("B,H,W", [(2, 3, 4), (5, 3, 4)])
def test_decode_lanes_guard_bands(kernel, B, H, W):
    """4. basic_scanline_decode_lanes_dev at K = 3 with its outputs as views into sentinel-filled buffers: all of sym, idx and ybuf
    is written with the reference's values and nothing outside; a refusal ("does not fit") writes nothing."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    lanes = 3
    coder = _exact_coder(lanes)
    sl = _plan_of(coder, C)
    y, prior, ref = _case(B, H, W)
    n = H * W * C
    d_words, d_woff = _lane_words(coder, torch.from_numpy(ref["sym"].copy()).cuda(), torch.from_numpy(ref["idx"].copy()).cuda(), B, H * W, lanes)
    table = coder._scale_table_dev.to(device="cuda", dtype=torch.float32).contiguous()
    off, fresh = 64, 0x7FC00001
    bufs = [torch.full((off + B * n + BAND,), GUARD, dtype=torch.int32, device="cuda") for _ in range(3)]
    for b in bufs:
        b[off: off + B * n] = fresh
    sym, idx, ybuf = (b[off: off + B * n] for b in bufs)
    refused = False
    with _Forced(coder, kernel):
        try:
            _lib.check(_lib.lib().basic_scanline_decode_lanes_dev(sl._h, coder._tables._h, d_words.data_ptr(), d_woff.data_ptr(), prior.data_ptr(), B,
                                                                  lanes, H, W, table.data_ptr(), table.numel(), sym.data_ptr(), idx.data_ptr(),
                                                                  ybuf.data_ptr(), K._stream()))
        except (RuntimeError, ValueError) as e:
            if "does not fit" not in str(e):
                raise
            refused = True
        sl.check()
    assert refused == (kernel == "pipelined" and B > 2), "the pipelined kernel serves one or two images at this width, the others any"
    for name, b in zip(("sym", "idx", "ybuf"), bufs):
        h = b.cpu()
        assert bool((h[:off] == GUARD).all()) and bool((h[off + B * n:] == GUARD).all()), f"the launch wrote outside {name}"
    if refused:
        assert all(bool((b[off: off + B * n] == fresh).all()) for b in bufs)
        return
    assert sl.last_kernel() == kernel
    assert np.array_equal(sym.cpu().numpy().reshape(B, -1), ref["sym"]) and np.array_equal(idx.cpu().numpy().reshape(B, -1), ref["idx"])
    assert np.array_equal(ybuf.cpu().numpy().reshape(ref["ybuf"].shape), ref["ybuf"].view(np.int32))


@pytest.mark.parametrize("lanes", [12, 1])
def test_pack_and_strided_lanes_guard_bands(lanes):
    """5. basic_lanes_pack_dev against the NumPy permutation and basic_rans_decode_batch_lanes_dev (one call per position, as the
    per-step path makes them) against the oracle's decoder, both on sentinel-filled buffers: B = 2, P = 6, C = 192."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    from oracle.rans_oracle import Rans64Decoder
    B, H, W = 2, 2, 3
    P, n = H * W, H * W * C
    coder = _exact_coder(1)
    _, _, ref = _case(B, H, W)
    perm = lane_permutation_numpy(P, C, lanes)
    off, fresh = 64, 0x7FC00001
    src = [torch.from_numpy(ref[k].copy()).cuda() for k in ("sym", "idx")]
    outs = [torch.full((off + B * n + BAND,), GUARD, dtype=torch.int32, device="cuda") for _ in range(2)]
    for o in outs:
        o[off: off + B * n] = fresh
    _lib.check(_lib.lib().basic_lanes_pack_dev(src[0].data_ptr(), src[1].data_ptr(), B, P, C, lanes, outs[0][off:].data_ptr(), outs[1][off:].data_ptr(),
                                               K._stream()))
    for key, o in zip(("sym", "idx"), outs):
        h = o.cpu().numpy()
        assert (h[:off] == GUARD).all() and (h[off + B * n:] == GUARD).all(), f"the pack wrote outside {key}"
        assert np.array_equal(h[off: off + B * n].reshape(B, lanes, -1), ref[key][:, perm]), key
        if lanes == 1:
            assert np.array_equal(h[off: off + B * n].reshape(B, -1), ref[key])   # the identity
    # the lane streams, written by the oracle; decoded position by position on the dense [B][n] arrays
    enc = _oracle(coder)
    streams = [s for img in oracle_lane_streams(enc, ref["sym"], ref["idx"], P, C, lanes) for s in img]
    dec = Rans64Decoder(coder.freq_precision, coder.use_bypass_coding, coder.bypass_precision)
    dec.init_params(*coder._ans_params)
    for s, data in enumerate(streams):
        b, k = divmod(s, lanes)
        back = np.asarray(dec.decode_with_indexes(data, np.ascontiguousarray(ref["idx"][b][perm[k]])), dtype=np.int32)
        assert np.array_equal(back, ref["sym"][b][perm[k]])   # the oracle's decoder reads the oracle's streams
    woff = np.concatenate([[0], np.cumsum([len(s) // 4 for s in streams])]).astype(np.int64)
    d_words = torch.from_numpy(np.frombuffer(b"".join(streams), dtype=np.int32).copy()).cuda()
    d_woff = torch.from_numpy(woff).cuda()
    out = torch.full((off + B * n + BAND,), GUARD, dtype=torch.int32, device="cuda")
    out[off: off + B * n] = fresh
    state = torch.zeros((B * lanes,), device="cuda", dtype=torch.int64)
    pos = torch.full((B * lanes,), -1, device="cuda", dtype=torch.int64)
    for p in range(P):
        coder._tables.decode_batch_lanes(d_words, d_woff, src[1], p * C, n, lanes, C // lanes, B, out[off:], state, pos)
    h = out.cpu().numpy()
    assert (h[:off] == GUARD).all() and (h[off + B * n:] == GUARD).all(), "the decoder wrote outside its symbols"
    assert np.array_equal(h[off: off + B * n].reshape(B, -1), ref["sym"])
    assert np.array_equal(pos.cpu().numpy(), np.diff(woff))   # every stream was read to its end, none beyond


def test_refusals_on_the_host():
    """6. What the format does not offer raises ValueError before any launch."""
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import (GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder,
                                                                            TopoGroupDynamicMaskConv2dContextModel as Ctx)
    mk = lambda **kw: Coder(in_channels=C, topo_group_context_model=Ctx(in_channels=C, out_channels=2 * C), **kw)
    for bad in (5, 24, 0):
        with pytest.raises(ValueError, match="stream_lanes"):
            mk(default_topo_group_method="scanline", stream_lanes=bad)
    with pytest.raises(ValueError, match="stream_lanes"):
        mk(default_topo_group_method="checkerboard", stream_lanes=3)
    with pytest.raises(ValueError, match="stream_lanes"):
        mk(default_topo_group_method="scanline", channel_groups=2, stream_lanes=3)
    with pytest.raises(ValueError, match="stream_lanes"):
        mk(default_topo_group_method="scanline", batch_stream_mode="reference", stream_lanes=3)
    assert mk(default_topo_group_method="scanline", stream_lanes=3).stream_lanes == 3
    coder = _exact_coder(3)
    sl = _plan_of(coder, C)
    before = sl.last_kernel()
    y, prior, _ = _case(2, 3, 4)
    pgm = torch.zeros(2, 1, 3, 4, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="pgm"):
        coder.encode(y, prior=prior, pgm=pgm)
    data = coder.encode(y, prior=prior)
    sl.check()
    before = sl.last_kernel()
    with pytest.raises(ValueError, match="pgm"):
        coder.decode(data, prior=prior, pgm=pgm)
    streams = _split(data, 6)
    for keep in (5, 2):   # a body of another count: another batch's, or another lane count's
        body = struct.pack("<I", keep) + b"".join(struct.pack("<I", len(s)) for s in streams[:keep]) + b"".join(streams[:keep])
        with pytest.raises(ValueError, match="streams"):
            coder.decode(body, prior=prior)
    with pytest.raises(ValueError, match="streams"):
        _exact_coder(12).decode(data, prior=prior)
    with pytest.raises(ValueError, match="lanes"):
        sl.choose(2, 3, 4, coder._scale_table_dev.numel(), "auto", 4, coder._tables, lanes=5)
    assert sl.last_kernel() == before   # no launch was made


@pytest.mark.parametrize("lanes", [1, 2, 3, 4, 6, 12])
def test_planner_counts_the_lane_wavefronts(lanes):
    """7, Python.  A decode call of 64 images (the batched kernel's, were there room) is left to the per-step path exactly when the
    compute workgroups and the ceil(B K / 4) decoder workgroups no longer fit the device's compute units; encode calls do not
    depend on the lanes."""
    B, H, W = 64, 2, 6
    coder = _exact_coder(lanes)
    sl = _plan_of(coder, C)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    over = sl.workgroups + math.ceil(B * lanes / 4) > cus
    kernel, _ = sl.choose(B, H, W, coder._scale_table_dev.numel(), "auto", coder.persistent_scanline_max_batch, coder._tables, lanes=lanes)
    print(f"K={lanes}: {sl.workgroups} compute + {math.ceil(B * lanes / 4)} decoder workgroups on {cus} compute units -> {kernel or 'per-step'}")
    assert (kernel is None) == over
    if not over:
        assert kernel == "batched"
    enc = sl.choose(B, H, W, coder._scale_table_dev.numel(), "raster", coder.persistent_scanline_max_batch, None, lanes=lanes)
    assert enc == sl.choose(B, H, W, coder._scale_table_dev.numel(), "raster", coder.persistent_scanline_max_batch, None)
    if lanes == 1:
        assert sl.choose(B, H, W, coder._scale_table_dev.numel(), "auto", coder.persistent_scanline_max_batch, coder._tables)[0] == kernel


def test_call_at_the_residency_limit_decodes():
    """7, kernel.  64 images at K = 12 -- 192 decoder workgroups, which fill a 256-unit chip to the last compute unit beside 64 compute
    workgroups and do not fit a smaller one -- decode to the reference's bits (first and last image) from streams that are the
    oracle's: through the per-step path exactly where the planner leaves the call to it, through the batched kernel otherwise."""
    B, H, W, lanes = 64, 2, 6, 12
    y, prior, ref = _case(B, H, W)
    coder = _exact_coder(lanes)
    sl = _plan_of(coder, C)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    plan = coder._plans_for(H, W, None, B)
    served = coder._scanline_plan(plan, prior, B, decode=True, width=W, height=H)
    assert (served is None) == (sl.workgroups + math.ceil(B * lanes / 4) > cus)
    data = coder.encode(y, prior=prior)
    got = _split(data, B * lanes)
    enc = _oracle(coder)
    perm = lane_permutation_numpy(H * W, C, lanes)
    for b in (0, B - 1):
        for k in (0, lanes - 1):
            assert got[b * lanes + k] == enc.encode_with_indexes(np.ascontiguousarray(ref["sym"][b][perm[k]]), np.ascontiguousarray(ref["idx"][b][perm[k]]))
    yhat = coder.decode(data, prior=prior)
    if served is not None:
        served.check()
        assert served.last_kernel() == "batched"
    bits = _bits(yhat)
    for b in (0, B - 1):
        assert np.array_equal(bits[b], ref["ybuf"].view(np.int32)[b]), f"image {b}"


def test_call_beyond_the_chip_goes_to_the_per_step_path():
    """7, the refusing side.  65 images at K = 12 are 195 decoder workgroups: with the compute workgroups more than the chip's compute
    units, whatever the coder's batch gate allows.  The planner leaves the decode call to the per-step path -- at K = 1 the same
    call's 17 decoder workgroups fit and it does not --, and the call decodes there to the reference's bits."""
    B, H, W, lanes = 65, 2, 6, 12
    coder = _exact_coder(lanes)
    sl = _plan_of(coder, C)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert sl.workgroups + math.ceil(B * lanes / 4) > cus >= sl.workgroups + math.ceil(B / 4)
    tl = coder._scale_table_dev.numel()
    assert sl.choose(B, H, W, tl, "auto", 128, coder._tables, lanes=lanes)[0] is None
    assert sl.choose(B, H, W, tl, "auto", 128, coder._tables, lanes=1)[0] is not None
    y, prior, ref = _case(B, H, W)
    data = coder.encode(y, prior=prior)
    assert len(_split(data, B * lanes)) == B * lanes
    coder.persistent_scanline_max_batch = 128   # the batch gate open: what keeps the call off the persistent kernels is the lanes' residency
    plan = coder._plans_for(H, W, None, B)
    assert coder._scanline_plan(plan, prior, B, decode=True, width=W, height=H) is None
    before = sl.last_kernel()
    yhat = coder.decode(data, prior=prior)
    assert sl.last_kernel() == before   # no persistent launch was made
    bits = _bits(yhat)
    for b in (0, B - 1):
        assert np.array_equal(bits[b], ref["ybuf"].view(np.int32)[b]), f"image {b}"


def _codecs():
    from cbench_basic_amd.presets import basic_codec, seed_synthetic_weights
    if "codecs" not in _STATE:
        made = []
        for kw in (dict(stream_lanes=3), dict(stream_lanes=1), dict()):
            torch.manual_seed(4321)   # (what seed_synthetic_weights leaves at its default initialisation comes from the global generator)
            c = seed_synthetic_weights(basic_codec(**kw), seed=0).eval().cuda()
            c.update_state()
            made.append(c)
        _STATE["codecs"] = made
    return _STATE["codecs"]


@pytest.mark.parametrize("level", [0, 7])
def test_codec_level(level):
    """8. BaSIC with three lane streams reconstructs exactly what the K = 1 codec reconstructs, from a longer body; the K = 1 codec's
    bytes are those of a codec built without the argument."""
    lanes3, lanes1, plain = _codecs()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(11)).cuda()
    for c in (lanes3, lanes1, plain):
        c.set_complex_level(level)
    assert lanes3.entropy_coder.latent_node_entropy_coders["y"].stream_lanes == 3
    assert plain.entropy_coder.latent_node_entropy_coders["y"].stream_lanes == 1
    d3, d1, d0 = lanes3.compress(x), lanes1.compress(x), plain.compress(x)
    assert d1 == d0
    assert d3 != d1 and len(d3) > len(d1)
    assert torch.equal(lanes3.decompress(d3), lanes1.decompress(d1))
