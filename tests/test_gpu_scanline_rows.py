"""Row streams of the scan-line y-coder (stream_rows = True, INTEGRATION.md "Row streams"): every latent row of every image (and
lane) is its own rANS64 stream, stream (b * H + r) * K + k.  The wavefront decode launch runs one decoder wavefront per stream and
walks an image's rows in parallel; the raster kernels change stream at every row start; the per-step path steps the row's streams.
Only the framing changes, so everything here is exact:

  * every stream equals, byte for byte, what the CPU rANS oracle writes for that (row, lane) slice of scanline_exact.py's reference
    symbols and table rows (never another path of the library), and decodes to the reference's float bits, through every path;
  * which path wrote the bytes and which one reads them is free, and an image's streams do not depend on the batch around it;
  * the new C entries write all of their outputs and nothing else (guard bands), a refusal writes nothing;
  * what the format does not offer is refused on the host, before any launch;
  * a decode call whose decoder wavefronts do not fit beside the wavefront's compute workgroups leaves the wavefront, and decodes.

The coders are scanline_cases._coder("ctxmodel...", 192)'s configuration built with stream_rows=True (and stream_lanes=K) as a user
builds them, with scanline_exact's layers installed."""
import math
import os
import struct

import numpy as np
import pytest
import torch

from scanline_cases import BAND, GUARD, _plan_of
from scanline_exact import C, exact_params, install
from test_cpu_stream_lanes import SIZE_CAP_PER_STREAM, oracle_encoder
from test_cpu_stream_rows import RASTER_CASES, WAVEFRONT_CASES, WAVEFRONT_CASES_K3, case_of, oracle_row_streams

pytestmark = pytest.mark.gpu

_STATE = {}
PERSISTENT = ("generic", "pipelined", "batched", "wavefront")


def _exact_coder(lanes=1, rows=True, ks=5):
    """One coder per (lane count, rows, window) for the whole run, every parameter overwritten with the exact layers."""
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import (GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder,
                                                                            TopoGroupDynamicMaskConv2dContextModel as Ctx)
    key = ("coder", lanes, rows, ks)
    if key not in _STATE:
        kw = dict(stream_rows=True) if rows else {}
        if lanes != 1:
            kw["stream_lanes"] = lanes
        c = Coder(in_channels=C, default_topo_group_method="scanline", topo_group_context_model=Ctx(in_channels=C, out_channels=2 * C, kernel_size=ks),
                  **kw).eval().cuda()
        install(c, exact_params(ks))
        c.update_state()
        assert c.stream_rows is rows and c.stream_lanes == lanes
        _STATE[key] = c
    c = _STATE[key]
    c.use_persistent_scanline = True
    c.scanline_encode_schedule = "auto"
    c.persistent_scanline_max_batch = type(c).persistent_scanline_max_batch
    return c


class _Forced:
    """Forces one path of the coder in both directions -- "per-step", or a persistent kernel through BASIC_SCAN_KERNEL (which a
    row-stream decode call honours for the wavefront too) -- and restores what was there."""

    def __init__(self, coder, path):
        self.coder, self.path = coder, path

    def __enter__(self):
        c, p = self.coder, self.path
        self.saved = (c.use_persistent_scanline, os.environ.get("BASIC_SCAN_KERNEL"))
        os.environ.pop("BASIC_SCAN_KERNEL", None)
        c.use_persistent_scanline = p != "per-step"   # (None: nothing forced)
        if p in PERSISTENT:
            os.environ["BASIC_SCAN_KERNEL"] = p
        return self

    def __exit__(self, *exc):
        self.coder.use_persistent_scanline, env = self.saved
        os.environ.pop("BASIC_SCAN_KERNEL", None)
        if env is not None:
            os.environ["BASIC_SCAN_KERNEL"] = env


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _oracle(coder):
    if "oracle" not in _STATE:
        _STATE["oracle"] = oracle_encoder(coder._ans_params, coder.freq_precision, coder.use_bypass_coding, coder.bypass_precision)
    return _STATE["oracle"]


def _case(ks, B, H, W):
    yn, pn, ref = case_of(ks, B, H, W)
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


_RASTER = RASTER_CASES[:2]
STREAM_CASES = ([("wavefront", c, 1) for c in WAVEFRONT_CASES] + [("wavefront", c, 3) for c in WAVEFRONT_CASES_K3] +
                [(p, c, k) for p in ("generic", "pipelined", "per-step") for c in _RASTER for k in (1, 3)] +
                [("batched", c, k) for c in RASTER_CASES[2:] for k in (1, 3)])


@pytest.mark.parametrize("path,case,lanes", STREAM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_row_streams_are_the_oracles(path, case, lanes):
    """1. Every stream is the CPU rANS oracle's for that (row, lane) slice of the NumPy reference; the decoder returns the reference's
    bits; both directions ran the forced kernel; the body is at most 16 bytes per stream longer than the plain coder's body of the
    same call (test_cpu_stream_rows.py confirms the cap with the oracle alone)."""
    ks, B, H, W = case
    y, prior, ref = _case(ks, B, H, W)
    coder = _exact_coder(lanes, True, ks)
    want = oracle_row_streams(_oracle(coder), ref["sym"], ref["idx"], H, W, C, lanes)
    n = B * H * lanes
    with _Forced(coder, path):
        data = coder.encode(y, prior=prior)
        _check_kernel(coder, path)
        got = _split(data, n)
        bad = [s for s in range(n) if got[s] != want[s // (H * lanes)][s % (H * lanes)]]
        print(f"k={ks} B={B} {H}x{W} K={lanes} [{path}]: {len(data)} bytes, {len(bad)} of {n} row streams differ from the oracle's")
        assert not bad, bad[:8]
        yhat = coder.decode(data, prior=prior)
        _check_kernel(coder, path)
        md = int((_bits(yhat) != ref["ybuf"].view(np.int32)).sum())
        print(f"k={ks} B={B} {H}x{W} K={lanes} [{path}]: decoded ybuf bit diffs {md}")
        assert md == 0
    one = _exact_coder(1, False, ks).encode(y, prior=prior)
    print(f"k={ks} B={B} {H}x{W} K={lanes} [{path}]: plain body {len(one)} bytes, {(len(data) - len(one)) / n:.2f} extra bytes per stream")
    assert len(data) - len(one) <= SIZE_CAP_PER_STREAM * n


@pytest.mark.parametrize("lanes", [1, 3])
def test_encoder_and_decoder_need_not_agree_on_a_path(lanes):
    """2. Bytes of the per-step path decode through the wavefront, the batched and the pipelined kernel to the reference's bits, and
    theirs through the per-step path; all write the same bytes."""
    for B, H, W, kernel in [(2, 7, 9, "wavefront"), (3, 5, 7, "batched"), (2, 7, 9, "pipelined")]:
        y, prior, ref = _case(5, B, H, W)
        coder = _exact_coder(lanes)
        with _Forced(coder, "per-step"):
            slow = coder.encode(y, prior=prior)
        with _Forced(coder, kernel):
            fast = coder.encode(y, prior=prior)
            _check_kernel(coder, kernel)
            back = coder.decode(slow, prior=prior)
            _check_kernel(coder, kernel)
        assert fast == slow
        assert np.array_equal(_bits(back), ref["ybuf"].view(np.int32)), kernel
        with _Forced(coder, "per-step"):
            back = coder.decode(fast, prior=prior)
        assert np.array_equal(_bits(back), ref["ybuf"].view(np.int32)), kernel


@pytest.mark.parametrize("lanes", [1, 3])
def test_batch_invariance(lanes):
    """3. Image b's H * K streams in a call of five images are the streams of that image coded alone."""
    B, H, W = 5, 3, 4
    y, prior, _ = _case(5, B, H, W)
    coder = _exact_coder(lanes)
    per = H * lanes
    together = _split(coder.encode(y, prior=prior), B * per)
    for b in range(B):
        alone = _split(coder.encode(y[b: b + 1].contiguous(), prior=prior[b: b + 1].contiguous()), per)
        assert alone == together[b * per: (b + 1) * per], f"image {b}"


def _oracle_words(coder, ref, H, W, lanes):
    """Device words and offsets of the oracle's row streams of a reference case, and the streams."""
    streams = [s for img in oracle_row_streams(_oracle(coder), ref["sym"], ref["idx"], H, W, C, lanes) for s in img]
    woff = np.concatenate([[0], np.cumsum([len(s) // 4 for s in streams])]).astype(np.int64)
    return torch.from_numpy(np.frombuffer(b"".join(streams), dtype=np.int32).copy()).cuda(), torch.from_numpy(woff).cuda(), woff


@pytest.mark.parametrize("kernel,B,H,W,lanes", [("wavefront", 2, 3, 4, 1), ("wavefront", 5, 3, 4, 3), ("batched", 5, 3, 4, 3), ("batched", 2, 3, 4, 1),
                                                ("wavefront", 1, 65, 3, 1), ("pipelined", 5, 3, 4, 1)])
def test_decode_rows_guard_bands(kernel, B, H, W, lanes):
    """4. basic_scanline_decode_rows_dev on the oracle's streams with its outputs as views into sentinel-filled buffers: all of sym,
    idx and ybuf is written with the reference's values and nothing outside; a refusal ("does not fit": 65 rows are more than the
    wavefront's 64 columns, five images more than the pipelined kernel serves at this width) writes nothing."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    coder = _exact_coder(lanes)
    sl = _plan_of(coder, C)
    y, prior, ref = _case(5, B, H, W)
    n = H * W * C
    d_words, d_woff, _ = _oracle_words(coder, ref, H, W, lanes)
    table = coder._scale_table_dev.to(device="cuda", dtype=torch.float32).contiguous()
    off, fresh = 64, 0x7FC00001
    bufs = [torch.full((off + B * n + BAND,), GUARD, dtype=torch.int32, device="cuda") for _ in range(3)]
    for b in bufs:
        b[off: off + B * n] = fresh
    sym, idx, ybuf = (b[off: off + B * n] for b in bufs)
    refused = False
    before = sl.last_kernel()
    with _Forced(coder, kernel):
        try:
            _lib.check(_lib.lib().basic_scanline_decode_rows_dev(sl._h, coder._tables._h, d_words.data_ptr(), d_woff.data_ptr(), prior.data_ptr(), B,
                                                                 lanes, H, W, table.data_ptr(), table.numel(), sym.data_ptr(), idx.data_ptr(),
                                                                 ybuf.data_ptr(), K._stream()))
        except (RuntimeError, ValueError) as e:
            if "does not fit" not in str(e):
                raise
            refused = True
        sl.check()
    assert refused == (H > 64 or (kernel == "pipelined" and B > 2))
    for name, b in zip(("sym", "idx", "ybuf"), bufs):
        h = b.cpu()
        assert bool((h[:off] == GUARD).all()) and bool((h[off + B * n:] == GUARD).all()), f"the launch wrote outside {name}"
    if refused:
        assert all(bool((b[off: off + B * n] == fresh).all()) for b in bufs)
        assert sl.last_kernel() == before
        return
    assert sl.last_kernel() == kernel
    assert np.array_equal(sym.cpu().numpy().reshape(B, -1), ref["sym"]) and np.array_equal(idx.cpu().numpy().reshape(B, -1), ref["idx"])
    assert np.array_equal(ybuf.cpu().numpy().reshape(ref["ybuf"].shape), ref["ybuf"].view(np.int32))


@pytest.mark.parametrize("lanes", [1, 3])
def test_strided_streams_guard_bands(lanes):
    """4. basic_rans_decode_batch_streams_dev, one call per position as the per-step path makes them, on the oracle's row streams
    and a sentinel-filled buffer: B = 2, 3 x 4, C = 192.  Every stream is read to its end and none beyond."""
    B, H, W = 2, 3, 4
    n = H * W * C
    coder = _exact_coder(lanes)
    _, _, ref = _case(5, B, H, W)
    d_words, d_woff, woff = _oracle_words(coder, ref, H, W, lanes)
    d_idx = torch.from_numpy(ref["idx"].copy()).cuda()
    off, fresh = 64, 0x7FC00001
    out = torch.full((off + B * n + BAND,), GUARD, dtype=torch.int32, device="cuda")
    out[off: off + B * n] = fresh
    ns = B * H * lanes
    state = torch.zeros((ns,), device="cuda", dtype=torch.int64)
    pos = torch.full((ns,), -1, device="cuda", dtype=torch.int64)
    for p in range(H * W):
        coder._tables.decode_batch_streams(d_words, d_woff, d_idx, p * C, n, lanes, C // lanes, B, (p // W) * lanes, H * lanes, out[off:], state, pos)
    h = out.cpu().numpy()
    assert (h[:off] == GUARD).all() and (h[off + B * n:] == GUARD).all(), "the decoder wrote outside its symbols"
    assert np.array_equal(h[off: off + B * n].reshape(B, -1), ref["sym"])
    assert np.array_equal(pos.cpu().numpy(), np.diff(woff))
    # stream base 0 and stride `lanes` is the lanes entry: the same call, image after image, row after row
    out2 = torch.full_like(out, GUARD)
    state.zero_(); pos.fill_(-1)
    for p in range(H * W):
        for b in range(B):
            base = (b * H + p // W) * lanes
            coder._tables.decode_batch_streams(d_words, d_woff[base:], d_idx, b * n + p * C, n, lanes, C // lanes, 1, 0, lanes, out2[off:],
                                               state[base:], pos[base:])
    assert np.array_equal(out2.cpu().numpy()[off: off + B * n].reshape(B, -1), ref["sym"])


def test_refusals_on_the_host():
    """5. A wrong stream count (another batch's, a rows-off body, another lane count's) and a pgm raise ValueError; no launch is made."""
    coder = _exact_coder(3)
    sl = _plan_of(coder, C)
    B, H, W = 2, 3, 4
    y, prior, _ = _case(5, B, H, W)
    data = coder.encode(y, prior=prior)
    sl.check()
    plain = _exact_coder(1, False).encode(y, prior=prior)
    lanes_only = _exact_coder(3, False).encode(y, prior=prior)
    before = sl.last_kernel()
    pgm = torch.zeros(B, 1, H, W, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="pgm"):
        coder.encode(y, prior=prior, pgm=pgm)
    with pytest.raises(ValueError, match="pgm"):
        coder.decode(data, prior=prior, pgm=pgm)
    streams = _split(data, B * H * 3)
    keep = H * 3   # one image's streams: another batch's body
    body = struct.pack("<I", keep) + b"".join(struct.pack("<I", len(s)) for s in streams[:keep]) + b"".join(streams[:keep])
    for wrong in (body, plain, lanes_only):
        with pytest.raises(ValueError, match="streams"):
            coder.decode(wrong, prior=prior)
    with pytest.raises(ValueError, match="streams"):
        _exact_coder(1).decode(data, prior=prior)       # another lane count's
    with pytest.raises(ValueError, match="streams"):
        _exact_coder(3, False).decode(data, prior=prior)   # a rows-off coder
    assert sl.last_kernel() == before   # no launch was made


def test_planner_counts_the_row_wavefronts():
    """6. Two images of 32 rows are 64 columns, two column tiles of compute workgroups (a tile: one workgroup per 32-row tile of the
    context layer plus one per 32-row tile of the largest merger layer, 12 + 20 at this shape); at K = 12 their 768 streams need 192
    decoder workgroups beside them -- the last compute unit of a 256-unit chip, too many for a smaller one.  A forced wavefront is
    refused ("does not fit") exactly where compute + decoder workgroups exceed the device's compute units, and auto never takes it
    there; the call then goes to a raster kernel, whose decoder workgroups are those of B * K streams.  Either way it decodes to the
    reference's bits from streams that are the oracle's.  With rows off the planner answers what it answers without the argument."""
    from scanline_exact import layer_sizes
    B, H, W, lanes = 2, 32, 2, 12
    coder = _exact_coder(lanes)
    sl = _plan_of(coder, C)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    tl = coder._scale_table_dev.numel()
    per_tile = 2 * C // 32 + max(layer_sizes()[1:]) // 32
    tiles = math.ceil(B * H / 32)
    need = tiles * per_tile + math.ceil(B * H * lanes / 4)
    over = need > cus
    auto = sl.choose(B, H, W, tl, "auto", 4, coder._tables, lanes=lanes, rows=True)[0]
    print(f"{tiles} x {per_tile} compute + {math.ceil(B * H * lanes / 4)} decoder workgroups = {need} on {cus} compute units -> auto: {auto}")
    with _Forced(coder, "wavefront"):
        if over:
            with pytest.raises((RuntimeError, ValueError), match="does not fit"):
                sl.choose(B, H, W, tl, "auto", 4, coder._tables, lanes=lanes, rows=True)
        else:
            assert sl.choose(B, H, W, tl, "auto", 4, coder._tables, lanes=lanes, rows=True)[0] == "wavefront"
        # a decode call without row streams goes on ignoring the forced wavefront
        assert sl.choose(B, H, W, tl, "auto", 4, coder._tables, lanes=lanes, rows=False)[0] in ("pipelined", "generic")
    if over:
        assert auto in ("pipelined", "generic"), auto   # two images, 24 streams: six decoder workgroups
    for dec in (coder._tables, None):
        for k in (1, lanes):
            assert sl.choose(B, H, W, tl, "auto", 4, dec, lanes=k, rows=False) == sl.choose(B, H, W, tl, "auto", 4, dec, lanes=k)
    assert sl.choose(B, H, W, tl, "auto", 4, None, lanes=1, rows=True) == sl.choose(B, H, W, tl, "auto", 4, None)   # encode: no dependence
    y, prior, ref = _case(5, B, H, W)
    data = coder.encode(y, prior=prior)
    got = _split(data, B * H * lanes)
    want = oracle_row_streams(_oracle(coder), ref["sym"], ref["idx"], H, W, C, lanes)
    assert all(got[s] == want[s // (H * lanes)][s % (H * lanes)] for s in range(B * H * lanes))
    for path in ([] if over else ["wavefront"]) + [None]:   # at the residency limit where it fits; then what auto takes
        with _Forced(coder, path):
            yhat = coder.decode(data, prior=prior)
            sl.check()
            assert sl.last_kernel() == (path or auto)
        assert np.array_equal(_bits(yhat), ref["ybuf"].view(np.int32)), path


def _codecs():
    from cbench_basic_amd.presets import basic_codec, seed_synthetic_weights
    if "codecs" not in _STATE:
        made = []
        for kw in (dict(stream_rows=True), dict(stream_rows=False), dict()):
            torch.manual_seed(4321)   # (what seed_synthetic_weights leaves at its default initialisation comes from the global generator)
            c = seed_synthetic_weights(basic_codec(**kw), seed=0).eval().cuda()
            c.update_state()
            made.append(c)
        _STATE["codecs"] = made
    return _STATE["codecs"]


@pytest.mark.parametrize("level", [0, 7])
def test_codec_level(level):
    """7. BaSIC with row streams reconstructs exactly what the plain codec reconstructs, from a longer body; stream_rows=False writes
    the bytes of a codec built without the argument."""
    rows, off, plain = _codecs()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(11)).cuda()
    for c in (rows, off, plain):
        c.set_complex_level(level)
    assert rows.entropy_coder.latent_node_entropy_coders["y"].stream_rows is True
    assert plain.entropy_coder.latent_node_entropy_coders["y"].stream_rows is False
    dr, d0, dp = rows.compress(x), off.compress(x), plain.compress(x)
    assert d0 == dp
    assert dr != dp and len(dr) > len(dp)
    assert torch.equal(rows.decompress(dr), plain.decompress(dp))
