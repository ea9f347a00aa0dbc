"""The band decode launch of the scan-line y-coder (scanline_decode_schedule = "band", row streams): the band
schedule's compute workgroups, one decoder wavefront per (image, slot, lane) that decodes the slot's rows one after the other, and as
many launches as the batch needs.  Addressing changes, arithmetic does not, so everything here is exact, against the yardsticks of
test_gpu_scanline_rows.py: the NumPy reference of scanline_exact.py and the CPU rANS oracle's row streams -- never another path of
the library.

The cases are the smallest shapes at which this launch can still go wrong (C = 192; s = ksize // 2 + 2, A = W // s + 1 slots):
W = s with two slots walking several rows back to back, three images in a tile; W < s, one slot coding every row with nothing but
idle steps between them; fewer rows than slots; three slots with a ragged last round of rows; the 3 x 3 window (s = 3, six slots,
five images per tile); a latent taller than the wavefront decode launch's 64 columns; and a batch of band_decode_max + 3 images,
which takes two launches, the second short."""
import math
import os

import numpy as np
import pytest
import torch

from scanline_cases import BAND, GUARD, _plan_of
from scanline_exact import C, layer_sizes
from test_cpu_stream_rows import oracle_row_streams
from test_gpu_scanline_rows import _Forced, _bits, _case, _exact_coder, _oracle, _oracle_words, _split

pytestmark = pytest.mark.gpu

CASES = [(5, 3, 9, 4), (5, 1, 5, 1), (5, 1, 1, 6), (5, 2, 7, 9), (3, 3, 16, 16), (5, 1, 70, 3)]
CASES_K3 = [(5, 2, 7, 9), (3, 3, 16, 16)]
TWO_LAUNCHES = (5, None, 4, 4)   # K = 3, B = band_decode_max(4, 4, lanes = 3) + 3


def _coder(lanes=1, rows=True, ks=5):
    c = _exact_coder(lanes, rows, ks)
    c.scanline_decode_schedule = "auto"
    return c


class _Band:
    """The band decode launch, asked for through the coder's attribute ("attr") or BASIC_SCAN_KERNEL=band ("env", which forces the
    band encode schedule too); restores what was there."""

    def __init__(self, coder, how="attr", schedule="band"):
        self.coder, self.how, self.schedule = coder, how, schedule

    def __enter__(self):
        c = self.coder
        self.saved = (c.use_persistent_scanline, c.scanline_decode_schedule, os.environ.get("BASIC_SCAN_KERNEL"))
        os.environ.pop("BASIC_SCAN_KERNEL", None)
        c.use_persistent_scanline = True
        if self.how == "env":
            os.environ["BASIC_SCAN_KERNEL"] = self.schedule
        else:
            c.scanline_decode_schedule = self.schedule
        return self

    def __exit__(self, *exc):
        c = self.coder
        c.use_persistent_scanline, c.scanline_decode_schedule, env = self.saved
        plan = (c._layers or {}).get("scanline", (None,))[0]
        if plan is not None:   # (the plan keeps the schedule of the coder's last decode call: the coders are shared with other test files)
            plan.set_decode_schedule("auto")
        os.environ.pop("BASIC_SCAN_KERNEL", None)
        if env is not None:
            os.environ["BASIC_SCAN_KERNEL"] = env


def _sl(coder):
    return _plan_of(coder, C)


def _resolve(case, lanes):
    """(ks, B, H, W) with the two-launch case's batch taken from the library: three images more than one launch decodes."""
    ks, B, H, W = case
    if B is None:
        coder = _coder(lanes, True, ks)
        B = _sl(coder).band_decode_max(coder._tables, H, W, lanes) + 3
        assert B > 3
    return ks, B, H, W


def _band_decoded(coder, data, prior):
    """coder.decode under the band, which must have run and finished clean."""
    with _Band(coder):
        out = coder.decode(data, prior=prior)
        sl = coder._layers["scanline"][0]
        sl.check()
        assert sl.last_kernel() == "band", sl.last_kernel()
    return out


STREAM_CASES = [(c, 1, "attr") for c in CASES] + [(c, 3, "attr") for c in CASES_K3] + [(TWO_LAUNCHES, 3, "attr"), (CASES[0], 1, "env")]


@pytest.mark.parametrize("case,lanes,how", STREAM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_oracle_streams_in_reference_bits_out(case, lanes, how):
    """1. The coder's body is the CPU rANS oracle's row streams of the NumPy reference, stream by stream, and coder.decode under the
    band returns the reference's float bits; the band ran (no case is refused on a chip where the test runs: a refusal raises), and
    its barriers completed.  The two-launch case must take two launches."""
    ks, B, H, W = _resolve(case, lanes)
    y, prior, ref = _case(ks, B, H, W)
    coder = _coder(lanes, True, ks)
    sl = _sl(coder)
    n = B * H * lanes
    want = oracle_row_streams(_oracle(coder), ref["sym"], ref["idx"], H, W, C, lanes)
    with _Band(coder, how):
        data = coder.encode(y, prior=prior)
        got = _split(data, n)
        bad = [s for s in range(n) if got[s] != want[s // (H * lanes)][s % (H * lanes)]]
        print(f"k={ks} B={B} {H}x{W} K={lanes} [{how}]: {len(data)} bytes, {len(bad)} of {n} row streams differ from the oracle's")
        assert not bad, bad[:8]
        per_launch = sl.band_decode_max(coder._tables, H, W, lanes)
        assert per_launch >= 1, "the band decode launch does not fit this chip"
        yhat = coder.decode(data, prior=prior)
        sl.check()
        assert sl.last_kernel() == "band", sl.last_kernel()
        # (the plan carries the coder's decode schedule from the decode call on: what the planner says of the call it just planned)
        planned = sl.choose(B, H, W, coder._scale_table_dev.numel(), "auto", coder.persistent_scanline_max_batch, coder._tables, lanes=lanes, rows=True)
        assert planned == ("band", math.ceil(B / per_launch)), planned
        if case[1] is None:
            assert planned[1] == 2
        md = int((_bits(yhat) != ref["ybuf"].view(np.int32)).sum())
        print(f"k={ks} B={B} {H}x{W} K={lanes} [{how}]: {planned[1]} launch(es) of {per_launch} images, decoded ybuf bit diffs {md}")
        assert md == 0


@pytest.mark.parametrize("lanes", [1, 3])
def test_paths_need_not_agree(lanes):
    """2. Bytes written under the per-step path decode through the band to the reference's bits; the band's input decodes through the
    per-step path and through the batched kernel to the same bits."""
    for ks, B, H, W in [(5, 3, 9, 4), (5, 3, 5, 7)]:
        y, prior, ref = _case(ks, B, H, W)
        coder = _coder(lanes)
        with _Forced(coder, "per-step"):
            slow = coder.encode(y, prior=prior)
        back = _band_decoded(coder, slow, prior)
        assert np.array_equal(_bits(back), ref["ybuf"].view(np.int32))
        with _Band(coder, "env"):   # (the band encode schedule writes the band's input)
            fast = coder.encode(y, prior=prior)
        assert fast == slow
        for path in ("per-step", "batched"):
            with _Forced(coder, path):
                back = coder.decode(fast, prior=prior)
                if path != "per-step":
                    sl = coder._layers["scanline"][0]
                    sl.check()
                    assert sl.last_kernel() == path
            assert np.array_equal(_bits(back), ref["ybuf"].view(np.int32)), path


@pytest.mark.parametrize("case,lanes", [((5, 3, 9, 4), 1), ((5, 2, 7, 9), 3), (TWO_LAUNCHES, 3)], ids=str)
def test_batch_invariance(case, lanes):
    """3. Image i of a band-decoded batch is, bit for bit, the same image band-decoded alone (the two-launch case: the first image,
    the two on either side of the launch boundary, and the last)."""
    ks, B, H, W = _resolve(case, lanes)
    y, prior, _ = _case(ks, B, H, W)
    coder = _coder(lanes, True, ks)
    together = _bits(_band_decoded(coder, coder.encode(y, prior=prior), prior))
    per_launch = _sl(coder).band_decode_max(coder._tables, H, W, lanes)
    images = range(B) if case[1] is not None else sorted({0, per_launch - 1, per_launch, B - 1})
    for b in images:
        yb, pb = y[b: b + 1].contiguous(), prior[b: b + 1].contiguous()
        alone = _bits(_band_decoded(coder, coder.encode(yb, prior=pb), pb))
        assert np.array_equal(alone[0], together[b]), f"image {b}"


@pytest.mark.parametrize("case,lanes", [((5, 2, 3, 4), 1), ((5, 5, 3, 4), 3), (TWO_LAUNCHES, 3), ((5, 1, 3, 130), 1)], ids=str)
def test_decode_rows_guard_bands(case, lanes):
    """4. basic_scanline_decode_rows_dev under the band decode schedule on the oracle's streams, its outputs views into
    sentinel-filled buffers: every element of sym, idx and ybuf is written with the reference's value, nothing outside.  A shape the
    planner has no band launch for (3 x 130: 33 slots do not fit a 32-column tile, band_decode_max == 0) is refused with "does not
    fit", writes nothing and leaves last_kernel() alone."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    ks, B, H, W = _resolve(case, lanes)
    coder = _coder(lanes, True, ks)
    sl = _sl(coder)
    y, prior, ref = _case(ks, B, H, W)
    n = H * W * C
    d_words, d_woff, _ = _oracle_words(coder, ref, H, W, lanes)
    table = coder._scale_table_dev.to(device="cuda", dtype=torch.float32).contiguous()
    off, fresh = 64, 0x7FC00001
    bufs = [torch.full((off + B * n + BAND,), GUARD, dtype=torch.int32, device="cuda") for _ in range(3)]
    for b in bufs:
        b[off: off + B * n] = fresh
    sym, idx, ybuf = (b[off: off + B * n] for b in bufs)
    fits = sl.band_decode_max(coder._tables, H, W, lanes) >= 1
    assert fits == (W != 130)
    refused = False
    before = sl.last_kernel()
    saved = os.environ.pop("BASIC_SCAN_KERNEL", None)
    sl.set_decode_schedule("band")
    try:
        _lib.check(_lib.lib().basic_scanline_decode_rows_dev(sl._h, coder._tables._h, d_words.data_ptr(), d_woff.data_ptr(), prior.data_ptr(), B,
                                                             lanes, H, W, table.data_ptr(), table.numel(), sym.data_ptr(), idx.data_ptr(),
                                                             ybuf.data_ptr(), K._stream()))
    except (RuntimeError, ValueError) as e:
        if "does not fit" not in str(e):
            raise
        refused = True
    finally:
        sl.set_decode_schedule("auto")
        if saved is not None:
            os.environ["BASIC_SCAN_KERNEL"] = saved
    sl.check()
    assert refused == (not fits)
    for name, b in zip(("sym", "idx", "ybuf"), bufs):
        h = b.cpu()
        assert bool((h[:off] == GUARD).all()) and bool((h[off + B * n:] == GUARD).all()), f"the launch wrote outside {name}"
    if refused:
        assert all(bool((b[off: off + B * n] == fresh).all()) for b in bufs)
        assert sl.last_kernel() == before
        return
    assert sl.last_kernel() == "band"
    assert np.array_equal(sym.cpu().numpy().reshape(B, -1), ref["sym"]) and np.array_equal(idx.cpu().numpy().reshape(B, -1), ref["idx"])
    assert np.array_equal(ybuf.cpu().numpy().reshape(ref["ybuf"].shape), ref["ybuf"].view(np.int32))


def test_planner_counts_the_slot_wavefronts():
    """5. A launch of n images holds ceil(n / (32 // A)) column tiles of compute workgroups (a tile: one workgroup per 32-row tile of
    the context layer plus one per 32-row tile of the largest merger layer, 12 + 20 at this shape) and ceil(n * min(A, H) * K / 4)
    decoder workgroups, all resident: band_decode_max is the largest n <= band_max for which they fit the device's compute units.
    Under the schedule a row-stream call of B images is planned as ceil(B / n) band launches; a call without row streams is planned
    as it is today."""
    coder = _coder(1)
    sl = _sl(coder)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    tl, gate = coder._scale_table_dev.numel(), coder.persistent_scanline_max_batch
    per_tile = 2 * C // 32 + max(layer_sizes()[1:]) // 32
    s = 5 // 2 + 2
    for H, W, lanes in [(32, 48, 1), (32, 48, 3), (32, 48, 12), (16, 16, 1)]:
        A = W // s + 1
        ipt = 32 // A
        fits = [n for n in range(1, sl.band_max(H, W) + 1) if math.ceil(n / ipt) * per_tile + math.ceil(n * min(A, H) * lanes / 4) <= cus]
        n = max(fits, default=0)
        got = sl.band_decode_max(coder._tables, H, W, lanes)
        print(f"{H}x{W} K={lanes}: {A} slots, {ipt} images per tile of {per_tile} workgroups, band_max {sl.band_max(H, W)} on {cus} compute units -> "
              f"band_decode_max {got}, restated {n}")
        assert got == n
        if n == 0:
            continue
        for B in (1, n, n + 1, 2 * n + 1):
            today = sl.choose(B, H, W, tl, "auto", gate, coder._tables, lanes=lanes, rows=False)
            assert sl.choose(B, H, W, tl, "auto", gate, coder._tables, lanes=lanes, rows=True)[0] != "band"   # auto stays as it is
            sl.set_decode_schedule("band")
            try:
                assert sl.choose(B, H, W, tl, "auto", gate, coder._tables, lanes=lanes, rows=True) == ("band", math.ceil(B / n))
                assert sl.choose(B, H, W, tl, "auto", gate, coder._tables, lanes=lanes, rows=False) == today
                assert sl.choose(B, H, W, tl, "auto", gate, None) == sl.choose(B, H, W, tl, "auto", gate, None, rows=True)   # encode: no dependence
            finally:
                sl.set_decode_schedule("auto")


def test_refusals_on_the_host():
    """6. "band" (or "wavefront") on a coder without row streams, and an unknown schedule name, raise ValueError when the call is made;
    no launch is made."""
    B, H, W = 2, 3, 4
    y, prior, _ = _case(5, B, H, W)
    plain = _coder(1, False)
    sl = _sl(plain)
    data = plain.encode(y, prior=prior)
    sl.check()
    before = sl.last_kernel()
    for bad in ("band", "wavefront", "diagonal"):
        with _Band(plain, "attr", bad):
            with pytest.raises(ValueError, match="scanline_decode_schedule"):
                plain.decode(data, prior=prior)
    rows = _coder(1, True)
    data = rows.encode(y, prior=prior)
    before_rows = _sl(rows).last_kernel()
    with _Band(rows, "attr", "diagonal"):
        with pytest.raises(ValueError, match="scanline_decode_schedule"):
            rows.decode(data, prior=prior)
    with pytest.raises(ValueError, match="decode schedule"):
        sl.set_decode_schedule("diagonal")
    assert sl.last_kernel() == before and _sl(rows).last_kernel() == before_rows   # no launch was made
    assert plain.scanline_decode_schedule == "auto" and type(plain).scanline_decode_schedule == "auto"


_STATE = {}


def _codec():
    from cbench_basic_amd.presets import basic_codec, seed_synthetic_weights
    if "codec" not in _STATE:
        with pytest.raises(ValueError, match="stream_rows"):
            basic_codec(scanline_decode_schedule="band")
        torch.manual_seed(4321)
        c = seed_synthetic_weights(basic_codec(stream_rows=True, scanline_decode_schedule="band"), seed=0).eval().cuda()
        c.update_state()
        assert c.entropy_coder.latent_node_entropy_coders["y"].scanline_decode_schedule == "band"
        _STATE["codec"] = c
    return _STATE["codec"]


@pytest.mark.parametrize("level", [0, 7])
def test_codec_level(level):
    """7. BaSIC with row streams decompresses the same bytes to the same images under the band and under the raster decode schedule,
    and the y-coder's plan says which launch ran."""
    codec = _codec()
    yc = codec.entropy_coder.latent_node_entropy_coders["y"]
    x = torch.rand(3, 3, 128, 128, generator=torch.Generator().manual_seed(11)).cuda()
    codec.set_complex_level(level)
    saved = os.environ.pop("BASIC_SCAN_KERNEL", None)
    try:
        data = codec.compress(x)
        out = {}
        for schedule in ("band", "raster"):
            yc.scanline_decode_schedule = schedule
            out[schedule] = codec.decompress(data)
            sl = yc._layers["scanline"][0]
            sl.check()
            ran = sl.last_kernel()
            print(f"level {level}: {len(data)} bytes, decode schedule {schedule} -> {ran}")
            assert (ran == "band") == (schedule == "band") and ran != "wavefront", ran
    finally:
        yc.scanline_decode_schedule = "band"
        if saved is not None:
            os.environ["BASIC_SCAN_KERNEL"] = saved
    assert torch.equal(out["band"], out["raster"])
