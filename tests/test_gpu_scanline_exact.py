"""Every scan-line path at the BaSIC shape (C = 192: context 192 -> 384, merger 768 -> 640 -> 512 -> 384) against the plain NumPy
fp64 raster loop of scanline_exact.py -- never against another path of the library.  The layers, the latent and the prior are
chosen so that all arithmetic is exact in fp32 in any summation order (test_cpu_scanline_exact.py holds the premises), and the
0.5-step scale table puts scales on table entries and exactly between them and residuals on k + 1/2.  So the per-step path and the
five persistent kernels (generic, pipelined, batched, and the batched kernel's wavefront and band encode schedules) must give the
reference's symbols, table rows and the float BITS of the coded latent, with no tolerance, and the decoder must return those
bits from the coder's own bytes.  What this pins that "equals the per-step path" does not: the causal window, the row lag
s = k / 2 + 2 of the wavefront, the band's slot mapping, the order of cat(ctx, prior), first-minimum and round-half-even on ties.

Every scale here is finite.  Infinite and NaN scales are left to test_gpu_entropy_kernels.py (the per-step path's Gaussian step,
where they are defined as table row 0).  The persistent kernels' encoders consume the last layer's outputs in the lanes that
computed them, but their decoders hand a position's table rows and means to the decoder wavefronts through the tagged exchange
(st_gran in csrc/scanline.hip), so the last layer's outputs do pass through it and non-finite ones are not run through these
kernels here."""
import os

import numpy as np
import pytest
import torch

from scanline_cases import BAND, GUARD, _coder, _plan_of
from scanline_exact import C, exact_case, exact_params, install

pytestmark = pytest.mark.gpu

_CODERS = {}


def _exact_coder(ks):
    """One coder per window size for the whole run, its layers overwritten with the exact ones."""
    if ks not in _CODERS:
        c = _coder("ctxmodel" if ks == 5 else f"ctxmodel-k{ks}", C)
        install(c, exact_params(ks))
        c.update_state()
        _CODERS[ks] = c
    c = _CODERS[ks]
    c.use_persistent_scanline = True
    c.scanline_encode_schedule = "auto"
    return c


class _Forced:
    """Forces one path of the coder -- "per-step", a kernel through BASIC_SCAN_KERNEL or an encode schedule -- and restores it."""

    def __init__(self, coder, path):
        self.coder, self.path = coder, path

    def __enter__(self):
        c, p = self.coder, self.path
        self.saved = (c.use_persistent_scanline, c.scanline_encode_schedule, os.environ.get("BASIC_SCAN_KERNEL"))
        os.environ.pop("BASIC_SCAN_KERNEL", None)
        c.use_persistent_scanline = p != "per-step"
        c.scanline_encode_schedule = p if p in ("wavefront", "band") else "auto"
        if p in ("generic", "pipelined", "batched"):
            os.environ["BASIC_SCAN_KERNEL"] = p
        return self

    def __exit__(self, *exc):
        c = self.coder
        c.use_persistent_scanline, c.scanline_encode_schedule, env = self.saved
        os.environ.pop("BASIC_SCAN_KERNEL", None)
        if env is not None:
            os.environ["BASIC_SCAN_KERNEL"] = env


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _check_case(path, ks, B, H, W):
    """-> whether `path` ran the case (False: it refused the shape with "does not fit")."""
    coder = _exact_coder(ks)
    yn, pn, ref = exact_case(ks, B, H, W, 1000 * B + 10 * H + W)
    y, prior = torch.from_numpy(yn.copy()).cuda(), torch.from_numpy(pn.copy()).cuda()
    with _Forced(coder, path):
        try:
            s, i, yb, _ = coder._run_encode(y, prior)
        except (RuntimeError, ValueError) as e:
            if "does not fit" not in str(e):
                raise
            print(f"k={ks} B={B} {H}x{W} [{path}]: refused ({e})")
            return False
        if path != "per-step":
            sl = coder._layers["scanline"][0]
            sl.check()
            assert sl.last_kernel() == path, sl.last_kernel()
        ms, mi = int((s.cpu().numpy() != ref["sym"]).sum()), int((i.cpu().numpy() != ref["idx"]).sum())
        my = int((_bits(yb) != ref["ybuf"].view(np.int32)).sum())
        print(f"k={ks} B={B} {H}x{W} [{path}]: symbol diffs {ms}, index diffs {mi}, ybuf bit diffs {my} of {ref['sym'].size}")
        assert ms == 0 and mi == 0 and my == 0
        data = coder.encode(y, prior=prior)
        if path != "per-step":
            sl.check()
            assert sl.last_kernel() == path, sl.last_kernel()
        yhat = coder.decode(data, prior=prior)
        if path != "per-step":
            sl.check()
            if path in ("generic", "pipelined", "batched"):   # (the decoder has no wavefront and no band: it takes what auto gives it)
                assert sl.last_kernel() == path, sl.last_kernel()
        md = int((_bits(yhat) != ref["ybuf"].view(np.int32)).sum())
        print(f"k={ks} B={B} {H}x{W} [{path}]: decoded ybuf bit diffs {md}")
        assert md == 0
    return True


# (ks, B, H, W); B None: three images more than one launch of the band holds (two launches)
_LANE = [(5, 1, 5, 6), (5, 2, 3, 2), (5, 2, 7, 9)]   # 2x3x2: narrower than s = 4 (the pipelined kernel refuses it)
CASES = {
    "per-step": _LANE,
    "generic": _LANE,
    "pipelined": _LANE,
    "batched": [(5, 33, 2, 6), (5, 3, 5, 7)],              # two column tiles, the second one ragged; one ragged tile
    "wavefront": [(5, 2, 7, 9), (5, 1, 16, 16), (3, 1, 4, 3)],
    "band": [(5, 3, 9, 4), (5, 1, 5, 1), (5, 1, 1, 6), (3, 3, 16, 16), (5, None, 4, 4)],   # 1x5x1: W < s; 1x1x6: fewer rows than slots
}


@pytest.mark.parametrize("path", list(CASES))
def test_path_codes_the_reference_integers(path):
    """Each path on its cases: the NumPy reference's symbols, table rows and coded-latent bits, the same bits back from the decoder,
    and at least two cases that the path did not refuse."""
    ran = 0
    for ks, B, H, W in CASES[path]:
        if B is None:
            per_launch = _plan_of(_exact_coder(ks), C).band_max(H, W)
            assert per_launch >= 1
            B = per_launch + 3
        ran += _check_case(path, ks, B, H, W)
    assert ran >= 2, f"{path} ran {ran} of its cases"


@pytest.mark.parametrize("kernel", ["generic", "pipelined", "batched"])
@pytest.mark.parametrize("B,H,W", [(2, 3, 4), (5, 3, 4)])
def test_decode_guard_bands(kernel, B, H, W):
    """basic_scanline_decode_dev with symbols, table rows and the decoded latent as views into sentinel-filled buffers, on the coder's
    own stream of an exact case: the launch writes all of each view -- the reference's values -- and nothing outside; a kernel that
    refuses the batch ("does not fit": the pipelined one above two images) writes nothing at all."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    coder = _exact_coder(5)
    sl = _plan_of(coder, C)
    yn, pn, ref = exact_case(5, B, H, W, 1000 * B + 10 * H + W)
    y, prior = torch.from_numpy(yn.copy()).cuda(), torch.from_numpy(pn.copy()).cuda()
    n = H * W * C
    with _Forced(coder, "generic"):
        s, i, _, _ = coder._run_encode(y, prior)
        sl.check()
    words, woff = coder._tables.encode_batch_end(coder._tables.encode_batch_begin(s.reshape(-1), i.reshape(-1), n))   # one stream per image
    d_words = torch.from_numpy(words[: int(woff[-1])].view(np.int32).copy()).cuda()
    d_woff = torch.from_numpy(woff.astype(np.int64)).cuda()
    table = coder._scale_table_dev.to(device="cuda", dtype=torch.float32).contiguous()
    off, fresh = 64, 0x7FC00001   # (a NaN as float, no symbol or table row as integer)
    bufs = [torch.full((off + B * n + BAND,), GUARD, dtype=torch.int32, device="cuda") for _ in range(3)]
    for b in bufs:
        b[off: off + B * n] = fresh
    sym, idx, ybuf = (b[off: off + B * n] for b in bufs)
    refused = False
    with _Forced(coder, kernel):
        try:
            _lib.check(_lib.lib().basic_scanline_decode_dev(sl._h, coder._tables._h, d_words.data_ptr(), d_woff.data_ptr(), prior.data_ptr(), B, H, W,
                                                            table.data_ptr(), table.numel(), sym.data_ptr(), idx.data_ptr(), ybuf.data_ptr(), K._stream()))
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
