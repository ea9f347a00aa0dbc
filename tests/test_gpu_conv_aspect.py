"""GPU: tall, narrow inputs through every conv kernel family, against the fp64 reference and the bounds of conv_ref.py.

tile_shape() (csrc/conv.hip) lets a workgroup tile become a column where the position grid is narrow: the tile width is
pow2_ceil(mw) <= 16 and the height takes what is left of the 128 / 256 positions, so a grid 2 positions wide runs tiles of
2 x 64 or 2 x 128.  The LDS patch of such a tile has (th - 1) * s_in + span_y rows; where it exceeds the stage budget or
the gather descriptors with one image per tile, the launch drops the 16-byte patch rows first and then halves the tile
height (dead lanes, as for tiny maps).  The other conv tests stay below 70 rows and columns and near-square; here every
shape is a column (with one row-shaped control per family), so that the lane-to-position arithmetic of the tall tiles,
the gather descriptors at a large patch height, the reduced tiles and the split-fp16 kernel's choice between LDS patch
and direct loads (tb * (th + kh - 1) * (tw + kw - 1) <= 416 positions) are all executed.

Every check, bound and constant comes from conv_ref.py; nothing is skipped: a refused launch (BasicHipError) fails.
"""
import pytest
import torch

from conv_ref import (RMS_FLOOR, SPLIT_RMS_FACTOR, Case, _bound_a, _check_bound, _check_exact, _gdn_bound, _guarded_run,
                      _layer, _linear64, _plan, _run, _seed)

pytestmark = pytest.mark.gpu

# class: cin, cout, k, s, p, op, transposed, activation, BASIC_CONV_DEBUG, BASIC_CONV_F32
CLASSES = {
    # forward, 8 waves (GDN, 4 M-tiles, more than 9 taps): 5x5 unrolled at both strides, 4x4 by the tap table
    "w8_k5s2": (32, 128, 5, 2, 2, 0, False, "gdn", "", False),
    "w8_k5s1": (32, 128, 5, 1, 2, 0, False, "gdn", "", False),
    "w8_k4s2": (32, 128, 4, 2, 1, 0, False, "gdn", "", False),
    "first": (3, 128, 5, 2, 2, 0, False, "gdn", "", False),                # the persistent first-layer kernel
    "plain_mt6_chunks": (24, 192, 5, 2, 2, 0, False, "none", "8", False),  # 6 M-tiles in one launch
    "plain_mt6_slices": (24, 192, 5, 2, 2, 0, False, "none", "4", False),  # 32-channel slices over gridDim.y
    "k3": (24, 128, 3, 1, 1, 0, False, "relu", "", False),
    # k5 s2 p2 op1 transposed
    "fused": (24, 128, 5, 2, 2, 1, True, "relu", "", False),               # fused column phases
    "fused_igdn_f32": (24, 100, 5, 2, 2, 1, True, "igdn", "", False),      # cin % 16 != 0: no split-fp16 variant
    "tr_mt6": (24, 192, 5, 2, 2, 1, True, "leaky", "", False),
    "split": (32, 128, 5, 2, 2, 1, True, "igdn", "", False),               # the split-fp16 kernel
    "split_f32": (32, 128, 5, 2, 2, 1, True, "igdn", "", True),            # ... and the fp32 kernel of the same layer
    "cout3": (8, 3, 5, 2, 2, 1, True, "none", "", False),
}
FORWARD = ("w8_k5s2", "w8_k5s1", "w8_k4s2", "first", "plain_mt6_chunks", "plain_mt6_slices", "k3")
TRANSPOSED = ("fused", "fused_igdn_f32", "tr_mt6", "split", "split_f32", "cout3")
WAVES8 = ("w8_k5s2", "w8_k5s1", "w8_k4s2", "first")
# H x W of the input; the last line of each list are the row-shaped controls
FORWARD_SHAPES = [(64, 16), (34, 12), (66, 8), (64, 8), (66, 4), (132, 4), (260, 2), (260, 1), (9, 4),
                  (16, 64), (1, 260)]
TRANSPOSED_SHAPES = [(64, 1), (66, 1), (130, 1), (65, 2), (130, 2), (65, 4), (33, 8),
                     (1, 130)]
SPLIT_PATCH_LIMIT = [(64, 4), (128, 2)]   # 1 x 64 x 4 tile: 66 x 6 = 396 patch positions; 1 x 128 x 2: 130 x 4 = 520 > 416


def _case(cls, B, H, W, debug=None):
    cin, cout, k, s, p, op, tr, act, dbg, _ = CLASSES[cls]
    return Case(cin, cout, k, s, p, op, tr, act, B, H, W, dbg if debug is None else debug, 0)


def _has_output(c):
    """A k4 s2 p1 convolution of a 1-wide (or 1-tall) input has no output position: not a case."""
    if c.tr:
        return True
    return (c.H + 2 * c.p - c.k) // c.s + 1 >= 1 and (c.W + 2 * c.p - c.k) // c.s + 1 >= 1


def _cases():
    out = []
    for cls in FORWARD:
        out += [(cls, _case(cls, 1, h, w)) for h, w in FORWARD_SHAPES]
    for cls in WAVES8:   # tb starts above 1 and is halved
        out += [(cls, _case(cls, 3, h, w)) for h, w in ((9, 4), (64, 8))]
    for cls in TRANSPOSED:
        out += [(cls, _case(cls, 1, h, w)) for h, w in TRANSPOSED_SHAPES]
    out.append(("fused", _case("fused", 3, 33, 8)))
    for cls in ("split", "split_f32"):   # one shape on each side of the split-fp16 kernel's patch limit
        out += [(cls, _case(cls, 1, h, w)) for h, w in SPLIT_PATCH_LIMIT]
    out += [("split", _case("split", 1, h, w, debug="1024")) for h, w in SPLIT_PATCH_LIMIT]   # ... by direct loads only
    return [(cls, c) for cls, c in out if _has_output(c)]


CASES = _cases()


def _id(v):
    cls, c = v
    return f"{cls}-{c.H}x{c.W}" + (f"-B{c.B}" if c.B != 1 else "") + (f"-dbg{c.debug}" if c.debug and "mt6" not in cls else "")


def _f32(cls):
    return CLASSES[cls][9]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_aspect_exact_integers(case, monkeypatch):
    cls, c = case
    x, w, b, gamma, beta = _layer(c, True, _seed(cls, tuple(c), "int"))
    plan = _plan(c, w, b, gamma, beta)
    got = _run(plan, x, monkeypatch, c.debug, f32=_f32(cls))
    _check_exact(c, got, _linear64(c, x, w, b), beta)


def _check_split(c, plan, x, lin, A, monkeypatch, what):
    """What test_split_geometry asserts of the split-fp16 kernel: both kernels within TAU * A per element, different
    bits, and the split kernel's RMS(err / A) within SPLIT_RMS_FACTOR of the fp32 kernel's on the same inputs."""
    got = _run(plan, x, monkeypatch, c.debug)
    got32 = _run(plan, x, monkeypatch, c.debug, f32=True)
    assert not torch.equal(got, got32), "the split-fp16 path did not run"
    r, r32 = _check_bound(c, got, lin, A, what + " split"), _check_bound(c, got32, lin, A, what + " fp32")
    rms, rms32 = float(r.pow(2).mean().sqrt()), float(r32.pow(2).mean().sqrt())
    assert rms <= SPLIT_RMS_FACTOR * rms32 + RMS_FLOOR, (rms, rms32)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_aspect_randn_bound(case, monkeypatch):
    cls, c = case
    x, w, b, gamma, beta = _layer(c, False, _seed(cls, tuple(c), "randn"))
    plan = _plan(c, w, b, gamma, beta)
    lin, A = _linear64(c, x, w, b), _bound_a(c, x, w, b)
    if cls == "split":
        _check_split(c, plan, x, lin, A, monkeypatch, _id(case))
    else:
        _check_bound(c, _run(plan, x, monkeypatch, c.debug, f32=_f32(cls)), lin, A, _id(case))


@pytest.mark.parametrize("case", [v for v in CASES if v[1].act in ("gdn", "igdn")], ids=_id)
def test_aspect_gdn_real_gamma(case, monkeypatch):
    cls, c = case
    x, w, b, gamma, beta = _layer(c, False, _seed(cls, tuple(c), "gamma"), gamma_kind="real")
    plan = _plan(c, w, b, gamma, beta)
    got = _run(plan, x, monkeypatch, c.debug, f32=_f32(cls))
    _gdn_bound(c, got, _linear64(c, x, w, b), _bound_a(c, x, w, b), gamma, beta)


# ---------------------------------------------------------------------------------------------------------------------
# guard bands: one tall shape of each kernel family

GUARDED = [("w8_k5s2", 64, 16), ("first", 132, 4), ("fused", 66, 1), ("split", 128, 2), ("cout3", 130, 4)]


@pytest.mark.parametrize("cls,H,W", GUARDED, ids=lambda v: str(v))
def test_aspect_guard_bands(cls, H, W, monkeypatch):
    """Integer data into an output view at an aligned offset and at 1 float: every element written and exact, the bands
    bitwise unchanged.  (At 1 float the transposed layers of more than 3 channels take their four-phase fallback.)"""
    c = _case(cls, 1, H, W)
    x, w, b, gamma, beta = _layer(c, True, _seed(cls, tuple(c), "guard"))
    plan = _plan(c, w, b, gamma, beta)
    lin = _linear64(c, x, w, b)
    for out_off in (64, 1):
        _check_exact(c, _guarded_run(plan, c, x, 64, out_off, monkeypatch, c.debug), lin, beta)


# ---------------------------------------------------------------------------------------------------------------------
# an image's bits do not depend on the batch it is run in


@pytest.mark.parametrize("cls,H,W", [("w8_k5s2", 66, 8), ("fused", 66, 1), ("split", 65, 4)], ids=lambda v: str(v))
def test_aspect_batch_invariant(cls, H, W, monkeypatch):
    c = _case(cls, 3, H, W)
    x, w, b, gamma, beta = _layer(c, False, _seed(cls, tuple(c), "batch"), gamma_kind="real")
    plan = _plan(c, w, b, gamma, beta)
    together = _run(plan, x, monkeypatch, c.debug)
    for i in range(3):
        alone = _run(plan, x[i:i + 1].contiguous(), monkeypatch, c.debug)
        assert torch.equal(together[i], alone[0]), f"image {i} differs between the batch of 3 and its own run"
