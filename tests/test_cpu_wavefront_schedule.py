"""The wavefront encode schedule of the scan-line coder (kernels.wavefront_schedule, the arithmetic csrc/scanline.hip walks):
row r runs s = ksize // 2 + 2 columns behind row r - 1.  Checked on the CPU: every position is coded exactly once, the left
neighbour is one step old and every other causal tap at least two (the kernel's late / early halves), and a tap outside the image
always lands on a slot that holds zeros in that step -- an idle row or a pad row above the image."""
import os
import re

import pytest

SHAPES = [(16, 16, 5), (32, 48, 5), (48, 32, 5), (1, 1, 5), (5, 1, 5), (3, 2, 5), (1, 6, 5), (4, 3, 3), (7, 9, 7), (2, 2, 5), (64, 1, 5)]


def _schedule(h, w, k):
    from cbench_basic_amd.nn.kernels import wavefront_schedule
    return wavefront_schedule(h, w, k)


def _taps(k):
    half = k // 2
    return [(dy, dx) for dy in range(-half, 1) for dx in range(-half, half + 1) if dy < 0 or dx < 0]


@pytest.mark.parametrize("h,w,k", SHAPES)
def test_step_count_and_every_position_once(h, w, k):
    steps, table = _schedule(h, w, k)
    s = k // 2 + 2
    assert steps == w + s * (h - 1) == len(table)
    seen = {}
    for t, row_cols in enumerate(table):
        assert len(row_cols) == h
        for r, c in enumerate(row_cols):
            if c is not None:
                assert 0 <= c < w and (r, c) not in seen
                seen[r, c] = t
    assert len(seen) == h * w


@pytest.mark.parametrize("h,w,k", SHAPES)
def test_tap_ages_and_out_of_image_taps(h, w, k):
    steps, table = _schedule(h, w, k)
    s = k // 2 + 2
    step_of = {(r, c): t for t, cols in enumerate(table) for r, c in enumerate(cols) if c is not None}
    for (r, c), t in step_of.items():
        for dy, dx in _taps(k):
            slab = t + dx + s * dy            # the step whose slab the kernel reads for this tap, at row r + dy
            age = t - slab
            assert age == 1 if (dy, dx) == (0, -1) else age >= 2
            nr, nc = r + dy, c + dx
            if 0 <= nr < h and 0 <= nc < w:
                assert step_of[nr, nc] == slab            # inside: that slab holds exactly the neighbour
            elif slab < 0:
                pass                                      # before the first step: the kernel skips the tap for every row
            elif nr < 0:
                assert -nr <= k // 2                      # a pad row above the image (k // 2 of them, zeros in every step)
            else:
                assert slab < steps and table[slab][nr] is None   # row nr is idle in that step: it published zeros


def test_header_declares_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "basic_hip.h")) as f:
        header = f.read()
    for name in ("basic_scanline_wavefront_max", "basic_scanline_last_kernel", "basic_scanline_set_encode_schedule"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
