"""The premises of tests/test_gpu_msssim.py, checked without a GPU: the fp64 evaluation of tests/msssim_exact.py and the package's
torch restatement (benchmark/ms_ssim.py, fp32 on the CPU) describe one algorithm, the closed forms hold exactly in fp64, and the
host half of the C ABI (the workspace size, the declarations) is in place."""
import ctypes
import os
import re

import numpy as np
import pytest

import msssim_exact as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restatement():
    from cbench_basic_amd.benchmark import ms_ssim
    return ms_ssim


def _library():
    from cbench_basic_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_restatement_agrees_with_fp64():
    """dev32 / dev32_terms: the largest distance of the fp32 restatement from fp64 over every case.  The GPU test's bounds are four
    times these; here only the guard that both state one algorithm (a wrong tap, divisor or padding side moves a value by far
    more than 1e-4)."""
    M = _restatement()
    for case in E.CASES:
        r, (rvalue, rterms) = E.reference(case), E.restatement(case, M)
        print(f"{E.case_id(case)}: value dev {np.abs(rvalue - r['value']).max():.3e}  terms dev {np.abs(rterms - r['terms']).max():.3e}")
    dev32, dev32_terms = E.restatement_deviation(M)
    print(f"dev32 {dev32:.3e}  dev32_terms {dev32_terms:.3e}")
    assert dev32 < 1e-4


@pytest.mark.parametrize("shape", E.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("base", E.BASES)
def test_closed_forms(shape, base):
    """y = x gives exactly 1 and y = 1 - x exactly 0 in fp64; the restatement gives 0.0 for 1 - x too, so the clamp case is real."""
    M = _restatement()
    same, inverse = E.reference((shape, base, "same")), E.reference((shape, base, "inverse"))
    assert (same["value"] == 1.0).all() and (same["terms"] == 1.0).all()
    assert (inverse["value"] == 0.0).all()
    assert (inverse["terms"][..., :4] == 0.0).any()   # a clamped contrast term is what makes it 0
    assert (E.restatement((shape, base, "inverse"), M)[0] == 0.0).all()


def test_pooling_rule():
    """The helper's pooling against torch's avg_pool2d(kernel_size=2, padding=side % 2) in fp64, on odd and even sides."""
    import torch
    import torch.nn.functional as F
    a = torch.rand(2, 1, 7, 10, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    for h, w in ((7, 10), (6, 9), (7, 9), (6, 10), (1, 1)):
        t = a[..., :h, :w]
        want = F.avg_pool2d(t, kernel_size=2, padding=[h % 2, w % 2]).numpy()
        got = E._pool(t.numpy())
        assert got.shape == want.shape == (2, 1, h // 2 + h % 2, w // 2 + w % 2)
        assert np.array_equal(got, want)


def test_workspace_bytes():
    L = _library()
    f = L.basic_msssim_workspace_bytes
    base = (2, 3, 161, 161)
    assert f(*base) > 0
    for shape in E.SHAPES + [(24, 3, 512, 768)]:
        assert f(*shape) > 0
    for arg in range(4):   # does not decrease in any argument: every step over four tiles' worth, then some large ones
        sizes = [f(*[v + k if i == arg else v for i, v in enumerate(base)]) for k in list(range(140)) + [500, 4000]]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        assert sizes[-1] > sizes[0]
    for bad in ((2, 3, 160, 300), (2, 3, 300, 160), (2, 3, 10, 10), (0, 3, 200, 200), (2, 0, 200, 200), (2, 3, -5, 200)):
        assert f(*bad) == -1
    assert f(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == -1   # no overflow into a plausible size


def test_cabi_declares_msssim():
    from cbench_basic_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "basic_hip.h")).read()
    declared = set(re.findall(r"\b(basic_[a-z0-9_]+)\s*\(", hdr))
    for name in ("basic_msssim_workspace_bytes", "basic_msssim_per_image_dev"):
        assert name in declared and name in _lib._SIGNATURES
    assert _lib._SIGNATURES["basic_msssim_workspace_bytes"][0] is ctypes.c_int64
    assert len(_lib._SIGNATURES["basic_msssim_per_image_dev"][1]) == 12
    L = _library()
    assert hasattr(L, "basic_msssim_workspace_bytes") and hasattr(L, "basic_msssim_per_image_dev")


def test_argument_checks_need_no_device():
    """A refused call returns before any launch, so the refusals can be seen without a GPU."""
    from cbench_basic_amd import _lib
    L = _library()
    need = L.basic_msssim_workspace_bytes(1, 1, 161, 161)
    ws = ctypes.create_string_buffer(16)   # never dereferenced: every call below is refused
    p = ctypes.addressof(ws)
    for args in ((p, p, 1, 1, 160, 161, 1.0, p, need, p, None, None),        # a side of 160
                 (p, p, 1, 1, 161, 161, 1.0, p, need, None, None, None),     # null output
                 (p, p, 1, 1, 161, 161, 1.0, p, need - 1, p, None, None)):   # one byte short
        with pytest.raises(_lib.BasicHipError) as e:
            _lib.check(L.basic_msssim_per_image_dev(*args))
        assert "msssim" in str(e.value)
