"""8-bit images without a GPU: the C ABI of the uint8 path (include/basic_hip.h section 8b) is declared, prototyped and exported; the
layout of a tensor is read from its shape and strides; the datasets yield uint8 on request and what they yielded before otherwise."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("basic_image_u8_to_f32_dev", "basic_image_f32_to_u8_dev", "basic_hp_encode_images_u8", "basic_hp_decode_images_u8")


def _header():
    return open(os.path.join(ROOT, "include", "basic_hip.h")).read()


def test_cabi_declares_prototypes_and_exports_the_image_entries():
    from cbench_basic_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    declared = set(re.findall(r"\b(basic_[a-z0-9_]+)\s*\(", _header()))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _lib._SIGNATURES, name
        assert hasattr(lib, name), name
    sig = _lib._SIGNATURES
    assert len(sig["basic_image_u8_to_f32_dev"][1]) == 8 and len(sig["basic_image_f32_to_u8_dev"][1]) == 8
    # the uint8 entries of the session: the float entries' arguments plus the layout (and, decoding, where xhat lives)
    assert len(sig["basic_hp_encode_images_u8"][1]) == len(sig["basic_hp_encode_images"][1]) + 1
    assert len(sig["basic_hp_decode_images_u8"][1]) == len(sig["basic_hp_decode_images"][1]) + 2
    assert all(sig[n][0] is ctypes.c_int for n in NEW)
    _lib.lib()


def test_layout_constants_agree_with_the_header():
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    defines = dict(re.findall(r"#define (BASIC_IMAGE_[A-Z]+) (\d+)", _header()))
    assert defines == {"BASIC_IMAGE_CHW": "0", "BASIC_IMAGE_HWC": "1"}
    assert _lib.IMAGE_CHW == int(defines["BASIC_IMAGE_CHW"]) and _lib.IMAGE_HWC == int(defines["BASIC_IMAGE_HWC"])
    assert K.IMAGE_LAYOUTS == {"chw": _lib.IMAGE_CHW, "hwc": _lib.IMAGE_HWC}


def test_bad_arguments_are_refused_before_a_device_is_needed():
    """The argument checks come first: BASIC_ERR_INVALID with a message, with or without a GPU (nothing can have been launched)."""
    from cbench_basic_amd import _lib
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    for bad in ((p, 0, 0, 3, 4, 4, p), (p, 0, 1, 0, 4, 4, p), (p, 0, 1, 3, -1, 4, p), (p, 0, 1, 3, 4, 0, p), (p, 2, 1, 3, 4, 4, p),
                (p, -1, 1, 3, 4, 4, p), (None, 0, 1, 3, 4, 4, p), (p, 0, 1, 3, 4, 4, None), (p, 0, 1, 3, 4, 4, p + 2),
                (p, 0, 1 << 20, 1 << 10, 1 << 10, 1 << 10, p)):
        assert L.basic_image_u8_to_f32_dev(*bad, None) == _lib.ERR_INVALID, bad
        assert "image_u8_to_f32" in _lib.last_error()
    for bad in ((p, 0, 3, 4, 4, 0, p), (p, 1, 3, 4, 4, 7, p), (None, 1, 3, 4, 4, 0, p), (p, 1, 3, 4, 4, 0, None), (p + 1, 1, 3, 4, 4, 0, p)):
        assert L.basic_image_f32_to_u8_dev(*bad, None) == _lib.ERR_INVALID, bad
        assert "image_f32_to_u8" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(L.basic_image_u8_to_f32_dev(p, 5, 1, 3, 4, 4, p, None))


def test_image_layout_of():
    from cbench_basic_amd.nn.kernels import image_layout_of
    x = torch.zeros(2, 3, 5, 7, dtype=torch.uint8)
    assert image_layout_of(x) == "chw"
    assert image_layout_of(x.float()) == "chw"                                   # shape and strides only
    assert image_layout_of(x.contiguous(memory_format=torch.channels_last)) == "hwc"
    a = np.zeros((5, 7, 3), np.uint8)                                            # what an image decoder delivers
    v = torch.from_numpy(a).permute(2, 0, 1)[None]
    assert image_layout_of(v) == "hwc" and v.data_ptr() == a.ctypes.data         # no copy on the way
    assert image_layout_of(torch.from_numpy(np.zeros((4, 5, 7, 3), np.uint8)).permute(0, 3, 1, 2)) == "hwc"
    assert image_layout_of(x[:, :, :, ::2]) is None                              # strided
    assert image_layout_of(x[:, :, 1:4, :]) is None                              # rows cut out of every plane
    assert image_layout_of(x[:, :2]) is None                                     # channels cut out
    assert image_layout_of(x[1:]) == "chw"                                       # a batch slice stays dense
    assert image_layout_of(x.permute(0, 1, 3, 2)) is None
    assert image_layout_of(x[0]) is None                                         # not [B, C, H, W]
    # one channel: both readings coincide
    g = torch.zeros(2, 1, 5, 7, dtype=torch.uint8)
    assert image_layout_of(g) == "chw"
    assert image_layout_of(g.contiguous(memory_format=torch.channels_last)) == "chw"
    assert image_layout_of(torch.from_numpy(np.zeros((5, 7, 1), np.uint8)).permute(2, 0, 1)[None]) == "chw"


def test_synthetic_uint8_images_are_deterministic_and_distinct():
    from cbench_basic_amd.data import RandomImageDataset
    ds = RandomImageDataset(num=3, size=(3, 16, 20), dtype=torch.uint8)
    a, b, again = ds[0], ds[1], ds[0]
    assert a.dtype == torch.uint8 and tuple(a.shape) == (3, 16, 20)
    assert torch.equal(a, again) and not torch.equal(a, b)
    torch.manual_seed(1)
    assert torch.equal(b, torch.randint(0, 256, (3, 16, 20), dtype=torch.uint8))
    assert int(a.max()) > 200 and int(a.min()) < 50                              # the whole byte range
    with pytest.raises(IndexError):
        ds[3]
    with pytest.raises(TypeError):
        RandomImageDataset(dtype=torch.float64)


def test_float_datasets_return_what_they_returned():
    from cbench_basic_amd.data import RandomImageDataset, batched
    ds = RandomImageDataset(num=3, size=(3, 8, 12))
    torch.manual_seed(2)
    want = torch.rand(3, 8, 12)
    assert ds[2].dtype == torch.float32 and torch.equal(ds[2], want)
    got = list(batched(ds, 2))
    assert [tuple(g.shape) for g in got] == [(2, 3, 8, 12), (1, 3, 8, 12)] and torch.equal(got[1][0], want)
    assert all(g.is_contiguous() for g in got)


def test_image_folder_float_and_uint8(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from cbench_basic_amd.data import ImageFolderDataset, batched
    from cbench_basic_amd.nn.kernels import image_layout_of
    rng = np.random.default_rng(0)
    arrays = [rng.integers(0, 256, (6, 9, 3), dtype=np.uint8) for _ in range(3)]
    for i, a in enumerate(arrays):
        Image.fromarray(a).save(str(tmp_path / f"{i}.png"))
    f32, u8 = ImageFolderDataset(str(tmp_path)), ImageFolderDataset(str(tmp_path), dtype=torch.uint8)
    for i, a in enumerate(arrays):
        want = torch.from_numpy(a).permute(2, 0, 1).contiguous().float().div_(255.0)   # the float ingest, as it was
        assert f32[i].dtype == torch.float32 and f32[i].is_contiguous() and torch.equal(f32[i], want)
        x = u8[i]
        assert x.dtype == torch.uint8 and tuple(x.shape) == (3, 6, 9) and torch.equal(x, torch.from_numpy(a).permute(2, 0, 1))
        assert x.stride() == (1, 27, 3)                                          # the decoder's array, not a copy of it
        assert torch.equal(x.float().div(255), want)
    one = list(batched(u8, 1))
    assert len(one) == 3 and all(image_layout_of(b) == "hwc" and tuple(b.shape) == (1, 3, 6, 9) for b in one)
    two = list(batched(u8, 2))
    assert [tuple(b.shape) for b in two] == [(2, 3, 6, 9), (1, 3, 6, 9)] and image_layout_of(two[0]) == "hwc"
    assert torch.equal(two[0][1], u8[1])
