"""The skip-coding kernels of csrc/entropy.hip on the GPU (INTEGRATION.md "Skip coding"): basic_skip_compact_dev and
basic_skip_expand_dev equal the NumPy restatement (tests/skip_exact.py) exactly -- symbols, indexes and every entry of d_seg.  The
entry points are called through ctypes on sentinel-filled outputs, so a store past the kept total shows too.

Shapes: per in {1, 63, 64, 65, C - 1, C, C + 1, 2 C + 37} (C = BASIC_SKIP_CHUNK: below a wave, on and around a wave of lanes, on and
around a chunk, three chunks with a ragged tail; per % 4 != 0 puts every stream but the first off the 16-byte path) crossed with
1 and 5 streams.  The largest case is 5 x (2 C + 37) int32."""
import ctypes

import numpy as np
import pytest
import torch

import skip_exact as SX

pytestmark = pytest.mark.gpu

C = 1024          # BASIC_SKIP_CHUNK
R = 12            # skip_rows of the pattern tests
SENTINEL = -77
PERS = [1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 37]
PATTERNS = ["all", "none", "first", "last", "straddle", "rand0.03", "rand0.5", "rand0.97", "empty_between"]
ERR_INVALID = -1


@pytest.fixture(scope="module")
def K():
    from cbench_basic_amd.nn import kernels
    assert kernels.SKIP_CHUNK == C
    return kernels


def _keep(pattern, ns, per, rng):
    keep = np.zeros((ns, per), dtype=bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "first":
        keep[:, 0] = True
    elif pattern == "last":
        keep[:, -1] = True
    elif pattern == "straddle":
        # kept runs across a lane's four elements, a wave's 256, and a chunk's C -- wherever the stream is long enough
        for edge in (4, 256, C, 2 * C):
            keep[:, max(0, min(edge, per) - 3):min(per, edge + 3)] = True
    elif pattern.startswith("rand"):
        keep = rng.random((ns, per)) < float(pattern[4:])
    elif pattern == "empty_between":
        keep[0::2] = True   # streams 0, 2, 4 full, 1 and 3 empty
    return keep


def _arrays(keep, rng, r=R):
    """Indexes whose rows say ``keep`` under skip_rows = r, over the whole table; symbols of both signs, never the sentinel or 0."""
    idx = np.where(keep, rng.integers(r, 64, keep.shape), rng.integers(0, r, keep.shape)).astype(np.int32)
    sym = rng.integers(1, 1000, keep.shape).astype(np.int32) * np.where(rng.random(keep.shape) < 0.5, -1, 1).astype(np.int32)
    sym[sym == SENTINEL] = 5
    return sym, idx


def _lib():
    from cbench_basic_amd import _lib
    return _lib.lib()


def _scratch(K, ns, per):
    return torch.empty((max(K.skip_scratch_bytes(ns, per) // 8, 1),), device="cuda", dtype=torch.int64)


def _compact(K, sym, idx, ns, r, with_sym=True):
    """basic_skip_compact_dev on sentinel-filled outputs -> (rc, sym_out or None, idx_out, seg) as numpy."""
    per = idx.size // ns
    d_idx = torch.from_numpy(np.ascontiguousarray(idx)).cuda()
    d_sym = torch.from_numpy(np.ascontiguousarray(sym)).cuda() if with_sym else None
    so = torch.full((idx.size,), SENTINEL, device="cuda", dtype=torch.int32) if with_sym else None
    io = torch.full((idx.size,), SENTINEL, device="cuda", dtype=torch.int32)
    seg = torch.full((ns + 1,), SENTINEL, device="cuda", dtype=torch.int64)
    scratch = _scratch(K, ns, per)
    rc = _lib().basic_skip_compact_dev(d_sym.data_ptr() if with_sym else None, d_idx.data_ptr(), ns, per, r, scratch.data_ptr(),
                                       so.data_ptr() if with_sym else None, io.data_ptr(), seg.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, (so.cpu().numpy() if with_sym else None), io.cpu().numpy(), seg.cpu().numpy()


def _expand(K, sym_c, idx, ns, r):
    per = idx.size // ns
    d_idx = torch.from_numpy(np.ascontiguousarray(idx)).cuda()
    d_c = torch.from_numpy(np.ascontiguousarray(sym_c)).cuda()
    out = torch.full((idx.size,), SENTINEL, device="cuda", dtype=torch.int32)
    scratch = _scratch(K, ns, per)
    rc = _lib().basic_skip_expand_dev(d_c.data_ptr(), d_idx.data_ptr(), ns, per, r, scratch.data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().reshape(ns, per)


def _check_compact(K, sym, idx, ns, r, what):
    ref_s, ref_i, ref_seg = SX.compact(sym, idx, ns, r)
    total = int(ref_seg[-1])
    rc, so, io, seg = _compact(K, sym, idx, ns, r)
    assert rc == 0, what
    assert seg.dtype == np.int64 and np.array_equal(seg, ref_seg), (what, seg, ref_seg)
    assert np.array_equal(so[:total], ref_s) and np.array_equal(io[:total], ref_i), what
    assert (so[total:] == SENTINEL).all() and (io[total:] == SENTINEL).all(), f"{what}: a store past the {total} kept elements"
    # the decoder's form: indexes and segments only
    rc2, none, io2, seg2 = _compact(K, None, idx, ns, r, with_sym=False)
    assert rc2 == 0 and none is None and np.array_equal(io2, io) and np.array_equal(seg2, seg), what
    # the inverse, from a compact array as long as the input (what lies past the total is never read into the result)
    rc3, dense = _expand(K, so, idx, ns, r)
    assert rc3 == 0 and np.array_equal(dense, SX.expand(ref_s, idx, ns, r)), what
    keep = SX.keep_mask(idx.reshape(ns, -1), r)
    assert np.array_equal(dense[keep], sym.reshape(ns, -1)[keep]) and not dense[~keep].any(), what
    return so, io, seg


@pytest.mark.parametrize("ns", [1, 5])
@pytest.mark.parametrize("per", PERS)
def test_compact_and_expand_equal_the_restatement(K, per, ns):
    rng = np.random.default_rng(1000 * ns + per)
    for pattern in PATTERNS:
        keep = _keep(pattern, ns, per, rng)
        sym, idx = _arrays(keep, rng)
        # the data would catch the likely mistakes: the mask is the pattern, and a non-trivial one is neither full nor empty
        assert np.array_equal(SX.keep_mask(idx, R), keep)
        if pattern == "none":
            assert not keep.any()
        if pattern == "rand0.5" and per >= 63:
            assert 0.2 < keep.mean() < 0.8
        so, io, seg = _check_compact(K, sym, idx, ns, R, f"{pattern} per={per} ns={ns}")
        if pattern == "none":
            assert (seg == 0).all()   # every seg entry equal
        if pattern in ("first", "last"):
            assert seg.tolist() == list(range(ns + 1))
        if pattern == "all":
            assert seg.tolist() == [k * per for k in range(ns + 1)] and np.array_equal(so, sym.reshape(-1))
        if pattern == "empty_between" and ns == 5:
            assert seg.tolist() == [0, per, per, 2 * per, 2 * per, 3 * per]


@pytest.mark.parametrize("ns,per", [(1, 1), (5, 65), (5, C + 1), (5, 2 * C + 37)])
def test_skip_rows_zero_copies_and_large_rows_skip_everything(K, ns, per):
    rng = np.random.default_rng(7)
    sym, idx = _arrays(rng.random((ns, per)) < 0.5, rng)
    so, io, seg = _check_compact(K, sym, idx, ns, 0, "r = 0")
    assert np.array_equal(so, sym.reshape(-1)) and np.array_equal(io, idx.reshape(-1))
    assert seg.tolist() == [k * per for k in range(ns + 1)]
    for r in (64, 2 ** 31 - 1):   # greater than every idx
        assert idx.max() < r
        so, io, seg = _check_compact(K, sym, idx, ns, r, f"r = {r}")
        assert (seg == 0).all() and (so == SENTINEL).all() and (io == SENTINEL).all()
    # the boundary itself: idx == r is kept, idx == r - 1 is not
    idx2 = np.full((ns, per), R, dtype=np.int32)
    idx2[:, ::2] = R - 1
    _, _, seg = _check_compact(K, sym, idx2, ns, R, "idx == r")
    assert seg[-1] == ns * (per // 2)


def test_unaligned_base_pointers(K):
    """The arrays start one element off a 16-byte boundary: every lane takes the element-by-element lines."""
    ns, per = 5, C
    rng = np.random.default_rng(11)
    keep = rng.random((ns, per)) < 0.5
    sym, idx = _arrays(keep, rng)
    n = ns * per
    d_sym = torch.zeros(n + 1, device="cuda", dtype=torch.int32)
    d_idx = torch.zeros(n + 1, device="cuda", dtype=torch.int32)
    d_sym[1:] = torch.from_numpy(sym.reshape(-1)).cuda()
    d_idx[1:] = torch.from_numpy(idx.reshape(-1)).cuda()
    assert d_idx[1:].data_ptr() % 16 == 4
    so = torch.full((n + 1,), SENTINEL, device="cuda", dtype=torch.int32)
    io = torch.full((n + 1,), SENTINEL, device="cuda", dtype=torch.int32)
    dense = torch.full((n + 1,), SENTINEL, device="cuda", dtype=torch.int32)
    seg = torch.zeros(ns + 1, device="cuda", dtype=torch.int64)
    scratch = _scratch(K, ns, per)
    lib = _lib()
    assert lib.basic_skip_compact_dev(d_sym[1:].data_ptr(), d_idx[1:].data_ptr(), ns, per, R, scratch.data_ptr(), so[1:].data_ptr(),
                                      io[1:].data_ptr(), seg.data_ptr(), None) == 0
    assert lib.basic_skip_expand_dev(so[1:].data_ptr(), d_idx[1:].data_ptr(), ns, per, R, scratch.data_ptr(), dense[1:].data_ptr(), None) == 0
    torch.cuda.synchronize()
    ref_s, ref_i, ref_seg = SX.compact(sym, idx, ns, R)
    total = int(ref_seg[-1])
    assert np.array_equal(seg.cpu().numpy(), ref_seg)
    so, io, dense = so.cpu().numpy(), io.cpu().numpy(), dense.cpu().numpy()
    assert so[0] == SENTINEL and io[0] == SENTINEL and dense[0] == SENTINEL
    assert np.array_equal(so[1:1 + total], ref_s) and np.array_equal(io[1:1 + total], ref_i) and (so[1 + total:] == SENTINEL).all()
    assert np.array_equal(dense[1:].reshape(ns, per), SX.expand(ref_s, idx, ns, R))


def test_two_calls_give_identical_output(K):
    ns, per = 5, 2 * C + 37
    rng = np.random.default_rng(3)
    sym, idx = _arrays(rng.random((ns, per)) < 0.5, rng)
    a, b = _compact(K, sym, idx, ns, R), _compact(K, sym, idx, ns, R)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    ea, eb = _expand(K, a[1], idx, ns, R), _expand(K, a[1], idx, ns, R)
    assert ea[0] == 0 and np.array_equal(ea[1], eb[1])


def test_python_front_ends(K):
    ns, per = 5, C + 1
    rng = np.random.default_rng(5)
    sym, idx = _arrays(rng.random((ns, per)) < 0.5, rng)
    ref_s, ref_i, ref_seg = SX.compact(sym, idx, ns, R)
    total = int(ref_seg[-1])
    d_sym, d_idx = torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda()
    sc, ic, seg = K.skip_compact(d_sym, d_idx, ns, R)
    assert sc.dtype == torch.int32 and seg.dtype == torch.int64 and sc.numel() == ns * per
    assert np.array_equal(seg.cpu().numpy(), ref_seg) and np.array_equal(sc.cpu().numpy()[:total], ref_s)
    assert np.array_equal(ic.cpu().numpy()[:total], ref_i)
    none, ic2, seg2 = K.skip_compact(None, d_idx, ns, R)
    assert none is None and torch.equal(ic2[:total], ic[:total]) and torch.equal(seg2, seg)
    dense = K.skip_expand(sc, d_idx, ns, R)
    assert dense.shape == d_idx.shape and np.array_equal(dense.cpu().numpy(), SX.expand(ref_s, idx, ns, R))
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            K.skip_compact(d_sym, d_idx, ns, bad)
    with pytest.raises(ValueError):
        K.skip_compact(d_sym, d_idx, 4, R)   # 5 * (C + 1) elements are no four equal streams
    with pytest.raises(ValueError):
        K.skip_expand(sc, d_idx, 0, R)


def test_argument_errors_launch_nothing(K):
    ns, per = 2, 65
    n = ns * per
    d_sym = torch.ones(n, device="cuda", dtype=torch.int32)
    d_idx = torch.full((n,), 20, device="cuda", dtype=torch.int32)
    so = torch.full((n,), SENTINEL, device="cuda", dtype=torch.int32)
    io = torch.full((n,), SENTINEL, device="cuda", dtype=torch.int32)
    seg = torch.full((ns + 1,), SENTINEL, device="cuda", dtype=torch.int64)
    scratch = torch.full((8,), SENTINEL, device="cuda", dtype=torch.int64)
    lib = _lib()
    S, I, SO, IO, SEG, SCR = (t.data_ptr() for t in (d_sym, d_idx, so, io, seg, scratch))
    bad_compact = [
        (S, None, ns, per, R, SCR, SO, IO, SEG),      # null indexes
        (S, I, ns, per, R, None, SO, IO, SEG),        # null scratch
        (S, I, ns, per, R, SCR, SO, None, SEG),       # null index output
        (S, I, ns, per, R, SCR, SO, IO, None),        # null segments
        (S, I, 0, per, R, SCR, SO, IO, SEG),          # nstreams < 1
        (S, I, -3, per, R, SCR, SO, IO, SEG),
        (S, I, ns, 0, R, SCR, SO, IO, SEG),           # per < 1
        (S, I, ns, -per, R, SCR, SO, IO, SEG),
        (S, I, ns, per, -1, SCR, SO, IO, SEG),        # skip_rows < 0
        (S, I, ns, per, R, SCR, None, IO, SEG),       # d_sym without d_sym_out
        (None, I, ns, per, R, SCR, SO, IO, SEG),      # and the reverse
        (S, I, ns, per, R, SCR + 4, SO, IO, SEG),     # a misaligned scratch
    ]
    for a in bad_compact:
        assert lib.basic_skip_compact_dev(*a, None) == ERR_INVALID, a
    DN = so.data_ptr()
    bad_expand = [
        (None, I, ns, per, R, SCR, DN), (S, None, ns, per, R, SCR, DN), (S, I, ns, per, R, None, DN), (S, I, ns, per, R, SCR, None),
        (S, I, 0, per, R, SCR, DN), (S, I, ns, 0, R, SCR, DN), (S, I, ns, per, -1, SCR, DN),
    ]
    for a in bad_expand:
        assert lib.basic_skip_expand_dev(*a, None) == ERR_INVALID, a
    torch.cuda.synchronize()
    for t in (so, io, seg, scratch):
        assert bool((t == SENTINEL).all()), "a refused call wrote something"
    assert ctypes.c_char_p(lib.basic_last_error()).value   # the refusal left its text
