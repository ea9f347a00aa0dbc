"""Every rANS and tANS launch path against the oracle's bytes, with the kernel that ran asserted.

    path                                 selector (launch_encode / launch_decode / launch_tans)      cases (tests/rans_cases.py)
    rans_encode_fast_kernel<W>           fast_enc_ok: <= 2048 rows, every frequency in 1 .. 2^p,     extreme16*, lowp7 .. lowp15, row_widths_no2,
      W = 1, 2, 4, 8, 16                 precision >= 7; W from basic_rans_set_waves                 image_too_big, global_tables, rows2048, resume_*
    rans_encode_kernel                   !fast_enc_ok                                                lowp1 .. lowp6, row_widths, row_widths_4097,
                                                                                                     rows2049, zero_width
    rans_encode_kernel, AR remap         host entry point, table with an AR remap                    global_tables_ar, small_ar
    rans_decode_fast_kernel<W>           no AR, rows <= 4096 entries, search image <= 156 KB,        extreme16*, lowp7 .. lowp15, row_widths, row_widths_no2,
                                         precision >= 7                                              rows2048, rows2049, zero_width, resume_fast
    rans_decode_kernel<false, true>      otherwise, packed rows <= 144 KiB (copied to the LDS)       lowp1 .. lowp6, row_widths_4097, image_too_big, resume_lds
    rans_decode_kernel<false, false>     packed rows over 144 KiB                                    global_tables, resume_global
    rans_decode_kernel<true, true>       AR remap, packed rows <= 144 KiB                            small_ar
    rans_decode_kernel<true, false>      AR remap, packed rows over 144 KiB                          global_tables_ar
    tans_encode_kernel<true / false>     (rows + bypass) * 2^L * 2 bytes <= 144 KiB / over           L12 x 8, 9, 17 / L12 x 18
    tans_decode_kernel<true / false>     (rows + bypass) * 2^L * 4 bytes <= 144 KiB / over           L12 x 8, L9 x 5 / L12 x 9, 17, 18

Every comparison is exact (bytes, integers).  What the kernels may write -- slots, word counts, symbols, state, position -- and
what they read are views into buffers whose bands (and whose untouched elements) hold a NaN payload and must come back bit for
bit.  tests/test_cpu_rans_cases.py proves on the CPU that the cases name every kernel of both enums and sit on them.

Precisions below 7 go to the general kernels since these tests: both fast kernels feed a high word (of x / freq in the encoder,
of x >> p in the decoder) that is below 2^(31-p) to a 24-bit multiply.  Measured on the MI355X with the fast kernels still taking
them (19 streams, W = 1 and 8 alike): encoder p = 1, 2, 4: 13 streams differ from the oracle, p = 6: 10, the first of them stream 3
(63 symbols) from its word 0 on; decoder p = 1, 2, 4: 13 streams wrong, p = 6: 10, first wrong symbol 25 / 12 / 22 / 30 of stream
3; p = 7, 8, 11, 15: none, either way.
"""
import ctypes
import functools
import threading

import numpy as np
import pytest
import torch

import rans_cases as rc
import tans_cases

pytestmark = pytest.mark.gpu

GUARD = 0x7FC0BEEF          # NaN payload of the guard bands
GUARD64 = (GUARD << 32) | GUARD
BAND = 256                  # elements of guard band on each side of a view
BATCHED = rc.names(lambda c: c.ar is None)
AR = rc.names(lambda c: c.ar is not None)


def _kernel(name):
    from cbench_basic_amd.nn import kernels
    return getattr(kernels, "RANS_KERNEL_" + name)


class Guarded:
    """A device view of n elements, BAND elements into a buffer filled with the guard pattern."""

    def __init__(self, n, dtype, data=None):
        self.n, self.fill = n, GUARD if dtype == torch.int32 else GUARD64
        self.buf = torch.full((2 * BAND + n,), self.fill, dtype=dtype, device="cuda")
        self.view = self.buf[BAND: BAND + n]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)).view(dtype))

    def ptr(self):
        return self.view.data_ptr()

    def host(self):
        """The view on the host, after checking both bands."""
        b = self.buf.cpu().numpy()
        assert (b[:BAND] == self.fill).all() and (b[BAND + self.n:] == self.fill).all(), "guard band overwritten"
        return b[BAND: BAND + self.n]


@functools.lru_cache(maxsize=4)
def _tables(name):
    from cbench_basic_amd.nn.kernels import RansTables
    c = rc.case(name)
    return RansTables(cdfs=c.cdfs, cdf_sizes=c.sizes, offsets=c.offsets, precision=c.precision, bypass=c.bypass,
                      bypass_precision=c.bypass_precision)


def _batches(c, w):
    n = len(c.streams)
    longest = int(np.argmax([idx.size for _, idx in c.streams]))
    return [list(range(n)), [longest], list(range(n - min(w, n), n))]      # all (ragged), one stream, exactly W


def _concat(c, sel):
    sym = np.concatenate([c.streams[i][0] for i in sel] + [np.zeros(0, np.int32)])
    idx = np.concatenate([c.streams[i][1] for i in sel] + [np.zeros(0, np.int32)])
    seg = np.concatenate([[0], np.cumsum([c.streams[i][1].size for i in sel])]).astype(np.int64)
    return sym, idx, seg


def _first_difference(got, want):
    n = min(got.size, want.size)
    d = np.flatnonzero(got[:n] != want[:n])
    return f"{got.size} words against the oracle's {want.size}, first differing word {int(d[0]) if d.size else n}"


def _encode(c, sel, slot):
    """-> (slot words [len(sel)][slot] with the guard pattern where nothing was written, nwords)."""
    from cbench_basic_amd import _lib
    sym, idx, seg = _concat(c, sel)
    g_sym, g_idx = Guarded(max(sym.size, 1), torch.int32, sym if sym.size else None), Guarded(max(idx.size, 1), torch.int32, idx if idx.size else None)
    g_seg = Guarded(seg.size, torch.int64, seg)
    g_slots, g_nw = Guarded(len(sel) * slot, torch.int32), Guarded(len(sel), torch.int32)
    _lib.check(_lib.lib().basic_rans_encode_batch_dev(_tables(c.name)._h, g_sym.ptr(), g_idx.ptr(), g_seg.ptr(), len(sel), g_slots.ptr(), slot,
                                                      g_nw.ptr(), None))
    torch.cuda.synchronize()
    for g, a in ((g_sym, sym), (g_idx, idx), (g_seg, seg)):
        assert np.array_equal(g.host()[: a.size], a.view(g.host().dtype))
    return g_slots.host().view(np.uint32).reshape(len(sel), slot), g_nw.host()


def _check_streams(c, sel, slots, nwords, want, slot):
    for k, i in enumerate(sel):
        if want[i].size > slot:
            assert nwords[k] == -1, (c.name, i)
            continue
        assert nwords[k] == want[i].size, (c.name, f"stream {i}", int(nwords[k]), want[i].size)
        got = slots[k, slot - nwords[k]:]
        assert np.array_equal(got, want[i]), (c.name, f"stream {i} of {c.streams[i][1].size} symbols", _first_difference(got, want[i]))
        assert (slots[k, : slot - nwords[k]] == GUARD).all(), (c.name, i, "words below the stream were written")


@pytest.mark.parametrize("w", rc.WAVES)
@pytest.mark.parametrize("name", BATCHED)
def test_encode_bytes_equal_the_oracle(oracle, name, w):
    """basic_rans_encode_batch_dev at W streams per workgroup: every stream's words and word count are the oracle's, the launch
    is the case's kernel at W (1 for the one-wave kernel), nothing outside the streams is written."""
    from cbench_basic_amd.nn.kernels import RansTables, rans_waves
    c, want = rc.case(name), rc.oracle_streams(name)
    slot = max(s.size for s in want) + 5
    with rans_waves(w):
        for sel in _batches(c, w):
            slots, nwords = _encode(c, sel, slot)
            assert RansTables.last_launch() == (_kernel(c.enc), w if c.enc == "ENC_FAST" else 1), (name, rc.predict(c))
            _check_streams(c, sel, slots, nwords, want, slot)


@pytest.mark.parametrize("w", rc.WAVES)
@pytest.mark.parametrize("name", rc.names(lambda c: c.ar is None and len(c.streams) == rc.BATCH))
def test_slot_one_word_short(oracle, name, w):
    """A slot one word too small for the longest stream of the batch: -1 for that stream only, the others' words unchanged,
    the bands intact (checked by Guarded.host)."""
    from cbench_basic_amd.nn.kernels import rans_waves
    c, want = rc.case(name), rc.oracle_streams(name)
    sizes = sorted(s.size for s in want)
    assert sizes[-1] > sizes[-2]
    slot = sizes[-1] - 1
    with rans_waves(w):
        slots, nwords = _encode(c, list(range(len(want))), slot)
    assert (nwords == -1).sum() == 1
    _check_streams(c, list(range(len(want))), slots, nwords, want, slot)


@pytest.mark.parametrize("w", rc.WAVES)
@pytest.mark.parametrize("name", BATCHED)
def test_decode_symbols_state_and_position(oracle, name, w):
    """basic_rans_decode_batch_dev on the oracle's words: the symbols are the input, every stream ends at state 2^31 with all of
    its words read (what the oracle does: tests/test_cpu_rans_cases.py), the launch is the case's kernel."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn.kernels import RansTables, rans_waves
    c, want = rc.case(name), rc.oracle_streams(name)
    with rans_waves(w):
        for sel in _batches(c, w):
            sym, idx, seg = _concat(c, sel)
            words = np.concatenate([want[i] for i in sel])
            woff = np.concatenate([[0], np.cumsum([want[i].size for i in sel])]).astype(np.int64)
            g_words, g_woff = Guarded(words.size, torch.int32, words.view(np.int32)), Guarded(woff.size, torch.int64, woff)
            g_idx, g_seg = Guarded(max(idx.size, 1), torch.int32, idx if idx.size else None), Guarded(seg.size, torch.int64, seg)
            g_out, g_state = Guarded(max(sym.size, 1), torch.int32), Guarded(len(sel), torch.int64, np.zeros(len(sel), np.int64))
            g_pos = Guarded(len(sel), torch.int64, np.full(len(sel), -1, np.int64))
            _lib.check(_lib.lib().basic_rans_decode_batch_dev(_tables(name)._h, g_words.ptr(), g_woff.ptr(), g_idx.ptr(), g_seg.ptr(), len(sel),
                                                              g_out.ptr(), g_state.ptr(), g_pos.ptr(), None))
            torch.cuda.synchronize()
            assert RansTables.last_launch() == (_kernel(c.dec), w if c.dec == "DEC_FAST" else 1), (name, rc.predict(c))
            out = g_out.host()
            assert np.array_equal(out[: sym.size], sym), (name, len(sel), int(np.flatnonzero(out[: sym.size] != sym)[0]))
            assert (out[sym.size:] == GUARD).all()
            assert (g_state.host() == 1 << 31).all() and np.array_equal(g_pos.host(), np.diff(woff))
            assert np.array_equal(g_words.host(), words.view(np.int32)) and np.array_equal(g_idx.host()[: idx.size], idx)


@pytest.mark.parametrize("name", AR)
def test_ar_remap_through_the_host_entry_points(oracle, name):
    """Tables with an order-1 AR remap exist behind the host drop-in only: every stream's bytes equal the oracle's, decode gives
    the symbols, and the launches are the general encoder with AR and the AR decoder with packed rows in the LDS / in global memory."""
    from cbench_basic_amd import ans
    from cbench_basic_amd.nn.kernels import rans_last_launch
    c, want = rc.case(name), rc.oracle_streams(name)
    enc, dec = ans.Rans64Encoder(c.precision, c.bypass, 4), ans.Rans64Decoder(c.precision, c.bypass, 4)
    for o in (enc, dec):
        o.init_cdf_params(c.cdfs, c.sizes, c.offsets)
        o.init_ar_params(*c.ar)
    for i, (sym, idx) in enumerate(c.streams):
        kw = dict(ar_indexes=np.zeros_like(idx), ar_offsets=c.ar_offsets(idx.size))
        got = np.frombuffer(enc.encode_with_indexes(sym, idx, **kw), np.uint32)
        assert rans_last_launch() == (_kernel(c.enc), 1)
        assert np.array_equal(got, want[i]), (name, i, _first_difference(got, want[i]))
        assert np.array_equal(dec.decode_with_indexes(want[i].tobytes(), idx, **kw), sym), (name, i)
        if idx.size:
            assert rans_last_launch() == (_kernel(c.dec), 1)


def test_host_entry_points_record_their_launch(oracle):
    """The host encoder always launches one wave per workgroup; the host decoder goes through the batched launch and takes W."""
    from cbench_basic_amd import ans
    from cbench_basic_amd.nn.kernels import rans_last_launch, rans_waves
    for name in ("lowp8", "zero_width", "row_widths_4097"):
        c, want = rc.case(name), rc.oracle_streams(name)
        enc, dec = ans.Rans64Encoder(c.precision, c.bypass, 4), ans.Rans64Decoder(c.precision, c.bypass, 4)
        enc.init_cdf_params(c.cdfs, c.sizes, c.offsets)
        dec.init_cdf_params(c.cdfs, c.sizes, c.offsets)
        sym, idx = c.streams[9]
        with rans_waves(8):
            assert enc.encode_with_indexes(sym, idx) == want[9].tobytes()
            assert rans_last_launch() == (_kernel(c.enc), 1)
            assert np.array_equal(dec.decode_with_indexes(want[9].tobytes(), idx), sym)
            assert rans_last_launch() == (_kernel(c.dec), 8 if c.dec == "DEC_FAST" else 1)


def test_set_waves_and_the_launch_record():
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn.kernels import RANS_KERNEL_NONE, rans_last_launch, rans_waves
    L = _lib.lib()
    prev = ctypes.c_int(-7)
    _lib.check(L.basic_rans_set_waves(4, ctypes.byref(prev)))
    before = prev.value
    with rans_waves(16):
        with rans_waves(0):
            _lib.check(L.basic_rans_set_waves(2, ctypes.byref(prev)))
            assert prev.value == 0
        _lib.check(L.basic_rans_set_waves(16, ctypes.byref(prev)))
        assert prev.value == 16          # the inner block put back what it found
    _lib.check(L.basic_rans_set_waves(before, ctypes.byref(prev)))
    assert prev.value == 4
    for bad in (-1, 3, 5, 32):
        with pytest.raises(ValueError):
            _lib.check(L.basic_rans_set_waves(bad, None))
    seen = []
    t = threading.Thread(target=lambda: seen.append(rans_last_launch()))     # the record is per thread
    t.start()
    t.join()
    assert seen == [(RANS_KERNEL_NONE, 0)]


# ---------------------------------------------------------------------------------------------------------------------------
# resumed decoding
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _resume_reference(name):
    c, want = rc.case(name), rc.oracle_streams(name)
    return [rc.oracle_decode_pieces(c, want[s], c.streams[s][1], rc.RESUME_PIECES) for s in range(len(c.streams))]


@pytest.mark.parametrize("entry", ["streams", "lanes1", "strided"])
@pytest.mark.parametrize("name,w", [("resume_fast", 1), ("resume_fast", 4), ("resume_lds", 1), ("resume_global", 1)])
def test_resumed_decode(oracle, name, w, entry):
    """5 images x 3 lanes of 257 bypass-heavy symbols decoded in pieces of 1, 63, 64, 65 and 64 symbols (two streams of three
    resume directly behind an escape code): after EVERY piece the symbols so far, d_state and d_pos equal the oracle's
    set_stream / decode_stream over the same pieces.  Both sides use -1 for a fresh stream and otherwise the index of the next
    unread word (decode_impl of oracle/rans64_oracle.c: *pos = p - words), so the comparison is plain equality.
      streams : basic_rans_decode_batch_streams_dev, lanes 3, stream_first 2, stream_stride 4 -- the entries of word_off / state
                / pos in between belong to no stream of the launch and must keep their pattern;
      lanes1  : basic_rans_decode_batch_lanes_dev at lanes == 1 (15 streams);   strided : basic_rans_decode_batch_strided_dev."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn.kernels import RansTables, rans_waves
    c, want, ref = rc.case(name), rc.oracle_streams(name), _resume_reference(name)
    T = _tables(name)
    B, K, n = rc.RESUME_IMAGES, rc.RESUME_LANES, rc.RESUME_LEN
    first0 = 7
    if entry == "streams":
        lanes, nimg, sfirst, sstride, stride = K, B, 2, K + 1, K * n + 11
    else:
        lanes, nimg, sfirst, sstride, stride = 1, B * K, 0, 1, n + 3
    sid = [sfirst + (s // lanes) * sstride + s % lanes for s in range(B * K)]
    nslots = sfirst + nimg * sstride
    total = first0 + nimg * stride + 5

    def start(s, done, count):      # first element of stream s' piece that begins `done` symbols into the stream
        return first0 + lanes * done + (s // lanes) * stride + (s % lanes) * count

    idx = np.zeros(total, np.int32)
    woff = np.zeros(nslots + 1, np.int64)
    for s in range(B * K):
        woff[sid[s] + 1] = want[s].size
    woff = np.cumsum(woff)
    words = np.concatenate([want[s] for s in range(B * K)])       # sid ascends with s; the slots between hold no words
    pos0, state0 = np.full(nslots, GUARD64, np.int64), np.full(nslots, GUARD64, np.int64)
    pos0[sid] = -1
    g_words, g_woff = Guarded(words.size, torch.int32, words.view(np.int32)), Guarded(woff.size, torch.int64, woff)
    g_out, g_state, g_pos = Guarded(total, torch.int32), Guarded(nslots, torch.int64, state0), Guarded(nslots, torch.int64, pos0)
    exp_out, exp_state, exp_pos = np.full(total, GUARD, np.int32), state0.copy(), pos0.copy()
    done = 0
    for j, count in enumerate(rc.RESUME_PIECES):
        for s in range(B * K):
            idx[start(s, done, count): start(s, done, count) + count] = c.streams[s][1][done: done + count]
        done += count
    g_idx = Guarded(total, torch.int32, idx)
    L, h = _lib.lib(), T._h
    done = 0
    with rans_waves(w):
        for j, count in enumerate(rc.RESUME_PIECES):
            first = first0 + lanes * done
            if entry == "streams":
                T.decode_batch_streams(g_words.view, g_woff.view, g_idx.view, first, stride, lanes, count, nimg, sfirst, sstride,
                                       g_out.view, g_state.view, g_pos.view)
            elif entry == "lanes1":
                T.decode_batch_lanes(g_words.view, g_woff.view, g_idx.view, first, stride, 1, count, nimg, g_out.view, g_state.view, g_pos.view)
            else:
                _lib.check(L.basic_rans_decode_batch_strided_dev(h, g_words.ptr(), g_woff.ptr(), g_idx.ptr(), first, stride, count, nimg,
                                                                 g_out.ptr(), g_state.ptr(), g_pos.ptr(), None))
            torch.cuda.synchronize()
            assert RansTables.last_launch() == (_kernel(c.dec), w if c.dec == "DEC_FAST" else 1)
            for s in range(B * K):
                sym, state, pos = ref[s][j]
                assert np.array_equal(sym, c.streams[s][0][done: done + count])
                exp_out[start(s, done, count): start(s, done, count) + count] = sym
                exp_state[sid[s]], exp_pos[sid[s]] = state, pos
            out, state, pos = g_out.host(), g_state.host(), g_pos.host()
            assert np.array_equal(out, exp_out), (name, entry, j, np.flatnonzero(out != exp_out)[:4])
            assert np.array_equal(state.view(np.uint64), exp_state.view(np.uint64)), (name, entry, j, np.flatnonzero(state != exp_state)[:4])
            assert np.array_equal(pos, exp_pos), (name, entry, j, np.flatnonzero(pos != exp_pos)[:4])
            done += count
    assert all(exp_pos[sid[s]] == want[s].size and exp_state[sid[s]] == 1 << 31 for s in range(B * K))
    assert np.array_equal(g_words.host(), words.view(np.int32)) and np.array_equal(g_woff.host(), woff) and np.array_equal(g_idx.host(), idx)


# ---------------------------------------------------------------------------------------------------------------------------
# tANS
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tans_reference(L, nd):
    from oracle import tans_oracle
    return [tans_cases.run_raw(tans_oracle, c) for c in tans_cases.path_case(L, nd)]


@pytest.mark.parametrize("L,nd", tans_cases.PATH_CONFIGS)
def test_tans_batched_paths(L, nd):
    """37 ragged streams (one empty) through basic_tans_encode_batch_dev / basic_tans_decode_batch_dev: EVERY stream's bytes and
    coded-symbol count equal oracle.tans_oracle's raw stream (tans_cases.run_raw: `run` without the reference's output budget,
    which blanks streams the batched entry points do write), the decoded symbols are the input, every status is 0, and the
    launches are the image-in-LDS or image-in-global kernels as the table size says."""
    from cbench_basic_amd import _lib, ans
    cases, ref = tans_cases.path_case(L, nd), _tans_reference(L, nd)
    _, freqs, nsym, off, byp, _, _ = cases[0]
    enc, dec = ans.TansEncoder(L, 255, byp, 4), ans.TansDecoder(L, 255, byp, 4)
    enc.init_params(freqs, nsym, off)
    dec.init_params(freqs, nsym, off)
    S = len(cases)
    sym = np.concatenate([c[5] for c in cases])
    idx = np.concatenate([c[6] for c in cases])
    seg = np.concatenate([[0], np.cumsum([c[6].size for c in cases])]).astype(np.int64)
    lib = _lib.lib()
    slot = int(lib.basic_tans_encode_bound_words(enc._tables, int(np.diff(seg).max())))
    g_sym, g_idx, g_seg = Guarded(sym.size, torch.int32, sym), Guarded(idx.size, torch.int32, idx), Guarded(seg.size, torch.int64, seg)
    g_words, g_info = Guarded(S * slot, torch.int32), Guarded(2 * S, torch.int64)
    _lib.check(lib.basic_tans_encode_batch_dev(enc._tables, g_sym.ptr(), g_idx.ptr(), g_seg.ptr(), S, g_words.ptr(), slot, g_info.ptr(), None))
    torch.cuda.synchronize()
    want_enc, want_dec = tans_cases.path_kernels(L, nd)
    assert ans.tans_last_launch() == getattr(ans, "TANS_KERNEL_" + want_enc)
    info = g_info.host().reshape(S, 2)
    host = g_words.host().view(np.uint8).reshape(S, slot * 4)
    for i, (data, coded, back) in enumerate(ref):
        assert info[i, 0] > 0 and host[i, : (info[i, 0] + 7) // 8].tobytes() == data, (L, nd, i, int(info[i, 0]), 8 * len(data))
        assert info[i, 1] == coded, (L, nd, i)
    blob = np.frombuffer(b"".join(r[0] for r in ref), np.uint8)
    boff = np.concatenate([[0], np.cumsum([len(r[0]) for r in ref])]).astype(np.int64)
    g_blob = torch.from_numpy(blob.copy()).cuda()
    g_boff = Guarded(boff.size, torch.int64, boff)
    g_out, g_status = Guarded(sym.size, torch.int32), Guarded(S, torch.int32)
    _lib.check(lib.basic_tans_decode_batch_dev(dec._tables, g_blob.data_ptr(), g_boff.ptr(), g_idx.ptr(), g_seg.ptr(), S, g_out.ptr(),
                                               g_status.ptr(), None))
    torch.cuda.synchronize()
    assert ans.TansDecoder.last_launch() == getattr(ans, "TANS_KERNEL_" + want_dec)
    assert (g_status.host() == 0).all()
    assert np.array_equal(g_out.host(), sym)
