"""Thin torch-tensor front-ends of the C-ABI compute entry points (include/basic_hip.h).

PyTorch is used here for device memory and streams only; every operation below is a
hand-written HIP kernel.  All functions require CUDA(HIP) tensors and raise otherwise --
there is no CPU implementation behind them.
"""
import contextlib
import ctypes
import os

import numpy as np
import torch

from .. import _lib

ACT_NONE, ACT_RELU, ACT_LEAKY_RELU, ACT_GDN, ACT_IGDN = 0, 1, 2, 3, 4


def _dev(t, dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.BasicHipError("cbench_basic_amd kernels need tensors on the MI355X (got a CPU tensor); "
                                 "there is no CPU fallback")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return t.contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)


class ConvPlan:
    """Packed weights + fused epilogue of one conv / deconv layer (basic_conv_plan_*)."""

    def __init__(self, weight, bias, stride, padding, output_padding=0, transposed=False, act=ACT_NONE,
                 gamma=None, beta=None, cin_active=None, cout_active=None):
        w = _f32(weight)
        self.transposed = bool(transposed)
        cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
        self.cin = cin if cin_active is None else int(cin_active)
        self.cout = cout if cout_active is None else int(cout_active)
        b = _f32(bias) if bias is not None else None
        g = _f32(gamma) if gamma is not None else None
        be = _f32(beta) if beta is not None else None
        if g is not None and g.shape[0] != cout:
            # effective gamma/beta given for the active slice only: embed in a [cout][cout] frame
            gf = np.zeros((cout, cout), np.float32); gf[: g.shape[0], : g.shape[1]] = g
            bf = np.ones((cout,), np.float32); bf[: be.shape[0]] = be
            g, be = gf, bf
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().basic_conv_plan_create(
            w.ctypes.data, b.ctypes.data if b is not None else None, cin, cout, w.shape[2], int(stride), int(padding),
            int(output_padding), int(self.transposed), int(act), g.ctypes.data if g is not None else None,
            be.ctypes.data if be is not None else None, self.cin, self.cout, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().basic_conv_plan_destroy(h)
            except Exception:
                pass

    def out_hw(self, h, w):
        oh, ow = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.lib().basic_conv_plan_out_hw(self._h, int(h), int(w), ctypes.byref(oh), ctypes.byref(ow)))
        return oh.value, ow.value

    def flops(self, batch, h, w):
        return int(_lib.lib().basic_conv_plan_flops(self._h, int(batch), int(h), int(w)))

    def launches(self, batch, h, w):
        """Kernel launches of one forward call on a [batch, cin, h, w] input."""
        return int(_lib.lib().basic_conv_plan_launches(self._h, int(batch), int(h), int(w)))

    def __call__(self, x, out=None):
        x = _dev(x, torch.float32)
        B, C, H, W = x.shape
        if C != self.cin:
            raise ValueError(f"conv plan expects {self.cin} input channels, got {C}")
        oh, ow = self.out_hw(H, W)
        if out is None:
            out = torch.empty((B, self.cout, oh, ow), device=x.device, dtype=torch.float32)
        _lib.check(_lib.lib().basic_conv_forward_dev(self._h, x.data_ptr(), B, H, W, out.data_ptr(), _stream()))
        return out


MCONV_KERNEL_NONE, MCONV_KERNEL_GATHER, MCONV_KERNEL_BLOCK, MCONV_KERNEL_DMA = -1, 0, 1, 2


def mconv_choose(cin, cout, ksize, in_groups, out_groups, batch, h, w, n_pos):
    """MCONV_KERNEL_* a MaskedConvPlan of this layer would launch for n_pos listed positions of `batch` h x w maps
    (basic_mconv_choose: host code, no device needed; honours BASIC_MCONV_KERNEL)."""
    k = ctypes.c_int(MCONV_KERNEL_NONE)
    _lib.check(_lib.lib().basic_mconv_choose(int(cin), int(cout), int(ksize), int(in_groups), int(out_groups), int(batch), int(h),
                                             int(w), int(n_pos), ctypes.byref(k)))
    return k.value


class MaskedConvPlan:
    """basic_mconv_plan_*: topo-group masked conv evaluated at a position list."""

    def __init__(self, weight, bias, in_groups, out_groups, allow_same, act=ACT_NONE):
        w = _f32(weight)
        b = _f32(bias) if bias is not None else None
        self.cout, self.cin, self.k = w.shape[0], w.shape[1], w.shape[2]
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().basic_mconv_plan_create(w.ctypes.data, b.ctypes.data if b is not None else None, self.cin,
                                                      self.cout, self.k, int(in_groups), int(out_groups), int(bool(allow_same)),
                                                      int(act), ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().basic_mconv_plan_destroy(h)
            except Exception:
                pass

    @property
    def last_kernel(self):
        """MCONV_KERNEL_* the last call launched; MCONV_KERNEL_NONE before any launch."""
        k = ctypes.c_int(MCONV_KERNEL_NONE)
        _lib.check(_lib.lib().basic_mconv_last_kernel(self._h, ctypes.byref(k)))
        return k.value

    def __call__(self, x, topo_in, topo_out, pos, out, out_offset=0, step=None, first_step=None, in_perm=None, out_perm=None):
        """step / first_step: the coding-loop variant that only evaluates the (output group, position) pairs of the current
        step.  in_perm / out_perm (int32 [H*W]): position permutation inside the planes of x / out (private buffers of a
        chain of 1x1 layers; see basic_mconv_forward_ex_dev)."""
        x = _dev(x, torch.float32)
        B, C, H, W = x.shape
        topo_in, topo_out, pos = _dev(topo_in, torch.int32), _dev(topo_out, torch.int32), _dev(pos, torch.int32)
        out = _dev(out, torch.float32)
        if step is not None:
            first_step = _dev(first_step, torch.int32)
        in_perm = _dev(in_perm, torch.int32) if in_perm is not None else None
        out_perm = _dev(out_perm, torch.int32) if out_perm is not None else None
        _lib.check(_lib.lib().basic_mconv_forward_ex_dev(
            self._h, x.data_ptr(), topo_in.data_ptr(), topo_out.data_ptr(), B, H, W, pos.data_ptr(), pos.numel(), out.data_ptr(),
            out.shape[1], int(out_offset), int(step is not None), int(step) if step is not None else 0,
            first_step.data_ptr() if step is not None else None, in_perm.data_ptr() if in_perm is not None else None,
            out_perm.data_ptr() if out_perm is not None else None, _stream()))
        return out


# BASIC_RANS_KERNEL_* (include/basic_hip.h): what a rANS launch ran
(RANS_KERNEL_NONE, RANS_KERNEL_ENC_FAST, RANS_KERNEL_ENC_GENERAL, RANS_KERNEL_ENC_GENERAL_AR, RANS_KERNEL_DEC_FAST,
 RANS_KERNEL_DEC_GENERAL_LDS, RANS_KERNEL_DEC_GENERAL_GLOBAL, RANS_KERNEL_DEC_AR_LDS, RANS_KERNEL_DEC_AR_GLOBAL) = range(-1, 8)
RANS_KERNEL_NAMES = {RANS_KERNEL_NONE: "NONE", RANS_KERNEL_ENC_FAST: "ENC_FAST", RANS_KERNEL_ENC_GENERAL: "ENC_GENERAL",
                     RANS_KERNEL_ENC_GENERAL_AR: "ENC_GENERAL_AR", RANS_KERNEL_DEC_FAST: "DEC_FAST",
                     RANS_KERNEL_DEC_GENERAL_LDS: "DEC_GENERAL_LDS", RANS_KERNEL_DEC_GENERAL_GLOBAL: "DEC_GENERAL_GLOBAL",
                     RANS_KERNEL_DEC_AR_LDS: "DEC_AR_LDS", RANS_KERNEL_DEC_AR_GLOBAL: "DEC_AR_GLOBAL"}


def rans_last_launch():
    """(RANS_KERNEL_*, wavefronts per workgroup) of the calling thread's last rANS launch; (RANS_KERNEL_NONE, 0) before any."""
    k, w = ctypes.c_int(RANS_KERNEL_NONE), ctypes.c_int(0)
    _lib.check(_lib.lib().basic_rans_last_launch(ctypes.byref(k), ctypes.byref(w)))
    return k.value, w.value


@contextlib.contextmanager
def rans_waves(w):
    """Wavefronts (streams) per workgroup of the fast rANS kernels inside the block, for the calling thread: 1, 2, 4, 8 or 16
    (0: the environment's BASIC_RANS_WPB).  The previous value comes back on exit."""
    prev = ctypes.c_int(0)
    _lib.check(_lib.lib().basic_rans_set_waves(int(w), ctypes.byref(prev)))
    try:
        yield
    finally:
        _lib.check(_lib.lib().basic_rans_set_waves(prev.value, None))


class RansTables:
    """Device-resident CDF tables (basic_rans_tables_*) for the batched stream coder."""

    def __init__(self, freqs=None, nsym=None, offsets=None, cdfs=None, cdf_sizes=None, precision=16, bypass=True,
                 bypass_precision=4):
        h = ctypes.c_void_p()
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        if cdfs is not None:
            c = np.ascontiguousarray(cdfs, dtype=np.int32)
            s = np.ascontiguousarray(cdf_sizes, dtype=np.int32)
            _lib.check(_lib.lib().basic_rans_tables_from_cdfs(c.ctypes.data, c.shape[0], c.shape[1], s.ctypes.data, off.ctypes.data,
                                                              precision, int(bypass), bypass_precision, ctypes.byref(h)))
        else:
            f = np.ascontiguousarray(freqs, dtype=np.int32)
            n = np.ascontiguousarray(nsym, dtype=np.int32)
            _lib.check(_lib.lib().basic_rans_tables_from_freqs(f.ctypes.data, f.shape[0], f.shape[1], n.ctypes.data, off.ctypes.data,
                                                               precision, int(bypass), bypass_precision, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().basic_rans_tables_destroy(h)
            except Exception:
                pass

    @staticmethod
    def last_launch():
        """rans_last_launch(): tables do not launch on their own thread, so the record is the calling thread's."""
        return rans_last_launch()

    def get_cdfs(self):
        rows, mx = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.lib().basic_rans_tables_info(self._h, ctypes.byref(rows), ctypes.byref(mx)))
        out = np.zeros((rows.value, mx.value), dtype=np.int32)
        _lib.check(_lib.lib().basic_rans_tables_get_cdfs(self._h, out.ctypes.data, mx.value))
        return out

    def encode_batch(self, symbols, indexes, seg, slot_words=None):
        """symbols/indexes int32 [total]; seg int64 [nstreams+1] -> (words [nstreams, slot], nwords [nstreams])."""
        symbols, indexes, seg = _dev(symbols, torch.int32), _dev(indexes, torch.int32), _dev(seg, torch.int64)
        ns = seg.numel() - 1
        if slot_words is None:
            raise ValueError("slot_words is required")
        if symbols.numel() == 0:  # every stream empty: the C ABI still wants valid pointers
            symbols = indexes = torch.zeros((1,), device=seg.device, dtype=torch.int32)
        words = torch.empty((ns, slot_words), device=symbols.device, dtype=torch.int32)
        nwords = torch.empty((ns,), device=symbols.device, dtype=torch.int32)
        _lib.check(_lib.lib().basic_rans_encode_batch_dev(self._h, symbols.data_ptr(), indexes.data_ptr(), seg.data_ptr(), ns,
                                                          words.data_ptr(), slot_words, nwords.data_ptr(), _stream()))
        return words, nwords

    # ---- batched streams <-> host bytes.  begin() only enqueues GPU work (encode, device-side offsets, compaction);
    # end() is the single host synchronisation, so a caller can launch more kernels in between.
    def encode_batch_begin(self, symbols, indexes, n_per_stream, slot=None, seg=None):
        """``seg`` (skip coding): an int64 device tensor [ns + 1] bounding streams of unequal lengths inside symbols / indexes, as
        skip_compact writes it; ``n_per_stream`` is then the bound of a stream's length that sizes the slots."""
        symbols, indexes = _dev(symbols, torch.int32), _dev(indexes, torch.int32)
        given = seg
        if seg is None:
            ns = symbols.numel() // n_per_stream
            seg = torch.arange(ns + 1, device=symbols.device, dtype=torch.int64) * n_per_stream
        else:
            seg = _dev(seg, torch.int64)
            ns = seg.numel() - 1
        slot = slot or n_per_stream + 2  # the reference's own buffer size (rans64.cpp:240)
        words, nwords = self.encode_batch(symbols, indexes, seg, slot)
        d_off = torch.zeros((ns + 1,), device=symbols.device, dtype=torch.int64)
        torch.cumsum(nwords.clamp(min=0), 0, out=d_off[1:])
        packed = torch.empty((ns * slot,), device=symbols.device, dtype=torch.int32)
        _lib.check(_lib.lib().basic_rans_compact_streams_dev(words.data_ptr(), slot, nwords.data_ptr(), d_off.data_ptr(), ns,
                                                             packed.data_ptr(), _stream()))
        return dict(symbols=symbols, indexes=indexes, n=n_per_stream, ns=ns, slot=slot, nwords=nwords, packed=packed, keep=words,
                    seg=given)

    def _pinned(self, which, nbytes):
        """Page-locked staging buffer owned by this table set (D2H of encoded words / H2D of words to decode): DMA at
        full PCIe rate instead of the pageable path's bounce copies.  Grows geometrically, one per direction."""
        buf = getattr(self, "_pin_" + which, None)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty((max(nbytes, 1 << 16) * 3 // 2,), dtype=torch.uint8, pin_memory=True)
            setattr(self, "_pin_" + which, buf)
        return buf

    def encode_batch_end(self, h):
        """-> (uint32 words of all streams back to back (numpy), int64 word offsets [ns + 1]).  The words live in this
        table set's pinned staging buffer: valid until its next encode_batch_end()."""
        nw = h["nwords"].cpu().numpy()
        if (nw < 0).any():  # bypass-heavy data overflowed the reference's bound: redo with the guaranteed one
            h = self.encode_batch_begin(h["symbols"], h["indexes"], h["n"], slot=3 * h["n"] + 4, seg=h.get("seg"))
            nw = h["nwords"].cpu().numpy()
        off = np.zeros(h["ns"] + 1, dtype=np.int64)
        np.cumsum(nw, out=off[1:])
        n = int(off[-1])
        stage = self._pinned("out", 4 * n)[: 4 * n].view(torch.int32)
        stage.copy_(h["packed"][:n], non_blocking=True)
        torch.cuda.current_stream(h["packed"].device).synchronize()
        return stage.numpy().view(np.uint32), off

    def encode_batch_to_bytes(self, symbols, indexes, n_per_stream):
        """Equal-length streams (one per image): returns a list of ``bytes`` (reference py::bytes)."""
        host, off = self.encode_batch_end(self.encode_batch_begin(symbols, indexes, n_per_stream))
        return [host[off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]

    def _stage_in(self, nwords):
        """uint32 numpy view of nwords words of the pinned H2D staging buffer (waits for the previous DMA out of it)."""
        ev = getattr(self, "_pin_in_event", None)
        if ev is not None:
            ev.synchronize()
        return self._pinned("in", 4 * max(nwords, 1))[: 4 * nwords].view(torch.int32)

    def decode_batch_from_frame(self, data, indexes, n_per_stream, seg=None):
        """Framed body (frame_streams / write_body) -> int32 symbols like ``indexes``: the payloads are unframed by the C
        helper straight into the pinned staging buffer and DMA'd from there.  ``seg`` (skip coding): an int64 device tensor, one
        entry more than the body has streams, bounding the streams' symbols inside ``indexes`` instead of ``n_per_stream``."""
        h, w, n = frame_header(data)
        if seg is not None and seg.numel() != n + 1:
            raise ValueError(f"stream body holds {n} streams, the segment tensor bounds {seg.numel() - 1}")
        stage = self._stage_in((len(data) - 12 - 4 * n) // 4)
        words, word_off, _ = unframe_streams(data, out=stage.numpy().view(np.uint32))
        return self._decode_staged(stage[: words.size], word_off, indexes, n_per_stream, seg=seg)

    def decode_batch_from_words(self, host_words, word_off, indexes, n_per_stream):
        """Streams given as one uint32 array + word offsets (see unframe_streams): int32 symbols like ``indexes``."""
        stage = self._stage_in(host_words.size)
        stage.numpy()[:] = host_words.view(np.int32)
        return self._decode_staged(stage, word_off, indexes, n_per_stream)

    def _decode_staged(self, stage, word_off, indexes, n_per_stream, seg=None):
        indexes = _dev(indexes, torch.int32)
        ns = len(word_off) - 1
        d_words = stage.to(indexes.device, non_blocking=True)
        self._pin_in_event = torch.cuda.Event()
        self._pin_in_event.record(torch.cuda.current_stream(indexes.device))
        d_woff = torch.from_numpy(np.ascontiguousarray(word_off, dtype=np.int64)).to(indexes.device)
        if seg is None:
            seg = torch.arange(ns + 1, device=indexes.device, dtype=torch.int64) * n_per_stream
        out, _, _ = self.decode_batch(d_words, d_woff, indexes, seg)
        return out

    def decode_batch_from_bytes(self, strings, indexes, n_per_stream):
        """Inverse of encode_batch_to_bytes: int32 symbols shaped like ``indexes`` (device)."""
        for s in strings:
            if len(s) < 8 or len(s) % 4:
                raise ValueError("rANS stream must hold >= 2 whole 32-bit words")
        lens = np.array([len(s) // 4 for s in strings], dtype=np.int64)
        woff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        host = np.frombuffer(b"".join(strings), dtype=np.uint32).copy()
        return self.decode_batch_from_words(host, woff, indexes, n_per_stream)

    def decode_batch_lanes(self, words, word_off, indexes, first, stride, lanes, count, nimages, out, state, pos):
        """basic_rans_decode_batch_lanes_dev: stream b * lanes + k continues with the `count` symbols at first + b * stride +
        k * count of ``indexes`` / ``out`` (int32, device); state / pos int64 [nimages * lanes] as in decode_batch."""
        _lib.check(_lib.lib().basic_rans_decode_batch_lanes_dev(self._h, words.data_ptr(), word_off.data_ptr(), indexes.data_ptr(), int(first),
                                                                int(stride), int(lanes), int(count), int(nimages), out.data_ptr(),
                                                                state.data_ptr(), pos.data_ptr(), _stream()))
        return out, state, pos

    def decode_batch_streams(self, words, word_off, indexes, first, stride, lanes, count, nimages, stream_first, stream_stride, out, state, pos):
        """basic_rans_decode_batch_streams_dev: decode_batch_lanes with a stream base and stride -- the launch's stream (b, k) is
        stream stream_first + b * stream_stride + k of ``word_off`` / ``state`` / ``pos``."""
        _lib.check(_lib.lib().basic_rans_decode_batch_streams_dev(self._h, words.data_ptr(), word_off.data_ptr(), indexes.data_ptr(), int(first),
                                                                  int(stride), int(lanes), int(count), int(nimages), int(stream_first),
                                                                  int(stream_stride), out.data_ptr(), state.data_ptr(), pos.data_ptr(), _stream()))
        return out, state, pos

    def decode_batch(self, words, word_off, indexes, seg, out=None, state=None, pos=None):
        words, word_off = _dev(words, torch.int32), _dev(word_off, torch.int64)
        indexes, seg = _dev(indexes, torch.int32), _dev(seg, torch.int64)
        ns = seg.numel() - 1
        if out is None:
            out = torch.empty_like(indexes)
        if indexes.numel() == 0:  # every stream empty: nothing to decode
            return out, state, pos
        if state is None:
            state = torch.zeros((ns,), device=words.device, dtype=torch.int64)
            pos = torch.full((ns,), -1, device=words.device, dtype=torch.int64)
        _lib.check(_lib.lib().basic_rans_decode_batch_dev(self._h, words.data_ptr(), word_off.data_ptr(), indexes.data_ptr(),
                                                          seg.data_ptr(), ns, out.data_ptr(), state.data_ptr(), pos.data_ptr(), _stream()))
        return out, state, pos


def gc_quantize_index(y, scales, table, bound=0.11, want_yhat=True):
    y, scales, table = _dev(y, torch.float32), _dev(scales, torch.float32), _dev(table, torch.float32)
    sym = torch.empty(y.shape, device=y.device, dtype=torch.int32)
    idx = torch.empty(y.shape, device=y.device, dtype=torch.int32)
    yhat = torch.empty_like(y) if want_yhat else None
    _lib.check(_lib.lib().basic_gc_quantize_index_dev(y.data_ptr(), scales.data_ptr(), y.numel(), table.data_ptr(), table.numel(),
                                                      float(bound), sym.data_ptr(), idx.data_ptr(),
                                                      yhat.data_ptr() if yhat is not None else None, _stream()))
    return sym, idx, yhat


def qsteps_tensor(steps, batch, device):
    """Quantiser steps (a number, a sequence, an array or a tensor) as a float32 device tensor of 1 or ``batch`` elements,
    validated on the host first (utils/qstep.py: finite, in [2^-4, 2^6], one or one per image) -- ValueError otherwise, nothing launched."""
    from ..utils.qstep import check_qsteps
    return torch.from_numpy(check_qsteps(steps, batch)).to(device)


def _per_image(t):
    if t.dim() < 1 or t.shape[0] < 1:
        raise ValueError("the step kernels take [B, ...] tensors with B >= 1")
    return t.shape[0], t.numel() // t.shape[0]


def gc_quantize_index_q(y, scales, steps, table, bound=0.11, want_yhat=True, steps_on_device=False):
    """gc_quantize_index under a quantiser step per image of the [B, ...] latent (basic_gc_quantize_index_q_dev):
    sym = rint(y / step), idx from max(scale, bound) / step, yhat = sym * step.  ``steps``: see qsteps_tensor; with
    ``steps_on_device`` a float32 device tensor of 1 or B steps that a kernel chose among validated candidates (rate_select), read
    where it lies -- nothing comes back to the host."""
    y, scales, table = _dev(y, torch.float32), _dev(scales, torch.float32), _dev(table, torch.float32)
    B, per = _per_image(y)
    if steps_on_device:
        steps = _dev(steps, torch.float32)
        if steps.numel() not in (1, B):
            raise ValueError(f"{steps.numel()} quantiser steps for a batch of {B}: give one, or one per image")
    else:
        steps = qsteps_tensor(steps, B, y.device)
    sym = torch.empty(y.shape, device=y.device, dtype=torch.int32)
    idx = torch.empty(y.shape, device=y.device, dtype=torch.int32)
    yhat = torch.empty_like(y) if want_yhat else None
    _lib.check(_lib.lib().basic_gc_quantize_index_q_dev(y.data_ptr(), scales.data_ptr(), y.numel(), per, steps.data_ptr(), steps.numel(),
                                                        table.data_ptr(), table.numel(), float(bound), sym.data_ptr(), idx.data_ptr(),
                                                        yhat.data_ptr() if yhat is not None else None, _stream()))
    return sym, idx, yhat


def gc_dequantize_q(sym, steps):
    """float(sym) * step of the image, for a [B, ...] int32 tensor (basic_gc_dequantize_q_dev): the encoder's yhat bit for bit."""
    sym = _dev(sym, torch.int32)
    B, per = _per_image(sym)
    steps = qsteps_tensor(steps, B, sym.device)
    out = torch.empty(sym.shape, device=sym.device, dtype=torch.float32)
    _lib.check(_lib.lib().basic_gc_dequantize_q_dev(sym.data_ptr(), sym.numel(), per, steps.data_ptr(), steps.numel(), out.data_ptr(),
                                                    _stream()))
    return out


# ---- mean-scale y coder (INTEGRATION.md "Mean-scale hyperprior"): sym = rint(y - mu), yhat = sym + mu
def _ms_params(prior, means, B, per, what):
    """-> (scales address, means address, param_stride, tensors to keep alive) of the parameters of a [B, ...] latent with ``per``
    elements an image.  ``means`` None: ``prior`` is the chunked prior [B][2 M][...], scales then means along dim 1 (upstream's
    chunk(2, 1)), read in place -- it may be a view of a larger tensor as long as every image's 2 * per elements are contiguous.
    Else ``prior`` holds the scales and ``means`` the means, two contiguous tensors of B * per elements."""
    if means is not None:
        scales, means = _dev(prior, torch.float32), _dev(means, torch.float32)
        if scales.numel() != B * per or means.numel() != B * per:
            raise ValueError(f"{what}: scales and means hold one element per latent element ({B * per})")
        return scales.data_ptr(), means.data_ptr(), per, (scales, means)
    if not isinstance(prior, torch.Tensor) or not prior.is_cuda:
        raise _lib.BasicHipError("cbench_basic_amd kernels need tensors on the MI355X (got a CPU tensor); there is no CPU fallback")
    if prior.dtype != torch.float32:
        raise TypeError(f"expected {torch.float32}, got {prior.dtype}")
    if prior.dim() < 2 or prior.shape[0] != B or prior[0].numel() != 2 * per:
        raise ValueError(f"{what}: the chunked prior is [B][2 M][...] with twice the latent's {per} elements an image, got {tuple(prior.shape)}")
    if not prior[0].is_contiguous() or (B > 1 and prior.stride(0) < 2 * per):
        raise ValueError(f"{what}: the prior of an image must be contiguous (scales then means); call .contiguous() on it")
    stride = prior.stride(0) if B > 1 else 2 * per
    return prior.data_ptr(), prior.data_ptr() + 4 * per, stride, (prior,)


def _ms_steps(steps, B, device, steps_on_device):
    if steps is None:
        return None
    if steps_on_device:
        steps = _dev(steps, torch.float32)
        if steps.numel() not in (1, B):
            raise ValueError(f"{steps.numel()} quantiser steps for a batch of {B}: give one, or one per image")
        return steps
    return qsteps_tensor(steps, B, device)


def gc_quantize_index_ms(y, prior, table, bound=0.11, steps=None, means=None, want_yhat=True, steps_on_device=False):
    """basic_gc_quantize_index_ms_dev on a [B, ...] latent: sym = rint(y - mu) (rint((y - mu) / step) with ``steps``), idx from
    max(scale, bound) (/ step), yhat = sym + mu ((sym * step) + mu).  ``prior`` / ``means``: see _ms_params.  ``y`` None: indexes
    only (the decoder) -- the latent's shape is then the scales half of ``prior`` (or ``prior`` itself with ``means``), and
    (None, idx, None) comes back."""
    table = _dev(table, torch.float32)
    if y is None:
        if means is None:
            if prior.dim() < 2 or prior.shape[1] % 2:
                raise ValueError("gc_quantize_index_ms: the chunked prior is [B][2 M][...]")
            shape = (prior.shape[0], prior.shape[1] // 2) + tuple(prior.shape[2:])
        else:
            shape = tuple(prior.shape)
        B, per = shape[0], int(np.prod(shape[1:]))
        device = prior.device
    else:
        y = _dev(y, torch.float32)
        B, per = _per_image(y)
        shape, device = tuple(y.shape), y.device
    ps, pm, stride, keep = _ms_params(prior, means, B, per, "gc_quantize_index_ms")
    steps = _ms_steps(steps, B, device, steps_on_device)
    idx = torch.empty(shape, device=device, dtype=torch.int32)
    sym = torch.empty(shape, device=device, dtype=torch.int32) if y is not None else None
    yhat = torch.empty(shape, device=device, dtype=torch.float32) if (y is not None and want_yhat) else None
    _lib.check(_lib.lib().basic_gc_quantize_index_ms_dev(
        y.data_ptr() if y is not None else None, ps, pm if y is not None else None, B * per, per, stride,
        steps.data_ptr() if steps is not None else None, steps.numel() if steps is not None else 0, table.data_ptr(), table.numel(),
        float(bound), sym.data_ptr() if sym is not None else None, idx.data_ptr(), yhat.data_ptr() if yhat is not None else None, _stream()))
    del keep
    return sym, idx, yhat


def gc_dequantize_ms(sym, prior, steps=None, means=None):
    """float(sym) + mu, or (float(sym) * step) + mu, for a [B, ...] int32 tensor (basic_gc_dequantize_ms_dev).  ``prior`` / ``means``:
    see _ms_params (of a chunked prior only the means half is read)."""
    sym = _dev(sym, torch.int32)
    B, per = _per_image(sym)
    _, pm, stride, keep = _ms_params(prior, means, B, per, "gc_dequantize_ms")
    steps = _ms_steps(steps, B, sym.device, False)
    out = torch.empty(sym.shape, device=sym.device, dtype=torch.float32)
    _lib.check(_lib.lib().basic_gc_dequantize_ms_dev(sym.data_ptr(), pm, sym.numel(), per, stride,
                                                     steps.data_ptr() if steps is not None else None,
                                                     steps.numel() if steps is not None else 0, out.data_ptr(), _stream()))
    del keep
    return out


# ---- rate control (INTEGRATION.md "Rate control"): the coder's exact table cost at K candidate steps from one read of y and sigma
def rans_cost_table(cdfs, cdf_sizes, precision=16):
    """basic_rans_cost_table_host: uint32 [rows][stride] bit costs (2^-16 bit) of the symbols of int32 [rows][stride] cdfs.  Host
    code: it runs without a GPU."""
    c = np.ascontiguousarray(cdfs, dtype=np.int32)
    s = np.ascontiguousarray(cdf_sizes, dtype=np.int32).reshape(-1)
    if c.ndim != 2 or s.size != c.shape[0]:
        raise ValueError("rans_cost_table: cdfs is [rows][stride], cdf_sizes [rows]")
    out = np.zeros(c.shape, dtype=np.uint32)
    _lib.check(_lib.lib().basic_rans_cost_table_host(c.ctypes.data, c.shape[0], c.shape[1], s.ctypes.data, int(precision), out.ctypes.data))
    return out


def rans_tables_costs(tables):
    """The cost table of a RansTables set as its rate kernels read it: uint32 [rows][max cdf length]."""
    rows, mx = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().basic_rans_tables_info(tables._h, ctypes.byref(rows), ctypes.byref(mx)))
    out = np.zeros((rows.value, mx.value), dtype=np.uint32)
    _lib.check(_lib.lib().basic_rans_tables_costs(tables._h, out.ctypes.data))
    return out


def _rate_cand(cand, images):
    """-> (float32 device tensor, n_cand, cand_per_image) of a [K] (shared) or [B][K] (one grid per image) candidate tensor."""
    cand = _dev(cand, torch.float32)
    if cand.dim() == 1:
        return cand, cand.shape[0], 0
    if cand.dim() != 2 or cand.shape[0] != images:
        raise ValueError(f"candidates are [K] or [{images}][K], got {tuple(cand.shape)}")
    return cand, cand.shape[1], 1


CHUNKED = "chunked"   # means=CHUNKED: the ``scales`` argument is the chunked prior [B][2 M][...], scales then means, read in place


def rate_curve(y, scales, cand, table, tables, bound=0.11, lanes=1, out=None, means=None):
    """basic_gc_rate_curve_dev on a [B, ...] latent: int64 [B * lanes][K], entry (b * lanes + l, k) = the summed table cost (2^-16 bit)
    of lane stream l of image b at step ``cand[k]`` (``cand``: float32 device tensor [K], or [B][K] with a grid per image; the values
    are the caller's to validate).  ``tables``: the RansTables that will code the symbols.  ``out``: a contiguous int64 [B * lanes][K]
    device tensor to write instead of a new one (the rows of a larger curve tensor).  ``means``: the mean-scale coder's curve
    (basic_gc_rate_curve_ms_dev), the costs of rint((y - mu) / step) -- a tensor of means beside ``scales``, or CHUNKED when
    ``scales`` is the chunked prior (_ms_params)."""
    y, table = _dev(y, torch.float32), _dev(table, torch.float32)
    B, per = _per_image(y)
    ms = None
    if means is not None:
        ms = _ms_params(scales, None if isinstance(means, str) and means == CHUNKED else means, B, per, "rate_curve")
    else:
        scales = _dev(scales, torch.float32)
        if scales.numel() != y.numel():
            raise ValueError("rate_curve: y and scales must hold the same number of elements")
    if lanes < 1 or per % lanes:
        raise ValueError(f"rate_curve: {lanes} lanes do not divide the {per} symbols of an image")
    cand, K, cpi = _rate_cand(cand, B)
    if out is None:
        bits = torch.empty((B * lanes, K), device=y.device, dtype=torch.int64)
    else:
        bits = out
        if bits.dtype != torch.int64 or bits.device != y.device or tuple(bits.shape) != (B * lanes, K) or not bits.is_contiguous():
            raise ValueError(f"rate_curve: out is a contiguous int64 [{B * lanes}][{K}] tensor on the latent's device")
    if ms is not None:
        _lib.check(_lib.lib().basic_gc_rate_curve_ms_dev(y.data_ptr(), ms[0], ms[1], ms[2], B * lanes, per // lanes, int(lanes),
                                                         cand.data_ptr(), K, cpi, table.data_ptr(), table.numel(), float(bound),
                                                         tables._h, bits.data_ptr(), _stream()))
        return bits
    _lib.check(_lib.lib().basic_gc_rate_curve_dev(y.data_ptr(), scales.data_ptr(), B * lanes, per // lanes, int(lanes), cand.data_ptr(), K, cpi,
                                                  table.data_ptr(), table.numel(), float(bound), tables._h, bits.data_ptr(), _stream()))
    return bits


def rate_select(bits, per_seg, cand, budgets, extra_words=None, lanes=1):
    """basic_rate_select_dev: (steps float32 [B], choice int32 [B], pred_bytes int64 [B]) from the curves ``bits`` int64 [B * lanes][K],
    the candidates ([K] or [B][K]), byte budgets int64 [B] and, when given, int32 [B] words already spent per image."""
    bits = _dev(bits, torch.int64)
    B = bits.shape[0] // lanes
    cand, K, cpi = _rate_cand(cand, B)
    budgets = _dev(budgets, torch.int64)
    if bits.dim() != 2 or bits.shape[0] != B * lanes or bits.shape[1] != K or budgets.numel() != B:
        raise ValueError("rate_select: bits is [B * lanes][K] and budgets [B]")
    if extra_words is not None:
        extra_words = _dev(extra_words, torch.int32)
        if extra_words.numel() != B:
            raise ValueError("rate_select: extra_words is [B]")
    steps = torch.empty((B,), device=bits.device, dtype=torch.float32)
    choice = torch.empty((B,), device=bits.device, dtype=torch.int32)
    pred = torch.empty((B,), device=bits.device, dtype=torch.int64)
    _lib.check(_lib.lib().basic_rate_select_dev(bits.data_ptr(), B, int(lanes), int(per_seg), cand.data_ptr(), K, cpi,
                                                extra_words.data_ptr() if extra_words is not None else None, budgets.data_ptr(),
                                                steps.data_ptr(), choice.data_ptr(), pred.data_ptr(), _stream()))
    return steps, choice, pred


def rate_refine(cand, choice, t=None):
    """basic_rate_refine_dev: the next grids float32 [B][K] between every image's chosen candidate and the one below it."""
    choice = _dev(choice, torch.int32)
    B = choice.numel()
    cand, K, cpi = _rate_cand(cand, B)
    if t is None:
        from ..utils.rate import refine_t
        t = torch.from_numpy(refine_t(K)).to(cand.device)
    t = _dev(t, torch.float32)
    if t.numel() != K:
        raise ValueError("rate_refine: t is [K]")
    out = torch.empty((B, K), device=cand.device, dtype=torch.float32)
    _lib.check(_lib.lib().basic_rate_refine_dev(cand.data_ptr(), cpi, K, choice.data_ptr(), B, t.data_ptr(), out.data_ptr(), _stream()))
    return out


def rate_steps(y, scales, budgets, extra_words, candidates, passes, table, tables, bound=0.11, lanes=1, return_trace=False, means=None):
    """curve -> select -> (refine -> curve -> select) x (passes - 1) on the device, nothing synchronised: (steps float32 [B], choice
    int32 [B], pred_bytes int64 [B]) of the last pass.  ``candidates``: the first grid, validated on the host (utils/rate.py);
    ``budgets``: int64 [B] device tensor.  ``return_trace``: also the list of every pass's (candidates, bits, choice).  ``means``: as
    rate_curve's."""
    from ..utils.rate import check_candidates, check_passes, refine_t
    passes = check_passes(passes)
    B, per = _per_image(y)
    cand = torch.from_numpy(check_candidates(candidates)).to(y.device)
    t = torch.from_numpy(refine_t(cand.numel())).to(y.device)
    trace = []
    for p in range(passes):
        if p:
            cand = rate_refine(cand, choice, t)
        bits = rate_curve(y, scales, cand, table, tables, bound, lanes, means=means)
        steps, choice, pred = rate_select(bits, per // lanes, cand, budgets, extra_words, lanes)
        trace.append((cand, bits, choice))
    return (steps, choice, pred, trace) if return_trace else (steps, choice, pred)


def _group_csr(groups, n_tiles):
    """Groups (a sequence of sequences of tile numbers) as the host CSR arrays (group_first int32 [G + 1], group_tiles int32 [listed])
    and tile_group int64 [n_tiles], the group of every tile (-1: in none)."""
    first, tiles = [0], []
    tile_group = np.full(int(n_tiles), -1, dtype=np.int64)
    for g, members in enumerate(groups):
        members = [int(t) for t in members]
        tiles.extend(members)
        first.append(len(tiles))
        for t in members:
            if 0 <= t < n_tiles:
                tile_group[t] = g
    return np.asarray(first, dtype=np.int32), np.asarray(tiles, dtype=np.int32).reshape(-1), tile_group


def rate_select_groups(bits, tile_first_seg, tile_per_seg, groups, cand, budgets, tile_extra_words=None, lanes=1, block_threads=0):
    """basic_rate_select_groups_dev: rate_select with GROUPS of tiles in the place of images -- a group (a tiled picture) has one budget
    over all its tiles.  ``bits`` int64 [S][K]; tile t owns rows ``tile_first_seg[t]`` .. + lanes - 1, streams of ``tile_per_seg[t]``
    symbols; ``groups``: a sequence of sequences of tile numbers (or the CSR pair ``(group_first, group_tiles)``); ``cand`` [K] or
    [G][K]; ``budgets`` int64 [G]; ``tile_extra_words`` int32 [T] on the device or None.  The plan arrays are host data, checked by the
    entry point before it enqueues anything.  -> (steps float32 [G], choice int32 [G], pred_bytes int64 [G], tile_steps float32 [T],
    tile_pred int64 [T]); a tile in no group keeps step 1 and prediction 0."""
    bits = _dev(bits, torch.int64)
    first_seg = np.ascontiguousarray(tile_first_seg, dtype=np.int32).reshape(-1)
    per_seg = np.ascontiguousarray(tile_per_seg, dtype=np.int64).reshape(-1)
    T = first_seg.size
    if isinstance(groups, tuple) and len(groups) == 2 and isinstance(groups[0], np.ndarray):
        gfirst, gtiles = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in groups)
    else:
        gfirst, gtiles, _ = _group_csr(groups, T)
    G = gfirst.size - 1
    if bits.dim() != 2 or per_seg.size != T or T < 1 or G < 1 or gtiles.size != int(gfirst[-1]):
        raise ValueError("rate_select_groups: bits is [S][K], tile_first_seg and tile_per_seg are [T], the groups list tiles")
    cand, K, cpg = _rate_cand(cand, G)
    budgets = _dev(budgets, torch.int64)
    if bits.shape[1] != K or budgets.numel() != G:
        raise ValueError("rate_select_groups: bits is [S][K] and budgets [G]")
    if tile_extra_words is not None:
        tile_extra_words = _dev(tile_extra_words, torch.int32)
        if tile_extra_words.numel() != T:
            raise ValueError("rate_select_groups: tile_extra_words is [T]")
    dev = bits.device
    plan = torch.empty(((16 * T + 4 * (G + 1) + 7) // 8,), device=dev, dtype=torch.int64)
    steps = torch.empty((G,), device=dev, dtype=torch.float32)
    choice = torch.empty((G,), device=dev, dtype=torch.int32)
    pred = torch.empty((G,), device=dev, dtype=torch.int64)
    tile_steps = torch.ones((T,), device=dev, dtype=torch.float32)
    tile_pred = torch.zeros((T,), device=dev, dtype=torch.int64)
    _lib.check(_lib.lib().basic_rate_select_groups_dev(
        bits.data_ptr(), int(bits.shape[0]), int(lanes), T, first_seg.ctypes.data, per_seg.ctypes.data,
        tile_extra_words.data_ptr() if tile_extra_words is not None else None, G, gfirst.ctypes.data, gtiles.ctypes.data, plan.data_ptr(),
        cand.data_ptr(), K, cpg, budgets.data_ptr(), steps.data_ptr(), choice.data_ptr(), pred.data_ptr(), tile_steps.data_ptr(),
        tile_pred.data_ptr(), int(block_threads), _stream()))
    return steps, choice, pred, tile_steps, tile_pred


def rate_steps_groups(chunks, groups, budgets, tile_extra_words, candidates, passes, table, tables, bound=0.11, lanes=1,
                      return_trace=False, means=None):
    """rate_steps over the tiles of many pictures: ``chunks`` is a list of (y, scales) pairs of [B_c, ...] latents (one per pooled coding
    call; the tiles are numbered through the chunks in order), ``groups`` the tile numbers of every picture.  Per pass: one
    rate_curve per chunk into that chunk's rows of ONE curve tensor (every tile under its own picture's candidate grid), one
    rate_select_groups, and between passes one rate_refine with groups in the place of images.  Nothing is synchronised.
    -> (steps [G], choice [G], pred_bytes [G], tile_steps [T], tile_pred [T]) of the last pass; ``return_trace``: also the list of
    every pass's (candidates, bits, choice).  ``means``: the mean-scale coder -- CHUNKED when every chunk's ``scales`` is its chunked
    prior, or a list of one tensor of means per chunk (rate_curve)."""
    from ..utils.rate import check_candidates, check_passes, refine_t
    passes = check_passes(passes)
    grid0 = check_candidates(candidates)
    chunks = list(chunks)
    if means is None or isinstance(means, str):
        chunk_means = [means] * len(chunks)
    else:
        chunk_means = list(means)
        if len(chunk_means) != len(chunks):
            raise ValueError("rate_steps_groups: means is CHUNKED or one tensor per chunk")
    first_seg, per_seg, sizes = [], [], []
    for y, scales in chunks:
        B, per = _per_image(y)
        if means is None and scales.numel() != y.numel():
            raise ValueError("rate_steps_groups: y and scales must hold the same number of elements")
        if lanes < 1 or per % lanes:
            raise ValueError(f"rate_steps_groups: {lanes} lanes do not divide the {per} symbols of a tile")
        first_seg.extend((len(per_seg) + j) * lanes for j in range(B))
        per_seg.extend([per // lanes] * B)
        sizes.append(B)
    T = len(per_seg)
    if T < 1:
        raise ValueError("rate_steps_groups: no tiles")
    gfirst, gtiles, tile_group = _group_csr(groups, T)
    if (tile_group < 0).any():
        raise ValueError("rate_steps_groups: every tile belongs to a group")
    dev = chunks[0][0].device
    K = grid0.size
    cand = torch.from_numpy(grid0).to(dev)
    t = torch.from_numpy(refine_t(K)).to(dev)
    tile_group_dev = torch.from_numpy(tile_group).to(dev)
    bits = torch.empty((T * lanes, K), device=dev, dtype=torch.int64)
    trace = []
    for p in range(passes):
        if p:
            cand = rate_refine(cand, choice, t)
        row = 0
        for (y, scales), B, mu in zip(chunks, sizes, chunk_means):
            mine = cand if cand.dim() == 1 else cand.index_select(0, tile_group_dev[row:row + B])
            rate_curve(y, scales, mine, table, tables, bound, lanes, out=bits[row * lanes:(row + B) * lanes], means=mu)
            row += B
        steps, choice, pred, tile_steps, tile_pred = rate_select_groups(bits, first_seg, per_seg, (gfirst, gtiles), cand, budgets,
                                                                        tile_extra_words, lanes)
        trace.append((cand, bits.clone() if return_trace else None, choice))
    out = (steps, choice, pred, tile_steps, tile_pred)
    return out + (trace,) if return_trace else out


def lanes_pack(sym, idx, batch, positions, channels, lanes):
    """Lane streams of the scan-line coder: both int32 arrays from coding order [B][P][K][L] to [B * K][P * L] (a row per lane
    stream; basic_lanes_pack_dev)."""
    sym, idx = _dev(sym, torch.int32), _dev(idx, torch.int32)
    if sym.numel() != batch * positions * channels or idx.numel() != sym.numel():
        raise ValueError("lanes_pack: arrays must hold batch * positions * channels elements")
    so = torch.empty((batch * lanes, positions * (channels // lanes)), device=sym.device, dtype=torch.int32)
    io = torch.empty_like(so)
    _lib.check(_lib.lib().basic_lanes_pack_dev(sym.data_ptr(), idx.data_ptr(), int(batch), int(positions), int(channels), int(lanes),
                                               so.data_ptr(), io.data_ptr(), _stream()))
    return so, io


def group_lanes_pack(sym, idx, bases, lanes):
    """Lane streams of the group coders: both int32 arrays from group-major coding order [B][n] to [B * K][n / K], row b * K + k =
    the concatenation over the groups of the k-th of K equal parts of each group of image b (basic_group_lanes_pack_dev).
    ``bases``: int64 [G + 1] device tensor, the groups' first elements and n; every group a multiple of K long (the caller checks)."""
    sym, idx, bases = _dev(sym, torch.int32), _dev(idx, torch.int32), _dev(bases, torch.int64)
    if sym.dim() != 2 or idx.shape != sym.shape or bases.numel() < 2:
        raise ValueError("group_lanes_pack: arrays must be [B, n] and bases [G + 1]")
    B, n = sym.shape
    if n % lanes:
        raise ValueError(f"group_lanes_pack: {lanes} lanes do not divide {n} symbols")
    so = torch.empty((B * lanes, n // lanes), device=sym.device, dtype=torch.int32)
    io = torch.empty_like(so)
    _lib.check(_lib.lib().basic_group_lanes_pack_dev(sym.data_ptr(), idx.data_ptr(), int(B), int(n), bases.data_ptr(), int(bases.numel() - 1),
                                                     int(lanes), so.data_ptr(), io.data_ptr(), _stream()))
    return so, io


# ---- skip coding (INTEGRATION.md "Skip coding"): elements whose table row is below skip_rows are not coded
SKIP_CHUNK = 1024   # BASIC_SKIP_CHUNK: the elements of one stream a workgroup pass covers


def skip_scratch_bytes(nstreams, per):
    """BASIC_SKIP_SCRATCH_BYTES."""
    return 8 * int(nstreams) * ((int(per) + SKIP_CHUNK - 1) // SKIP_CHUNK)


def _skip_args(idx, nstreams, skip_rows, what):
    from ..utils.skip import check_skip_rows
    idx = _dev(idx, torch.int32)
    nstreams = int(nstreams)
    if nstreams < 1 or idx.numel() < nstreams or idx.numel() % nstreams:
        raise ValueError(f"{what}: {idx.numel()} elements are no whole number of {nstreams} non-empty streams")
    per = idx.numel() // nstreams
    rows = check_skip_rows(skip_rows, 2 ** 31 - 1)   # the table's length is the coder's to check
    scratch = torch.empty((max(skip_scratch_bytes(nstreams, per) // 8, 1),), device=idx.device, dtype=torch.int64)
    return idx, nstreams, per, rows, scratch


def skip_compact(sym, idx, nstreams, skip_rows):
    """basic_skip_compact_dev on int32 arrays of ``nstreams`` equal streams: -> (sym_c, idx_c, seg), the elements with
    idx >= skip_rows of stream 0, then stream 1, ..., back to back in their order; seg int64 [nstreams + 1] = their bounds
    (seg[-1] = the total kept).  sym_c / idx_c are flat and as long as the input: what lies past seg[-1] is unwritten.  ``sym`` None:
    indexes and segments only (None comes back for sym_c)."""
    idx, nstreams, per, rows, scratch = _skip_args(idx, nstreams, skip_rows, "skip_compact")
    if sym is not None:
        sym = _dev(sym, torch.int32)
        if sym.numel() != idx.numel():
            raise ValueError("skip_compact: symbols and indexes hold the same number of elements")
    sym_c = torch.empty((idx.numel(),), device=idx.device, dtype=torch.int32) if sym is not None else None
    idx_c = torch.empty((idx.numel(),), device=idx.device, dtype=torch.int32)
    seg = torch.empty((nstreams + 1,), device=idx.device, dtype=torch.int64)
    _lib.check(_lib.lib().basic_skip_compact_dev(sym.data_ptr() if sym is not None else None, idx.data_ptr(), nstreams, per, rows,
                                                 scratch.data_ptr(), sym_c.data_ptr() if sym_c is not None else None, idx_c.data_ptr(),
                                                 seg.data_ptr(), _stream()))
    return sym_c, idx_c, seg


def skip_expand(sym_compact, idx, nstreams, skip_rows):
    """basic_skip_expand_dev: int32 symbols shaped like the dense ``idx`` -- the j-th element with idx >= skip_rows of stream s
    receives the j-th of the stream's run in ``sym_compact`` (the runs back to back, as skip_compact writes them), every other 0."""
    idx, nstreams, per, rows, scratch = _skip_args(idx, nstreams, skip_rows, "skip_expand")
    sym_compact = _dev(sym_compact, torch.int32)
    if sym_compact.numel() == 0:   # everything skipped and an empty tensor given: the C ABI still wants a valid pointer
        sym_compact = torch.zeros((1,), device=idx.device, dtype=torch.int32)
    out = torch.empty(idx.shape, device=idx.device, dtype=torch.int32)
    _lib.check(_lib.lib().basic_skip_expand_dev(sym_compact.data_ptr(), idx.data_ptr(), nstreams, per, rows, scratch.data_ptr(),
                                                out.data_ptr(), _stream()))
    return out


def eb_quantize_index(z, medians):
    z, medians = _dev(z, torch.float32), _dev(medians, torch.float32)
    B, C = z.shape[0], z.shape[1]
    hw = z.numel() // (B * C)
    sym = torch.empty(z.shape, device=z.device, dtype=torch.int32)
    idx = torch.empty(z.shape, device=z.device, dtype=torch.int32)
    zhat = torch.empty_like(z)
    _lib.check(_lib.lib().basic_eb_quantize_index_dev(z.data_ptr(), medians.data_ptr(), B, C, hw, sym.data_ptr(), idx.data_ptr(),
                                                      zhat.data_ptr(), _stream()))
    return sym, idx, zhat


def eb_dequantize(sym, medians):
    sym, medians = _dev(sym, torch.int32), _dev(medians, torch.float32)
    B, C = sym.shape[0], sym.shape[1]
    hw = sym.numel() // (B * C)
    zhat = torch.empty(sym.shape, device=sym.device, dtype=torch.float32)
    _lib.check(_lib.lib().basic_eb_dequantize_dev(sym.data_ptr(), medians.data_ptr(), B, C, hw, zhat.data_ptr(), _stream()))
    return zhat


def i32_to_f32(sym):
    sym = _dev(sym, torch.int32)
    out = torch.empty(sym.shape, device=sym.device, dtype=torch.float32)
    _lib.check(_lib.lib().basic_i32_to_f32_dev(sym.data_ptr(), sym.numel(), out.data_ptr(), _stream()))
    return out


def mse_per_image(a, b):
    a, b = _dev(a, torch.float32), _dev(b, torch.float32)
    out = torch.empty((a.shape[0],), device=a.device, dtype=torch.float32)
    _lib.check(_lib.lib().basic_mse_per_image_dev(a.data_ptr(), b.data_ptr(), a.shape[0], a.numel() // a.shape[0], out.data_ptr(), _stream()))
    return out


def ms_ssim_per_image(x, y, data_range=1.0, return_terms=False, workspace=None):
    """MS-SSIM of each image of two [B, C, H, W] batches (basic_msssim_per_image_dev): [B], and with ``return_terms`` also the
    [B, C, 5] terms before the weights (relu(cs) of scales 0-3, relu(ssim) of scale 4).  Inputs are made fp32 and contiguous;
    the workspace is a ``torch.empty`` on their device (or ``workspace``, a uint8 tensor there); the call runs on the
    current stream."""
    if not (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor)) or x.dim() != 4 or x.shape != y.shape:
        raise ValueError("ms_ssim_per_image takes two [B, C, H, W] tensors of one shape")
    x, y = _dev(x).float().contiguous(), _dev(y).float().contiguous()
    if y.device != x.device:
        raise ValueError("ms_ssim_per_image: the two batches live on different devices")
    B, C, H, W = x.shape
    L = _lib.lib()
    with torch.cuda.device(x.device):
        need = L.basic_msssim_workspace_bytes(B, C, H, W)
        if workspace is None and need > 0:
            workspace = torch.empty((need,), device=x.device, dtype=torch.uint8)
        out = torch.empty((B,), device=x.device, dtype=torch.float32)
        terms = torch.empty((B, C, 5), device=x.device, dtype=torch.float32) if return_terms else None
        # a refused shape (need == -1) goes to the library all the same: the message is its own
        _lib.check(L.basic_msssim_per_image_dev(x.data_ptr(), y.data_ptr(), B, C, H, W, float(data_range), _lib.ptr(workspace),
                                                workspace.numel() * workspace.element_size() if workspace is not None else 0,
                                                out.data_ptr(), _lib.ptr(terms), _stream()))
    return (out, terms) if return_terms else out


def gauss_nll_per_image(q, scales_or_params, interleaved, scale_bound=0.11, likelihood_bound=1e-9, steps=None):
    """Rate estimate (nats per image) of a Gaussian-coded latent; see basic_gauss_nll_per_image_dev.  ``steps`` (zero-mean mode
    only; see qsteps_tensor): q holds the symbols rint(y / step), rated under max(scale, bound) / step
    (basic_gauss_nll_per_image_q_dev)."""
    q, sp = _dev(q, torch.float32), _dev(scales_or_params, torch.float32)
    B, C = q.shape[0], q.shape[1]
    hw = q.numel() // (B * C)
    out = torch.empty((B,), device=q.device, dtype=torch.float32)
    if steps is not None:
        if interleaved:
            raise ValueError("gauss_nll_per_image: steps= goes with the zero-mean mode (interleaved=False) only")
        steps = qsteps_tensor(steps, B, q.device)
        _lib.check(_lib.lib().basic_gauss_nll_per_image_q_dev(q.data_ptr(), sp.data_ptr(), B, C, hw, steps.data_ptr(), steps.numel(),
                                                              float(scale_bound), float(likelihood_bound), out.data_ptr(), _stream()))
        return out
    mode = 2 if interleaved == "round_residual" else int(bool(interleaved))
    _lib.check(_lib.lib().basic_gauss_nll_per_image_dev(q.data_ptr(), sp.data_ptr(), B, C, hw, mode, float(scale_bound),
                                                        float(likelihood_bound), out.data_ptr(), _stream()))
    return out


def eb_nll_per_image(zq, coef, likelihood_bound=1e-9):
    zq, coef = _dev(zq, torch.float32), _dev(coef, torch.float32)
    B, C = zq.shape[0], zq.shape[1]
    hw = zq.numel() // (B * C)
    out = torch.empty((B,), device=zq.device, dtype=torch.float32)
    _lib.check(_lib.lib().basic_eb_nll_per_image_dev(zq.data_ptr(), coef.data_ptr(), B, C, hw, float(likelihood_bound), out.data_ptr(), _stream()))
    return out


def frame_streams(host_words, word_off, shape_hw) -> bytes:
    """write_body (compressai_coder.py:75-84) for one stream per image, done by the C helper."""
    host_words = np.ascontiguousarray(host_words, dtype=np.uint32)
    word_off = np.ascontiguousarray(word_off, dtype=np.int64)
    n = len(word_off) - 1
    cap = 12 + 4 * n + 4 * int(word_off[-1] - word_off[0])
    out = np.empty(cap, dtype=np.uint8)
    out_len = ctypes.c_int64()
    _lib.check(_lib.lib().basic_frame_streams(host_words.ctypes.data, word_off.ctypes.data, n, int(shape_hw[0]), int(shape_hw[1]),
                                              out.ctypes.data, cap, ctypes.byref(out_len)))
    return out[: out_len.value].tobytes()


def frame_streams_size(word_off) -> int:
    """Bytes frame_streams() writes for these streams."""
    n = len(word_off) - 1
    return 12 + 4 * n + 4 * int(word_off[-1] - word_off[0])


def frame_streams_into(host_words, word_off, shape_hw, address: int, capacity: int) -> int:
    """frame_streams() straight into caller memory (e.g. the final bytes object of a codec): returns the length."""
    host_words = np.ascontiguousarray(host_words, dtype=np.uint32)
    word_off = np.ascontiguousarray(word_off, dtype=np.int64)
    out_len = ctypes.c_int64()
    _lib.check(_lib.lib().basic_frame_streams(host_words.ctypes.data, word_off.ctypes.data, len(word_off) - 1, int(shape_hw[0]),
                                              int(shape_hw[1]), address, capacity, ctypes.byref(out_len)))
    return out_len.value


def frame_header(data: bytes):
    """(h, w, n streams) of a framed body."""
    buf = np.frombuffer(data, dtype=np.uint8)
    h, w, n = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
    _lib.check(_lib.lib().basic_unframe_streams(buf.ctypes.data, len(data), ctypes.byref(h), ctypes.byref(w), ctypes.byref(n),
                                                None, 0, None))
    return h.value, w.value, n.value


def unframe_streams(data: bytes, out=None):
    """read_body (compressai_coder.py:63-72) for one stream per image: (uint32 words, word offsets, (h, w)).
    ``out``: optional uint32 array of at least (len(data) - 12 - 4 n) / 4 words to receive the payloads."""
    buf = np.frombuffer(data, dtype=np.uint8)
    h, w, n = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
    _lib.check(_lib.lib().basic_unframe_streams(buf.ctypes.data, len(data), ctypes.byref(h), ctypes.byref(w), ctypes.byref(n),
                                                None, 0, None))
    word_off = np.empty(n.value + 1, dtype=np.int64)
    payload = max((len(data) - 12 - 4 * n.value) // 4, 0)
    words = out if out is not None and payload > 0 and out.size >= payload else np.empty(max(payload, 1), dtype=np.uint32)
    _lib.check(_lib.lib().basic_unframe_streams(buf.ctypes.data, len(data), ctypes.byref(h), ctypes.byref(w), ctypes.byref(n),
                                                word_off.ctypes.data, n.value, words.ctypes.data))
    return words[: int(word_off[-1])], word_off, (h.value, w.value)


IMAGE_LAYOUTS = {"chw": _lib.IMAGE_CHW, "hwc": _lib.IMAGE_HWC}   # BASIC_IMAGE_*


def image_layout_of(t):
    """The memory order of a ``[B, C, H, W]`` tensor, from its shape and strides alone: ``"chw"`` when it is contiguous,
    ``"hwc"`` when its memory is ``[B][H][W][C]`` (``torch.channels_last``, or what ``torch.from_numpy(a).permute(2, 0, 1)[None]``
    gives for a decoder's array), ``None`` for anything else (the caller then makes it contiguous).  A dimension of size 1 fits
    any stride; with one channel both readings hold and ``"chw"`` is returned."""
    if t.dim() != 4:
        return None
    shape, stride = tuple(t.shape), tuple(t.stride())
    if 0 in shape:
        return None
    B, C, H, W = shape
    for name, want in (("chw", (C * H * W, H * W, W, 1)), ("hwc", (H * W * C, 1, W * C, C))):
        if all(n == 1 or s == e for n, s, e in zip(shape, stride, want)):
            return name
    return None


def _image_u8(t):
    """(tensor, layout name) of a uint8 [B, C, H, W] tensor as the library reads it: as it lies, or made contiguous."""
    if t.dim() != 4:
        raise ValueError(f"an image batch is [B, C, H, W], not {tuple(t.shape)}")
    layout = image_layout_of(t)
    if layout is None:
        t, layout = t.contiguous(), "chw"
    return t, layout


def image_u8_to_f32(t):
    """uint8 [B, C, H, W] on the GPU, contiguous or with [B][H][W][C] memory (image_layout_of) -> float32 [B, C, H, W],
    ``t.float().div(255)`` exactly (basic_image_u8_to_f32_dev)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        _dev(t)
    if t.dtype != torch.uint8:
        raise TypeError(f"expected torch.uint8, got {t.dtype}")
    t, layout = _image_u8(t)
    B, C, H, W = t.shape
    with torch.cuda.device(t.device):
        out = torch.empty((B, C, H, W), device=t.device, dtype=torch.float32)
        _lib.check(_lib.lib().basic_image_u8_to_f32_dev(t.data_ptr(), IMAGE_LAYOUTS[layout], B, C, H, W, out.data_ptr(), _stream()))
    return out


def image_f32_to_u8(t, layout="chw"):
    """float32 [B, C, H, W] on the GPU -> uint8 [B, C, H, W]: ``torch.nan_to_num(t, nan=0.0).clamp(0, 1).mul(255).round()``
    as bytes (basic_image_f32_to_u8_dev).  layout "hwc": the result's memory is [B][H][W][C] (a permuted view, ready for an
    image encoder after ``.permute(0, 2, 3, 1)``)."""
    if layout not in IMAGE_LAYOUTS:
        raise ValueError(f"layout is 'chw' or 'hwc', not {layout!r}")
    t = _dev(t, torch.float32)
    if t.dim() != 4:
        raise ValueError(f"an image batch is [B, C, H, W], not {tuple(t.shape)}")
    B, C, H, W = t.shape
    with torch.cuda.device(t.device):
        if layout == "hwc":
            out = torch.empty((B, H, W, C), device=t.device, dtype=torch.uint8).permute(0, 3, 1, 2)
        else:
            out = torch.empty((B, C, H, W), device=t.device, dtype=torch.uint8)
        _lib.check(_lib.lib().basic_image_f32_to_u8_dev(t.data_ptr(), B, C, H, W, IMAGE_LAYOUTS[layout], out.data_ptr(), _stream()))
    return out


def image_tiles_last_path():
    """0 (sample by sample) or 1 (wide) for the calling thread's last tiles call; -1 before any (basic_image_tiles_last_path)."""
    p = ctypes.c_int(-1)
    _lib.check(_lib.lib().basic_image_tiles_last_path(ctypes.byref(p)))
    return p.value


def _tiles_picture(img):
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        _dev(img)
    if img.dtype != torch.uint8:
        raise TypeError(f"expected torch.uint8, got {img.dtype}")
    if img.dim() != 4 or img.shape[0] != 1:
        raise ValueError(f"a picture is [1, C, H, W], not {tuple(img.shape)}")


def image_tiles_to_f32(img_u8, group):
    """The tiles of ``group`` -- ``(y0, x0, step_y, step_x, ny, nx, h, w, ...)``, a utils.tiling.TileGroup -- cut out of the uint8
    picture ``[1, C, H, W]`` on the GPU: float32 ``[ny * nx, C, h, w]``, tile i * nx + j equal to
    ``img[..., y:y + h, x:x + w].float().div(255)`` at its origin, in one launch (basic_image_tiles_u8_to_f32_dev; a group whose steps
    are smaller than its tiles, overlapped tiles, goes to basic_image_tiles_overlap_u8_to_f32_dev).  The picture is read as it lies
    when it is contiguous or its memory is [H][W][C] (image_layout_of), and made contiguous otherwise."""
    _tiles_picture(img_u8)
    y0, x0, step_y, step_x, ny, nx, h, w = (int(v) for v in tuple(group)[:8])
    img, layout = _image_u8(img_u8)
    _, C, H, W = img.shape
    if min(ny, nx, h, w) < 1:
        raise ValueError(f"a tile group has positive ny, nx, h and w, not {(ny, nx, h, w)}")
    with torch.cuda.device(img.device):
        out = torch.empty((ny * nx, C, h, w), device=img.device, dtype=torch.float32)
        L = _lib.lib()
        cut = L.basic_image_tiles_overlap_u8_to_f32_dev if (1 <= step_y < h or 1 <= step_x < w) else L.basic_image_tiles_u8_to_f32_dev
        _lib.check(cut(img.data_ptr(), IMAGE_LAYOUTS[layout], C, H, W, y0, x0, step_y, step_x, ny, nx, h, w, out.data_ptr(), _stream()))
    return out


def image_tiles_from_f32(batch, canvas_u8, group):
    """The way back: the top-left h x w of every ``[C, sh, sw]`` reconstruction of ``batch`` (float32 ``[ny * nx, C, sh, sw]`` on the
    GPU) as bytes (image_f32_to_u8's values) at its tile's place in ``canvas_u8``, a uint8 ``[1, C, H, W]`` picture on the same GPU
    that is contiguous or has [H][W][C] memory; one launch (basic_image_tiles_f32_to_u8_dev).  Bytes outside the tiles keep their
    value.  Returns the canvas."""
    _tiles_picture(canvas_u8)
    batch = _dev(batch, torch.float32)
    y0, x0, step_y, step_x, ny, nx, h, w = (int(v) for v in tuple(group)[:8])
    layout = image_layout_of(canvas_u8)
    if layout is None:
        raise ValueError("the canvas must be contiguous or have [H][W][C] memory: the tiles are written into it in place")
    _, C, H, W = canvas_u8.shape
    if batch.dim() != 4 or batch.shape[0] != ny * nx or batch.shape[1] != C:
        raise ValueError(f"{ny} x {nx} tiles of {C} channels need a [{ny * nx}, {C}, sh, sw] batch, not {tuple(batch.shape)}")
    if batch.device != canvas_u8.device:
        raise ValueError("image_tiles_from_f32: the batch and the canvas live on different devices")
    with torch.cuda.device(batch.device):
        _lib.check(_lib.lib().basic_image_tiles_f32_to_u8_dev(batch.data_ptr(), batch.shape[2], batch.shape[3], C, y0, x0, step_y, step_x,
                                                              ny, nx, h, w, canvas_u8.data_ptr(), IMAGE_LAYOUTS[layout], H, W, _stream()))
    return canvas_u8


def image_tiles_blend(sources, grid, out, region=None):
    """The picture of overlapped tiles, seams cross-faded, in ONE launch (basic_image_tiles_blend_dev; the values are defined in
    include/basic_hip.h section 8c).  ``sources``: a list of ``(batch, tile_indices)``, batch float32 ``[n, C, sh, sw]`` on the GPU --
    the reconstructions as decode() left them, any sh x sw that holds the tiles -- and the n row-major tile numbers of ``grid``, a
    utils.tiling.TileGrid, they belong to.  ``out``: uint8 or float32 ``[1, C, rh, rw]`` on the same GPU, contiguous or with [H][W][C]
    memory, the rectangle ``region = (y0, x0, y1, x1)`` of the picture (default: all of it); every sample of it is written.
    ValueError when the rectangle needs a tile nobody supplied.  The batches are read in place: keep them alive (and unchanged)
    until the launch has run.  Returns ``out``."""
    if not isinstance(out, torch.Tensor) or not out.is_cuda:
        _dev(out)
    if out.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"the output is torch.uint8 or torch.float32, not {out.dtype}")
    y0, x0, y1, x1 = (0, 0, grid.H, grid.W) if region is None else (int(v) for v in region)
    if not (0 <= y0 < y1 <= grid.H and 0 <= x0 < x1 <= grid.W):
        raise ValueError(f"region {(y0, x0, y1, x1)} is empty or leaves the {grid.H} x {grid.W} picture")
    if out.dim() != 4 or out.shape[0] != 1 or tuple(out.shape[2:]) != (y1 - y0, x1 - x0):
        raise ValueError(f"the output of region {(y0, x0, y1, x1)} is [1, C, {y1 - y0}, {x1 - x0}], not {tuple(out.shape)}")
    layout = image_layout_of(out)
    if layout is None:
        raise ValueError("the output must be contiguous or have [H][W][C] memory: it is written in place")
    C = out.shape[1]
    table = np.zeros(len(grid), dtype=np.dtype([("src", "<u8"), ("sh", "<i4"), ("sw", "<i4")]))   # basic_tile_source
    keep = []   # a batch that had to be made contiguous lives until the launch is enqueued (the allocator is stream-ordered)
    for batch, indices in sources:
        batch = _dev(batch, torch.float32)
        keep.append(batch)
        indices = [int(k) for k in indices]
        if batch.dim() != 4 or batch.shape[0] != len(indices) or batch.shape[1] != C:
            raise ValueError(f"{len(indices)} tiles of {C} channels need a [{len(indices)}, {C}, sh, sw] batch, not {tuple(batch.shape)}")
        if batch.device != out.device:
            raise ValueError("image_tiles_blend: a batch and the output live on different devices")
        sh, sw = int(batch.shape[2]), int(batch.shape[3])
        for n, k in enumerate(indices):
            _, _, h, w = grid.tile_rect(k)
            if sh < h or sw < w:
                raise ValueError(f"tile {k} is {h} x {w}; its reconstruction is {sh} x {sw}")
            table[k] = (batch.data_ptr() + 4 * n * C * sh * sw, sh, sw)
    missing = [k for g in grid.tiles_of_region(y0, x0, y1, x1) for k in g.indices if not table["src"][k]]
    if missing:
        raise ValueError(f"region {(y0, x0, y1, x1)} needs tiles {missing}, which no source supplies")
    with torch.cuda.device(out.device):
        d_table = torch.from_numpy(table.view(np.uint8)).to(out.device)
        _lib.check(_lib.lib().basic_image_tiles_blend_dev(d_table.data_ptr(), grid.H, grid.W, grid.th, grid.tw, grid.oy, grid.ox, C, y0, x0,
                                                          y1 - y0, x1 - x0, out.data_ptr(), _lib.PIXEL_U8 if out.dtype == torch.uint8 else
                                                          _lib.PIXEL_F32, IMAGE_LAYOUTS[layout], _stream()))
    del keep
    return out


_TILE_REF = np.dtype([("img", "<u8"), ("img_h", "<i4"), ("img_w", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("layout", "<i4"), ("pad", "<i4")])   # basic_tile_ref


def _tile_ref_table(pictures, refs, device):
    """The host table of ``refs`` -- ``(picture, tile index, y0, x0)`` rows, utils.tiling.PooledTile -- over ``pictures``, ``{index: (tensor as the
    library reads it, layout name)}``, and its device workspace."""
    rows = {p: (img.data_ptr(), img.shape[2], img.shape[3], IMAGE_LAYOUTS[layout]) for p, (img, layout) in pictures.items()}
    table = np.zeros(len(refs), dtype=_TILE_REF)
    for k, field in enumerate(("img", "img_h", "img_w", "layout")):   # column by column: a row per tile, a picture's values repeated
        table[field] = [rows[int(ref[0])][k] for ref in refs]
    table["y0"], table["x0"] = [int(ref[2]) for ref in refs], [int(ref[3]) for ref in refs]
    return table, torch.empty(len(refs) * _TILE_REF.itemsize, dtype=torch.uint8, device=device)


def image_tiles_gather(pictures, refs, h, w, pad=False):
    """Tiles of MANY pictures in one launch (basic_image_tiles_gather_u8_to_f32_dev, include/basic_hip.h section 8d).  ``pictures``: uint8
    ``[1, C, H, W]`` tensors on one GPU, of any sizes with one C, each read as it lies when it is contiguous or its memory is [H][W][C]
    (image_layout_of) and made contiguous otherwise; ``refs``: one ``(picture, tile index, y0, x0)`` per tile (utils.tiling.pool_tiles),
    ``picture`` an index into ``pictures``.  Returns float32 ``[len(refs), C, h, w]``, tile t equal to
    ``pictures[p][..., y0:y0 + h, x0:x0 + w].float().div(255)``: what image_tiles_to_f32 gives for that picture and origin.
    ``pad=True`` (basic_image_tiles_gather_pad_u8_to_f32_dev): a tile may leave its picture at the bottom and right -- its origin may
    not -- and sample (r, q) of it is the picture's ``[min(y0 + r, H - 1), min(x0 + q, W - 1)]``: the last row and column replicated."""
    refs = list(refs)
    if not refs:
        raise ValueError("image_tiles_gather: no tiles")
    used = sorted({int(r[0]) for r in refs})
    lie = {}
    for p in used:
        _tiles_picture(pictures[p])
        lie[p] = _image_u8(pictures[p])
    first = lie[used[0]][0]
    C = first.shape[1]
    if any(t.shape[1] != C or t.device != first.device for t, _ in lie.values()):
        raise ValueError("image_tiles_gather: the pictures share one channel count and one device")
    with torch.cuda.device(first.device):
        table, ws = _tile_ref_table(lie, refs, first.device)
        out = torch.empty((len(refs), C, int(h), int(w)), device=first.device, dtype=torch.float32)
        L = _lib.lib()
        gather = L.basic_image_tiles_gather_pad_u8_to_f32_dev if pad else L.basic_image_tiles_gather_u8_to_f32_dev
        _lib.check(gather(table.ctypes.data, len(refs), C, int(h), int(w), ws.data_ptr(), out.data_ptr(), _stream()))
    del lie, ws   # enqueued: the allocator is stream-ordered
    return out


def image_tiles_scatter(batch, canvases, refs, h, w, clip=False):
    """The way back (basic_image_tiles_scatter_f32_to_u8_dev): the top-left h x w of reconstruction t of ``batch`` (float32
    ``[len(refs), C, sh, sw]`` on the GPU) as bytes (image_f32_to_u8's values) at ``(y0, x0)`` of ``canvases[picture]`` of ``refs[t]``; the
    canvases are uint8 ``[1, C, H, W]`` on the same GPU, contiguous or with [H][W][C] memory, and are written in place, bytes outside
    the tiles keeping their value.  Tiles of one call must not intersect in a canvas.  One launch.  ``clip=True``
    (basic_image_tiles_scatter_clip_f32_to_u8_dev): a tile may leave its canvas at the bottom and right -- its origin may not -- and only
    the part of its h x w inside the canvas is written."""
    refs = list(refs)
    if not refs:
        raise ValueError("image_tiles_scatter: no tiles")
    batch = _dev(batch, torch.float32)
    if batch.dim() != 4 or batch.shape[0] != len(refs):
        raise ValueError(f"{len(refs)} tiles need a [{len(refs)}, C, sh, sw] batch, not {tuple(batch.shape)}")
    C = batch.shape[1]
    lie = {}
    for p in sorted({int(r[0]) for r in refs}):
        canvas = canvases[p]
        _tiles_picture(canvas)
        layout = image_layout_of(canvas)
        if layout is None:
            raise ValueError("a canvas must be contiguous or have [H][W][C] memory: the tiles are written into it in place")
        if canvas.shape[1] != C or canvas.device != batch.device:
            raise ValueError(f"image_tiles_scatter: canvas {p} is not a {C}-channel picture on the batch's device")
        lie[p] = (canvas, layout)
    with torch.cuda.device(batch.device):
        table, ws = _tile_ref_table(lie, refs, batch.device)
        L = _lib.lib()
        scatter = L.basic_image_tiles_scatter_clip_f32_to_u8_dev if clip else L.basic_image_tiles_scatter_f32_to_u8_dev
        _lib.check(scatter(batch.data_ptr(), batch.shape[2], batch.shape[3], C, int(h), int(w), table.ctypes.data, len(refs), ws.data_ptr(),
                           _stream()))
    del ws
    return canvases


def image_sse_u8(a, b):
    """The exact sum of squared differences of two uint8 [B, C, H, W] batches on one GPU, per image and channel: int64 [B, C]
    on that device (basic_image_sse_u8_dev; integer arithmetic, the same value at any batch, layout and alignment).  Each batch is
    read as it lies when it is contiguous or its memory is [B][H][W][C] (image_layout_of), and made contiguous otherwise."""
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            _dev(t)
        if t.dtype != torch.uint8:
            raise TypeError(f"expected torch.uint8, got {t.dtype}")
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f"image_sse_u8 takes two [B, C, H, W] batches of one shape, not {tuple(a.shape)} and {tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError("image_sse_u8: the two batches live on different devices")
    (a, layout_a), (b, layout_b) = _image_u8(a), _image_u8(b)
    B, C, H, W = a.shape
    with torch.cuda.device(a.device):
        out = torch.empty((B, C), device=a.device, dtype=torch.int64)
        _lib.check(_lib.lib().basic_image_sse_u8_dev(a.data_ptr(), IMAGE_LAYOUTS[layout_a], b.data_ptr(), IMAGE_LAYOUTS[layout_b], B, C, H, W,
                                                     out.data_ptr(), _stream()))
    return out


def ms_ssim_per_image_u8(a, b, return_terms=False):
    """MS-SSIM of each image of two uint8 [B, C, H, W] batches, BY DEFINITION
    ``ms_ssim_per_image(image_u8_to_f32(a), image_u8_to_f32(b), data_range=1.0)``, and computed as exactly that: two conversions in
    front of the float kernels.  This is a decision, not a measurement: the conversions move a small fraction of the bytes the ten
    MS-SSIM launches move, and a uint8 load phase in csrc/msssim.hip would double its instantiations; what the two extra passes cost
    was not measured."""
    return ms_ssim_per_image(image_u8_to_f32(a), image_u8_to_f32(b), data_range=1.0, return_terms=return_terms)


class HyperpriorSession:
    """basic_hp_session_*: the fused compress / decompress entry points of the two hyperprior latent graphs (one C call
    per batch instead of a Python walk over the graph): an ``h_s`` that ends in the latent's channels is the scale hyperprior, one
    that ends in twice as many (scales, then means) the mean-scale hyperprior.  Borrows the layer plans and table sets it is
    given (kept alive here); one session serves one call at a time."""

    def __init__(self, g_a, h_a, h_s, g_s, eb_medians, z_tables, scale_table, scale_bound, y_tables):
        self._keep = (list(g_a), list(h_a), list(h_s), list(g_s), z_tables, y_tables)
        arrs = []
        for plans in self._keep[:4]:
            a = (ctypes.c_void_p * len(plans))(*[p._h for p in plans])
            arrs.append(a)
        med = np.ascontiguousarray(eb_medians.detach().cpu().numpy() if isinstance(eb_medians, torch.Tensor) else eb_medians, dtype=np.float32)
        tab = np.ascontiguousarray(scale_table.detach().cpu().numpy() if isinstance(scale_table, torch.Tensor) else scale_table, dtype=np.float32)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().basic_hp_session_create(arrs[0], len(g_a), arrs[1], len(h_a), arrs[2], len(h_s), arrs[3], len(g_s),
                                                      med.ctypes.data, med.size, z_tables._h, tab.ctypes.data, tab.size,
                                                      float(scale_bound), y_tables._h, ctypes.byref(h)))
        self._h = h
        self.key = tuple(p._h.value for plans in self._keep[:4] for p in plans) + (z_tables._h.value, y_tables._h.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().basic_hp_session_destroy(h)
            except Exception:
                pass

    def set_rans_waves(self, waves_per_block):
        _lib.check(_lib.lib().basic_hp_session_set_rans_waves(self._h, int(waves_per_block)))

    def set_stream_lanes(self, lanes):
        """y streams per image (basic_hp_session_set_stream_lanes): 1 is the reference's format."""
        _lib.check(_lib.lib().basic_hp_session_set_stream_lanes(self._h, int(lanes)))

    def set_qsteps(self, steps):
        """Quantiser steps of the y latent for the calls that follow (basic_hp_session_set_qsteps): a number or a sequence of
        one step per image, validated on the host (ValueError); None clears them -- the session then launches what it always did."""
        if steps is None:
            _lib.check(_lib.lib().basic_hp_session_set_qsteps(self._h, None, 0))
            return
        from ..utils.qstep import check_qsteps
        steps = check_qsteps(steps)
        _lib.check(_lib.lib().basic_hp_session_set_qsteps(self._h, steps.ctypes.data, int(steps.size)))

    def set_skip_rows(self, rows):
        """Skip coding of the y latent for the calls that follow (basic_hp_session_set_skip_rows): elements whose table row is below
        ``rows`` are not coded; 0 / None is the format without it.  Refused (BasicHipError) while rate targets are set."""
        _lib.check(_lib.lib().basic_hp_session_set_skip_rows(self._h, int(rows or 0)))

    def set_rate_targets(self, budgets, candidates=None, passes=2):
        """Byte budgets of the payloads of the calls that follow (basic_hp_session_set_rate_targets): a number or one per image;
        ``candidates``: the first grid (utils/rate.py first_grid() by default), ``passes`` in [1, 3].  Validated on the host
        (ValueError).  None clears them -- the session then launches what it always did."""
        if budgets is None:
            _lib.check(_lib.lib().basic_hp_session_set_rate_targets(self._h, None, 0, None, 0, 0))
            return
        from ..utils.rate import check_budgets, check_candidates, check_passes, first_grid
        b = check_budgets(budgets)
        c = first_grid() if candidates is None else check_candidates(candidates)
        _lib.check(_lib.lib().basic_hp_session_set_rate_targets(self._h, b.ctypes.data, int(b.size), c.ctypes.data, int(c.size),
                                                                check_passes(passes)))

    def rate_result(self, batch):
        """The last rate-controlled encode's (steps float32 [B], predicted payload bytes int64 [B], choice words int32 [B])."""
        steps, pred, flags = np.zeros(batch, np.float32), np.zeros(batch, np.int64), np.zeros(batch, np.int32)
        _lib.check(_lib.lib().basic_hp_session_rate_result(self._h, steps.ctypes.data, pred.ctypes.data, flags.ctypes.data, int(batch)))
        return steps, pred, flags

    def set_transform_token(self, enable):
        """False / 0: no ordering; True / 1: the transform phases of all sessions one at a time; 2: two at a time."""
        _lib.check(_lib.lib().basic_hp_session_set_transform_token(self._h, int(enable)))

    def encode(self, x) -> bytes:
        """x: float32 or uint8 [B, C, H, W], on the GPU or on the host (uploaded inside the call; pinned memory goes at DMA rate).
        A uint8 batch is read as it lies when it is contiguous or its memory is [B][H][W][C] (image_layout_of), uploaded as
        bytes and converted on the device: the bytes written are those of ``x.float().div(255)``."""
        if x.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"expected float32 or uint8, got {x.dtype}")
        n = ctypes.c_int64()
        if x.dtype == torch.uint8:
            x, layout = _image_u8(x)
            B, C, H, W = x.shape
            if C != self._keep[0][0].cin:
                raise ValueError(f"the analysis transform expects {self._keep[0][0].cin} input channels, got {C}")
            _lib.check(_lib.lib().basic_hp_encode_images_u8(self._h, x.data_ptr(), 0 if x.is_cuda else 1, IMAGE_LAYOUTS[layout], B, H, W,
                                                            None, 0, ctypes.byref(n), _stream()))
        else:
            x = x.contiguous()
            B, C, H, W = x.shape
            _lib.check(_lib.lib().basic_hp_encode_images(self._h, x.data_ptr(), 0 if x.is_cuda else 1, B, H, W, None, 0, ctypes.byref(n), _stream()))
        # the final bytes object is allocated once at its exact size and the streams are framed straight into it
        api = ctypes.pythonapi
        api.PyBytes_FromStringAndSize.restype, api.PyBytes_FromStringAndSize.argtypes = ctypes.py_object, [ctypes.c_char_p, ctypes.c_ssize_t]
        api.PyBytes_AsString.restype, api.PyBytes_AsString.argtypes = ctypes.c_void_p, [ctypes.py_object]
        out = api.PyBytes_FromStringAndSize(None, n.value)
        _lib.check(_lib.lib().basic_hp_encode_result(self._h, api.PyBytes_AsString(out), n.value, None))
        return out

    def decode(self, data, device=None, output_dtype=torch.float32, out=None):
        """The reconstruction [B, C, H, W] on the GPU: float32 (the un-clamped output of g_s), or with
        ``output_dtype=torch.uint8`` the picture, ``clamp(0, 1).mul(255).round()`` of it converted on the device.
        ``out`` (uint8 only): a uint8 [B, C, H, W] tensor to fill instead, contiguous or with [B][H][W][C] memory, on the GPU or
        on the host (the bytes are then copied inside the call, one per sample; it returns with them in place)."""
        if output_dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"output_dtype is torch.float32 or torch.uint8, not {output_dtype}")
        if out is not None and output_dtype != torch.uint8:
            raise TypeError("out= takes a uint8 tensor and output_dtype=torch.uint8")
        buf = np.frombuffer(data, dtype=np.uint8)
        b, c, h, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.lib().basic_hp_decoded_shape(self._h, buf.ctypes.data, buf.size, ctypes.byref(b), ctypes.byref(c),
                                                     ctypes.byref(h), ctypes.byref(w)))
        shape = (b.value, c.value, h.value, w.value)
        if out is None:
            out = torch.empty(shape, device=device or torch.device("cuda", torch.cuda.current_device()), dtype=output_dtype)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or image_layout_of(out) is None:
            raise ValueError(f"out= must be a uint8 tensor of shape {shape} with [B][C][H][W] or [B][H][W][C] memory")
        if output_dtype == torch.uint8:
            _lib.check(_lib.lib().basic_hp_decode_images_u8(self._h, buf.ctypes.data, buf.size, IMAGE_LAYOUTS[image_layout_of(out)],
                                                            out.data_ptr(), 0 if out.is_cuda else 1, out.numel(), _stream()))
        else:
            _lib.check(_lib.lib().basic_hp_decode_images(self._h, buf.ctypes.data, buf.size, out.data_ptr(), out.numel(), _stream()))
        return out


SCAN_KERNELS = ("generic", "pipelined", "batched", "wavefront", "band")   # BASIC_SCAN_KERNEL_*
SCAN_SCHEDULES = ("auto", "raster", "wavefront", "band")                  # BASIC_SCAN_SCHEDULE_*


def wavefront_schedule(h, w, ksize):
    """The wavefront encode schedule of an h x w latent with a causal ksize x ksize window, as the kernel walks it
    (csrc/scanline.hip): row r runs s = ksize // 2 + 2 columns behind row r - 1, so step t codes column t - s * r of every
    row for which that lies in [0, w).  -> (steps, table): steps = w + s * (h - 1); table[t][r] = the column row r codes
    in step t, or None where the row is idle (it then stands for the zero padding left and right of the image)."""
    s = ksize // 2 + 2
    steps = w + s * (h - 1)
    return steps, [[t - s * r if 0 <= t - s * r < w else None for r in range(h)] for t in range(steps)]


def band_schedule(h, w, ksize, tight=False):
    """The band encode schedule of an h x w latent with a causal ksize x ksize window, as the kernel walks it (csrc/scanline.hip):
    the wavefront's steps -- row r codes column c at step t = s * r + c, s = ksize // 2 + 2 -- but an image owns only min(A, h)
    column slots; slot j codes rows j, j + A, j + 2 A, ... back to back with period A * s >= w.  At step t slot j has
    u = t - s * j, (n, c) = divmod(u, A * s) and row r = j + n * A; it is active iff u >= 0, r < h and c < w.
    A = w // s + 1 (what the kernel uses: every row is followed by an idle step of its slot), or with `tight` the smallest
    A with A * s >= w.  -> (A, steps, table): steps = w + s * (h - 1); table[t][j] = (row, col, active) for j < min(A, h), with
    row = col = None before the slot's first row (u < 0)."""
    s = ksize // 2 + 2
    A = -(-w // s) if tight else w // s + 1
    steps = w + s * (h - 1)
    table = []
    for t in range(steps):
        slots = []
        for j in range(min(A, h)):
            u = t - s * j
            if u < 0:
                slots.append((None, None, False))
                continue
            n, c = divmod(u, A * s)
            r = j + n * A
            slots.append((r, c, r < h and c < w))
        table.append(slots)
    return A, steps, table


class ScanlinePlan:
    """basic_scanline_*: the persistent scan-line AR coding loop (one launch for all H*W coding steps)."""

    def __init__(self, ctx_weight, ctx_bias, dense, prior_channels, ctx_act=False):
        """dense: list of (weight [out, in(, 1, 1)], bias or None, leaky_after: bool[, in_groups: int = 1]); in_groups = the
        input channel groups of the masked convolution the layer stands for (fixes the canonical summation blocks)."""
        dense = [tuple(d) + (1,) * (4 - len(d)) for d in dense]
        groups = np.array([int(d[3]) for d in dense], dtype=np.int32)
        dense = [d[:3] for d in dense]
        cw = _f32(ctx_weight)
        cb = _f32(ctx_bias) if ctx_bias is not None else None
        self.channels, self.ksize = cw.shape[1], cw.shape[2]
        ws = [_f32(w).reshape(w.shape[0], -1) for w, _, _ in dense]
        bs = [(_f32(b) if b is not None else None) for _, b, _ in dense]
        n = len(dense)
        wp = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
        bp = (ctypes.c_void_p * n)(*[(b.ctypes.data if b is not None else None) for b in bs])
        outs = np.array([w.shape[0] for w in ws], dtype=np.int32)
        acts = np.array([int(bool(ctx_act))] + [int(bool(a)) for _, _, a in dense], dtype=np.int32)
        # the layer sizes basic_scanline_plan_create gets: all the library's planner knows of the layers (csrc/scan_plan.h)
        self.layer_sizes = dict(channels=int(self.channels), ctx_out=int(cw.shape[0]), ksize=int(self.ksize), prior_channels=int(prior_channels),
                                dense_out=outs.tolist(), act_after=acts.tolist(), dense_in_groups=groups.tolist())
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().basic_scanline_plan_create(cw.ctypes.data, cb.ctypes.data if cb is not None else None, self.channels,
                                                         cw.shape[0], self.ksize, int(prior_channels), n, wp, bp, outs.ctypes.data,
                                                         acts.ctypes.data, groups.ctypes.data, ctypes.byref(h)))
        self._h = h
        wg, lb = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.lib().basic_scanline_plan_info(h, ctypes.byref(wg), ctypes.byref(lb)))
        self.workgroups, self.lds_weight_bytes = wg.value, lb.value

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().basic_scanline_plan_destroy(h)
            except Exception:
                pass

    def encode(self, y, prior, table):
        y, table = _dev(y, torch.float32), _dev(table, torch.float32)
        prior = _dev(prior, torch.float32) if prior is not None else None
        B, C, H, W = y.shape
        sym = torch.empty((B, H * W * C), device=y.device, dtype=torch.int32)
        idx = torch.empty((B, H * W * C), device=y.device, dtype=torch.int32)
        ybuf = torch.empty_like(y)
        _lib.check(_lib.lib().basic_scanline_encode_dev(self._h, y.data_ptr(), prior.data_ptr() if prior is not None else None, B, H, W,
                                                        table.data_ptr(), table.numel(), sym.data_ptr(), idx.data_ptr(), ybuf.data_ptr(),
                                                        _stream()))
        return sym, idx, ybuf

    def can_encode(self, batch):
        """The encoder launch needs its workgroups resident: one per compute unit."""
        return self.workgroups <= torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count

    def batched_max(self, width, decode=False):
        """Largest batch the batched persistent kernel serves for a latent `width` columns wide on this device (0: never)."""
        key = (int(width), bool(decode), torch.cuda.current_device())
        cache = self.__dict__.setdefault("_batched_max", {})
        if key not in cache:
            m = ctypes.c_int()
            _lib.check(_lib.lib().basic_scanline_batched_max(self._h, int(width), int(bool(decode)), ctypes.byref(m)))
            cache[key] = m.value
        return cache[key]

    def wavefront_max(self, height, width):
        """Largest batch the wavefront encode schedule serves for a `height` x `width` latent on this device (0: never)."""
        key = (int(height), int(width), torch.cuda.current_device())
        cache = self.__dict__.setdefault("_wavefront_max", {})
        if key not in cache:
            m = ctypes.c_int()
            _lib.check(_lib.lib().basic_scanline_wavefront_max(self._h, int(height), int(width), ctypes.byref(m)))
            cache[key] = m.value
        return cache[key]

    def band_max(self, height, width):
        """Images ONE launch of the band encode schedule codes of a `height` x `width` latent on this device; a larger batch takes
        several launches inside one call, so any batch is served when this is >= 1 (0: never)."""
        key = (int(height), int(width), torch.cuda.current_device())
        cache = self.__dict__.setdefault("_band_max", {})
        if key not in cache:
            m = ctypes.c_int()
            _lib.check(_lib.lib().basic_scanline_band_max(self._h, int(height), int(width), ctypes.byref(m)))
            cache[key] = m.value
        return cache[key]

    def band_decode_max(self, tables, height, width, lanes=1):
        """Images ONE band decode launch (row streams, `lanes` lane streams per image) decodes of a `height` x `width` latent with
        that table set on this device: the largest number whose column tiles' workgroups and decoder workgroups -- a wavefront per
        (image, slot, lane), four to a workgroup -- fit the chip together; a larger batch takes several launches inside one call
        (0: never)."""
        key = (id(tables), int(height), int(width), int(lanes), torch.cuda.current_device())
        cache = self.__dict__.setdefault("_band_decode_max", {})
        if key not in cache:
            m = ctypes.c_int()
            _lib.check(_lib.lib().basic_scanline_band_decode_max(self._h, tables._h, int(height), int(width), int(lanes), ctypes.byref(m)))
            cache[key] = (m.value, tables)   # (tables: keeps its id its own)
        return cache[key][0]

    def last_kernel(self):
        """The kernel the plan's last launch ran: "generic", "pipelined", "batched", "wavefront" or "band"; None before the first."""
        k = ctypes.c_int()
        _lib.check(_lib.lib().basic_scanline_last_kernel(self._h, ctypes.byref(k)))
        return SCAN_KERNELS[k.value] if 0 <= k.value < len(SCAN_KERNELS) else None

    def set_encode_schedule(self, schedule):
        """How encode calls are scheduled from now on: "auto", "raster" (never the wavefront or the band), "wavefront" or "band"
        (always: a call that does not fit it raises).  The coded integers do not depend on it."""
        if schedule not in SCAN_SCHEDULES:
            raise ValueError(f"encode schedule must be one of {SCAN_SCHEDULES}, not {schedule!r}")
        _lib.check(_lib.lib().basic_scanline_set_encode_schedule(self._h, SCAN_SCHEDULES.index(schedule)))

    def set_decode_schedule(self, schedule):
        """How decode calls over ROW STREAMS are scheduled from now on: "auto" (today: the raster kernels), "raster" (never the
        wavefront or the band), "wavefront" or "band" (always that launch: a call that does not fit it raises).  Decode calls
        without row streams never look at it.  The decoded integers do not depend on it."""
        if schedule not in SCAN_SCHEDULES:
            raise ValueError(f"decode schedule must be one of {SCAN_SCHEDULES}, not {schedule!r}")
        _lib.check(_lib.lib().basic_scanline_set_decode_schedule(self._h, SCAN_SCHEDULES.index(schedule)))
        self._decode_schedule = schedule

    def choose(self, batch, height, width, table_len, schedule="auto", lane_max_batch=0, tables=None, lanes=1, rows=False):
        """What an encode call (tables None) or a decode call with that table set would run for `batch` images of a `height` x
        `width` latent (0: not known), as the library's one planner decides it -- without launching: -> (kernel, launches), kernel
        one of SCAN_KERNELS, or None where the call is left to the per-step path.  `schedule` stands for the plan's encode schedule
        (BASIC_SCAN_KERNEL wins over it); batches above `lane_max_batch` are not given to the generic and pipelined kernels.  A
        forced kernel or schedule the call does not fit raises, as the launch would.  `lanes`: the lane streams per image of a decode
        call (a decoder wavefront each); `rows`: the decode call brings row streams (the wavefront or band decode launch may serve
        it: the plan's decode schedule, set_decode_schedule, holds for the answer as for the call)."""
        if schedule not in SCAN_SCHEDULES:
            raise ValueError(f"encode schedule must be one of {SCAN_SCHEDULES}, not {schedule!r}")
        # the answer depends on nothing but these, so a repeated call (every step of a stream worker) asks the library once: a
        # library call releases the interpreter lock, and with several workers each release is a chance to wait for it again
        key = (int(batch), int(height), int(width), int(table_len), schedule, int(lane_max_batch), id(tables), os.environ.get("BASIC_SCAN_KERNEL"),
               torch.cuda.current_device(), int(lanes), bool(rows), getattr(self, "_decode_schedule", "auto"))
        cache = self.__dict__.setdefault("_chosen", {})
        if key not in cache:
            k, n = ctypes.c_int(), ctypes.c_int()
            _lib.check(_lib.lib().basic_scanline_choose_rows(self._h, tables._h if tables is not None else None, int(batch), int(lanes),
                                                             int(bool(rows)), int(height), int(width), int(table_len),
                                                             SCAN_SCHEDULES.index(schedule), int(lane_max_batch), ctypes.byref(k),
                                                             ctypes.byref(n)))
            cache[key] = ((SCAN_KERNELS[k.value] if k.value >= 0 else None), n.value, tables)   # (tables: keeps its id its own)
        return cache[key][:2]

    def can_decode(self, tables, batch):
        ok = ctypes.c_int()
        _lib.check(_lib.lib().basic_scanline_can_decode(self._h, tables._h, int(batch), ctypes.byref(ok)))
        return bool(ok.value)

    def decode(self, tables, d_words, d_word_off, prior, batch, h, w, table, lanes=1, rows=False):
        """-> (symbols, indexes int32 [B, H*W*C] in coding order, y_hat [B, C, H, W]).  `lanes` > 1: d_word_off holds the
        batch * lanes + 1 offsets of the lane streams (basic_scanline_decode_lanes_dev); `rows`: the batch * h * lanes + 1 offsets
        of the row streams (basic_scanline_decode_rows_dev)."""
        table = _dev(table, torch.float32)
        prior = _dev(prior, torch.float32) if prior is not None else None
        d_words, d_word_off = _dev(d_words, torch.int32), _dev(d_word_off, torch.int64)
        C = self.channels
        sym = torch.empty((batch, h * w * C), device=table.device, dtype=torch.int32)
        idx = torch.empty((batch, h * w * C), device=table.device, dtype=torch.int32)
        ybuf = torch.empty((batch, C, h, w), device=table.device, dtype=torch.float32)
        entry = _lib.lib().basic_scanline_decode_rows_dev if rows else _lib.lib().basic_scanline_decode_lanes_dev
        _lib.check(entry(self._h, tables._h, d_words.data_ptr(), d_word_off.data_ptr(), prior.data_ptr() if prior is not None else None, batch,
                         int(lanes), h, w, table.data_ptr(), table.numel(), sym.data_ptr(), idx.data_ptr(), ybuf.data_ptr(), _stream()))
        return sym, idx, ybuf

    def check(self):
        """Synchronises the current stream; raises if a barrier of the last launch gave up."""
        bad = ctypes.c_int()
        _lib.check(_lib.lib().basic_scanline_status(self._h, _stream(), ctypes.byref(bad)))
        if bad.value:
            raise _lib.BasicHipError("persistent scan-line kernel: an in-kernel barrier timed out (grid not resident?)")
