"""Tables and streams that put every rANS launch path of csrc/rans.hip in front of the oracle (oracle/rans64_oracle.c).

The tables are built from CDF ROWS, not from random frequencies, so that a frequency of 1, 2^p - 1 or 2^p, a start of 2^p - 1, a
row of exactly 64 / 65 / 4096 / 4097 entries and a precision below 12 are placed where they are wanted.  Every case names the
kernels it must reach (BASIC_RANS_KERNEL_* of include/basic_hip.h, without the prefix); predict() restates the thresholds of
upload_tables / launch_encode / launch_decode in rans.hip, and tests/test_cpu_rans_cases.py holds the two against each other, so that a case
that drifts off its path fails on the CPU before tests/test_gpu_rans_paths.py asserts the path on the GPU.

Stream shapes, the same for every table: a ragged batch of 19 streams (a part-filled last workgroup at 2, 4, 8 and 16 streams
per workgroup) over the lengths 0, 1, 2, 63, 64, 65, 127, 128, 129 and 4097; the GPU tests also launch one stream alone and
exactly W of them.

What a table holds but the data never code, because the ORACLE (as the reference) divides by zero there:
  * a zero-width symbol (`zero_width`);
  * the one symbol of a 2-entry row at precision 16 (`row_widths*`): its frequency 2^16 is 0 after the reference's uint16_t
    cast.  The row is in the table for the image layout; below precision 16 (`lowp`) the row [0, 2^p] IS coded.
"""
import functools
import os
import re

import numpy as np

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097)
BATCH = 19
BATCH_LENGTHS = LENGTHS + LENGTHS[-2::-1]            # 19 streams: up the list and down again
WAVES = (1, 2, 4, 8, 16)
LOWP = (1, 2, 4, 6, 7, 8, 11, 15)
FAST_MIN_PRECISION = 7   # below it the 24-bit multiplies of the fast encoder and decoder lose bits of x / freq, x >> p: general kernels

RESUME_IMAGES, RESUME_LANES, RESUME_PIECES = 5, 3, (1, 63, 64, 65, 64)
RESUME_LEN = sum(RESUME_PIECES)                      # 257


class Case:
    """One table set and its streams.  streams: list of (symbols, indexes) int32 arrays.  ar: None, or (ar_table [1][rows][s1],
    init_ar_params' offsets argument); AR cases run through the host drop-in (one stream per call), ar_offsets(n) are their
    per-element back distances."""

    def __init__(self, name, precision, bypass, rows, offsets, streams_fn, enc, dec, ar=None, seed=0):
        self.name, self.precision, self.bypass, self.bypass_precision = name, int(precision), bool(bypass), 4
        self.sizes = np.array([len(r) for r in rows], np.int32)
        self.cdfs = np.zeros((len(rows), int(self.sizes.max())), np.int32)
        for r, row in enumerate(rows):
            self.cdfs[r, : len(row)] = row
        self.offsets = np.asarray(offsets, np.int32)
        self.enc, self.dec, self.ar = enc, dec, ar
        self.streams = [(np.ascontiguousarray(s, np.int32), np.ascontiguousarray(i, np.int32)) for s, i in streams_fn(self, np.random.default_rng(seed))]

    def __repr__(self):
        return self.name

    @property
    def kernels(self):
        return {self.enc, self.dec}

    @staticmethod
    def ar_offsets(n):
        off = np.ones((1, n), np.int32)    # order 1: the previous symbol of the stream
        off[0, :1] = 0
        return off

    # ---- data ----
    def codable(self, r):
        """Values 0 .. max of row r that the oracle can code as plain symbols (see the module docstring)."""
        row = self.cdfs[r, : self.sizes[r]].astype(np.int64)
        freq = np.diff(row)[: self.sizes[r] - 1 - (1 if self.bypass else 0)]    # with bypass the last symbol is the sentinel
        return np.flatnonzero((freq > 0) & (freq < 65536))

    def sentinel_ok(self, r):
        f = int(self.cdfs[r, self.sizes[r] - 1]) - int(self.cdfs[r, self.sizes[r] - 2])
        return 0 < f < 65536

    def draw(self, rng, n, rows=None, escape=0.0, picks=None):
        """n symbols over `rows` (default: every row with a codable symbol).  escape: share of bypass values, a third of them
        at 31 bits (raw code of 31 bits: eight payload digits), the rest within three of the row's ends."""
        if rows is None:
            rows = [r for r in range(len(self.sizes)) if len(self.codable(r)) or (self.bypass and self.sentinel_ok(r))]
        idx = rng.choice(np.asarray(rows), n).astype(np.int32)
        val = np.zeros(n, np.int64)
        for r in set(idx.tolist()):
            m = idx == r
            ok = picks[r] if picks is not None else self.codable(r)
            k = int(m.sum())
            esc = np.zeros(k, bool)
            if self.bypass and self.sentinel_ok(r):
                esc = rng.random(k) < (escape if len(ok) else 1.0)
            v = ok[rng.integers(0, max(len(ok), 1), k)] if len(ok) else np.zeros(k, np.int64)
            mx = int(self.sizes[r]) - 2
            near = np.where(rng.random(k) < 0.5, -1 - rng.integers(0, 3, k), mx + rng.integers(0, 4, k))
            far = rng.integers(1 << 29, 1 << 30, k) * rng.choice([-1, 1], k)
            val[m] = np.where(esc, np.where(rng.random(k) < 1 / 3, far, near), v)
        return (val + self.offsets[idx]).astype(np.int32), idx


def _cuts(rng, entries, precision):
    """A CDF row of `entries` entries: 0, entries - 2 distinct random cuts, 2^precision (every frequency >= 1)."""
    one = 1 << precision
    k = entries - 2
    if 4 * k < one:      # few cuts: draw until they are distinct
        inner = np.zeros(0, np.int64)
        while inner.size < k:
            inner = np.unique(np.concatenate([inner, rng.integers(1, one, k - inner.size)]))
    else:
        inner = np.sort(rng.choice(np.arange(1, one), k, replace=False))
    return [0] + [int(v) for v in inner] + [one]


def _batch(escape=0.0):
    def streams(case, rng):
        return [case.draw(rng, n, escape=escape) for n in BATCH_LENGTHS]
    return streams


EXTREME_ROWS = [[0, 65535, 65536], [0, 1, 65536], [0, 32768, 65536], list(range(40)) + [65536], [0, 3, 21847, 65536]]
FREQ1_STREAM = 11       # stream of `extreme16` that codes only symbols of frequency 1


def _extreme_streams(case, rng):
    s = _batch()(case, rng)
    s[10] = case.draw(rng, 5000)                                   # every row, every symbol
    ones = {0: np.array([1]), 1: np.array([0]), 3: np.arange(39)}   # the symbols of frequency 1
    s[FREQ1_STREAM] = case.draw(rng, 5000, rows=[0, 1, 3], picks=ones)
    return s


def _resume_streams(case, rng):
    """5 images x 3 lanes of 257 symbols, bypass-heavy; the last symbol of every piece (1, 63, 64, 65, 64 symbols) is a bypass
    value in two streams of three, so that a resumed call starts directly behind an escape code."""
    out = []
    ends = np.cumsum(RESUME_PIECES) - 1
    for s in range(RESUME_IMAGES * RESUME_LANES):
        sym, idx = case.draw(rng, RESUME_LEN, escape=0.3)
        if s % 3 != 2:
            far = rng.integers(1 << 29, 1 << 30, ends.size) * (1 if s % 3 else -1)
            sym[ends] = (far + case.offsets[idx[ends]]).astype(np.int32)
        out.append((sym, idx))
    return out


def _wide_rows(rng, rows, entries):
    return [_cuts(rng, entries, 16) for _ in range(rows)]


def _ar_table(rng, rows, s1):
    return rng.integers(0, rows, (1, rows, s1)).astype(np.int32), [[[0, 0, -1]]]


@functools.lru_cache(maxsize=None)
def all_cases():
    rng = np.random.default_rng(20240)
    cases = []
    add = cases.append
    add(Case("extreme16", 16, False, EXTREME_ROWS, [0, -1, 2, -20, 7], _extreme_streams, "ENC_FAST", "DEC_FAST", seed=1))
    add(Case("extreme16_bypass", 16, True, EXTREME_ROWS, [0, -1, 2, -20, 7], _batch(0.4), "ENC_FAST", "DEC_FAST", seed=2))
    for p in LOWP:
        rows = [_cuts(rng, min(1 << p, 5) + 1, p) for _ in range(3)]
        if p < 16:
            rows.append([0, 1 << p])    # one symbol with all the mass: zero bits per symbol
        fast = p >= FAST_MIN_PRECISION
        add(Case(f"lowp{p}", p, False, rows, [0, -2, 3, 1], _batch(), "ENC_FAST" if fast else "ENC_GENERAL",
                 "DEC_FAST" if fast else "DEC_GENERAL_LDS", seed=10 + p))
    widths = (2, 3, 63, 64, 65, 66, 128, 129, 4096)
    rw = [_cuts(rng, e, 16) for e in widths]
    r4097 = _cuts(rng, 4097, 16)
    offs = [-(3 * r) for r in range(len(widths) + 1)]
    # the 2-entry row's frequency 2^16 keeps the whole table off the fast ENCODER; `_no2` is the same table without it
    add(Case("row_widths", 16, False, rw, offs[:-1], _batch(), "ENC_GENERAL", "DEC_FAST", seed=30))
    add(Case("row_widths_4097", 16, False, rw + [r4097], offs, _batch(), "ENC_GENERAL", "DEC_GENERAL_LDS", seed=31))
    add(Case("row_widths_no2", 16, False, rw[1:], offs[1:-1], _batch(), "ENC_FAST", "DEC_FAST", seed=32))
    big = _wide_rows(rng, 10, 4096)
    add(Case("image_too_big", 16, False, big, [0] * 10, _batch(), "ENC_FAST", "DEC_GENERAL_LDS", seed=33))
    glob = _wide_rows(rng, 18, 4098)
    add(Case("global_tables", 16, False, glob, [-2000] * 18, _batch(), "ENC_FAST", "DEC_GENERAL_GLOBAL", seed=34))
    add(Case("global_tables_ar", 16, False, glob, [0] * 18, _batch(), "ENC_GENERAL_AR", "DEC_AR_GLOBAL", ar=_ar_table(rng, 18, 4098), seed=35))
    add(Case("small_ar", 12, False, [_cuts(rng, 9, 12) for _ in range(6)], [0] * 6, _batch(), "ENC_GENERAL_AR", "DEC_AR_LDS",
             ar=_ar_table(rng, 6, 9), seed=36))
    narrow = [_cuts(rng, 4, 16) for _ in range(2049)]
    add(Case("rows2049", 16, False, narrow, [0] * 2049, _batch(), "ENC_GENERAL", "DEC_FAST", seed=37))
    add(Case("rows2048", 16, False, narrow[:2048], [0] * 2048, _batch(), "ENC_FAST", "DEC_FAST", seed=38))
    add(Case("zero_width", 16, False, [[0, 100, 100, 65536]], [-1], _batch(), "ENC_GENERAL", "DEC_FAST", seed=39))
    # resumed decoding: the same three decoder paths with bypass coding on
    add(Case("resume_fast", 16, True, EXTREME_ROWS + [_cuts(rng, 66, 16)], [0, -1, 2, -20, 7, -30], _resume_streams, "ENC_FAST", "DEC_FAST", seed=40))
    add(Case("resume_lds", 16, True, big, [-2048] * 10, _resume_streams, "ENC_FAST", "DEC_GENERAL_LDS", seed=41))
    add(Case("resume_global", 16, True, glob, [-2048] * 18, _resume_streams, "ENC_FAST", "DEC_GENERAL_GLOBAL", seed=42))
    return tuple(cases)


def case(name):
    return next(c for c in all_cases() if c.name == name)


def names(pred=lambda c: True):
    return [c.name for c in all_cases() if pred(c)]


# ---------------------------------------------------------------------------------------------------------------------------
# the launch thresholds of rans.hip, restated
# ---------------------------------------------------------------------------------------------------------------------------
LDS_TABLE_BUDGET = 144 * 1024        # kLdsTableBudget: packed uint16 rows
FAST_IMAGE_BUDGET = 156 * 1024       # upload_tables: search image of the fast decoder


def packed_bytes(c):
    n = int(c.sizes.sum())
    return 2 * (n + (n & 1))


def image_bytes(c):
    """Search image of the fast decoder: 16 bytes per entry of a row of <= 64 entries; a wider row is one 16-byte lane, 64 block
    ends and the row, padded to 16 bytes; 256 words behind the last row."""
    words = 256
    for s in c.sizes.tolist():
        words += 4 * s if s <= 64 else (4 + 64 + s + 3) // 4 * 4
    return 4 * words


def predict(c):
    """(encoder, decoder) kernel names the library must choose for case c (launch_encode, launch_decode of rans.hip)."""
    one = 1 << c.precision
    fast_dec = int(c.sizes.max()) <= 4096 and image_bytes(c) <= FAST_IMAGE_BUDGET and c.precision >= FAST_MIN_PRECISION
    lds = packed_bytes(c) <= LDS_TABLE_BUDGET
    rows, stride = c.cdfs.shape
    fast_enc = rows <= 2048 and rows * stride <= (4 << 20) and c.precision >= FAST_MIN_PRECISION
    for r in range(rows):
        row = c.cdfs[r, : c.sizes[r]].astype(np.int64)
        freq = np.diff(row) & 0xFFFF        # the reference's uint16_t cast
        if (freq == 0).any() or (freq >= one + (0 if c.precision == 16 else 1)).any():
            fast_enc = False
    if c.ar is not None:
        return "ENC_GENERAL_AR", "DEC_AR_LDS" if lds else "DEC_AR_GLOBAL"
    return ("ENC_FAST" if fast_enc else "ENC_GENERAL",
            "DEC_FAST" if fast_dec else "DEC_GENERAL_LDS" if lds else "DEC_GENERAL_GLOBAL")


def header_enum(prefix):
    """{name: value} of the `#define <prefix>NAME value` lines of include/basic_hip.h, NONE left out."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "basic_hip.h")
    found = re.findall(r"#define\s+" + prefix + r"(\w+)\s+\(?(-?\d+)\)?", open(path).read())
    return {n: int(v) for n, v in found if n != "NONE"}


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle on a case (cached: the GPU tests of one case share it)
# ---------------------------------------------------------------------------------------------------------------------------
def oracle_coders(c):
    from oracle import rans_oracle
    enc = rans_oracle.Rans64Encoder(c.precision, c.bypass, c.bypass_precision)
    dec = rans_oracle.Rans64Decoder(c.precision, c.bypass, c.bypass_precision)
    for o in (enc, dec):
        o.init_cdf_params(c.cdfs, c.sizes, c.offsets)
        if c.ar is not None:
            o.init_ar_params(*c.ar)
    return enc, dec


@functools.lru_cache(maxsize=None)
def oracle_streams(name):
    """Tuple of uint32 word arrays, one per stream of the case: the oracle's bytes (capacity 2n + 8 words, or it raises)."""
    c = case(name)
    enc, _ = oracle_coders(c)
    out = []
    for sym, idx in c.streams:
        kw = dict(ar_indexes=np.zeros_like(idx), ar_offsets=c.ar_offsets(idx.size)) if c.ar is not None else {}
        w = np.frombuffer(enc.encode_with_indexes(sym, idx, **kw), np.uint32).copy()
        w.setflags(write=False)
        out.append(w)
    return tuple(out)


def oracle_decode_pieces(c, words, idx, pieces):
    """set_stream / decode_stream over `pieces` symbol counts: [(symbols, state, pos)] after every piece.  pos = the next unread
    word of the stream (-1 only BEFORE the first call: decode_impl of rans64_oracle.c), the convention of d_pos / d_state."""
    _, dec = oracle_coders(c)
    dec.set_stream(words.tobytes())
    out, at = [], 0
    for n in pieces:
        sym = dec.decode_stream(idx[at: at + n])
        out.append((sym, int(dec._st.value), int(dec._pos.value)))
        at += n
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# exact-integer encoder in plain Python (no bypass, no AR): the oracle's arithmetic, or the fast kernel's
# ---------------------------------------------------------------------------------------------------------------------------
def python_encode(c, sym, idx, cut24=False):
    """uint32 words of one stream.  cut24=False: rans64.h:65-84 with Python integers.  cut24=True: the update as
    rans_encode_fast_kernel spells it -- x' = x + start + q * (2^p - freq) with the HIGH word of q = x / freq entering a 24-bit
    multiply (v_mad_u32_u24), i.e. cut to its low 24 bits; frequency 1 as q = x - 1 with 2^p - 1 folded into the start."""
    assert not c.bypass and c.ar is None
    p, one, m64 = c.precision, 1 << c.precision, (1 << 64) - 1
    x, words = 1 << 31, []
    for i in range(len(idx) - 1, -1, -1):
        r = int(idx[i])
        v = int(sym[i]) - int(c.offsets[r])
        start, freq = int(c.cdfs[r, v]) & 0xFFFF, (int(c.cdfs[r, v + 1]) - int(c.cdfs[r, v])) & 0xFFFF
        if x >= freq << (63 - p):
            words.append(x & 0xFFFFFFFF)
            x >>= 32
        if not cut24:
            x = ((x // freq) << p) + x % freq + start
            continue
        q, st = (x - 1, start + one - 1) if freq == 1 else (x // freq, start)
        cm = one - freq
        hi = (((q >> 32) & 0xFFFFFF) * cm) & 0xFFFFFFFF
        x = (x + st + (q & 0xFFFFFFFF) * cm + (hi << 32)) & m64
    words += [x >> 32, x & 0xFFFFFFFF]
    return np.array(words[::-1], np.uint32)


def python_decode(c, words, idx, cut24=False):
    """Symbols of one stream (no bypass, no AR).  cut24=False: rans64.h:128-142 with Python integers.  cut24=True: the update as
    the wave decoder's generic path spells it -- freq * (x >> p) with the HIGH word of x >> p entering a 24-bit multiply
    (__umul24).  Words past the stream's end read as 0, as in the kernels."""
    assert not c.bypass and c.ar is None
    p, mask, m64 = c.precision, (1 << c.precision) - 1, (1 << 64) - 1
    x, pos, out = int(words[0]) | (int(words[1]) << 32), 2, []
    for r in idx.tolist():
        row = c.cdfs[r, : c.sizes[r]]
        cf = x & mask
        s = int(np.searchsorted(row, cf, side="right")) - 1
        start, freq, t = int(row[s]), int(row[s + 1]) - int(row[s]), x >> p
        if cut24:
            hi = ((freq & 0xFFFFFF) * ((t >> 32) & 0xFFFFFF)) & 0xFFFFFFFF
            x = (freq * (t & 0xFFFFFFFF) + (cf - start) + (hi << 32)) & m64
        else:
            x = freq * t + cf - start
        if x < 1 << 31:
            x = (x << 32) | (int(words[pos]) if pos < len(words) else 0)
            pos += 1
        out.append(s + int(c.offsets[r]))
    return np.array(out, np.int32), x, pos
