"""Shared driver of the table-ANS parity tests: runs any (TansEncoder, TansDecoder) pair -- the CPU oracle, the HIP drop-in,
oracle/_ref -- over the reference-generated known answers in tests/golden/tans_kat.npz (tests/golden/make_golden.py::tans_kats)."""
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    return np.load(os.path.join(G, "tans_kat.npz"), allow_pickle=False)


def check_known_answers(mod):
    z = load()
    nonempty = 0
    for name in z["names"]:
        L, byp, bprec = (int(v) for v in z[f"{name}.cfg"])
        enc, dec = mod.TansEncoder(L, 255, bool(byp), bprec), mod.TansDecoder(L, 255, bool(byp), bprec)
        enc.init_params(z[f"{name}.freqs"], z[f"{name}.nsym"], z[f"{name}.offsets"])
        dec.init_params(z[f"{name}.freqs"], z[f"{name}.nsym"], z[f"{name}.offsets"])
        kw = {}
        if f"{name}.ar_table" in z.files:
            enc.init_ar_params(z[f"{name}.ar_table"], z[f"{name}.ar_cfg"])
            dec.init_ar_params(z[f"{name}.ar_table"], z[f"{name}.ar_cfg"])
            kw = dict(ar_indexes=z[f"{name}.ar_indexes"], ar_offsets=z[f"{name}.ar_offsets"])
        sym, idx, ref = z[f"{name}.symbols"], z[f"{name}.indexes"], z[f"{name}.bytes"].tobytes()
        if int(z[f"{name}.error"]):
            with pytest.raises(ValueError):   # the reference: "Destination buffer is too small" (bitstream.h:192)
                enc.encode_with_indexes(sym, idx, **kw)
            continue
        assert enc.encode_with_indexes(sym, idx, **kw) == ref, name   # b"" where the reference's budget overflows
        if ref:
            nonempty += 1
            assert np.array_equal(dec.decode_with_indexes(ref, idx, **kw), z[f"{name}.decoded"]), name
    assert nonempty >= 7
    return nonempty


def random_case(rng, trial):
    L = int(rng.integers(9, 13))
    nd, ns = int(rng.integers(1, 8)), int(rng.integers(2, min(200, (1 << L) // 2)))
    if trial % 3 == 0:
        freqs = np.maximum((rng.random((nd, ns)) ** 6 * 5000).astype(np.int32), 1)
    else:
        freqs = rng.integers(1, 1024, (nd, ns)).astype(np.int32)
    nsym = rng.integers(2, ns + 1, nd).astype(np.int32)
    off = rng.integers(-5, 5, nd).astype(np.int32)
    n = int(rng.integers(6, 3000))
    idx = rng.integers(0, nd, n).astype(np.int32)
    byp = bool(trial % 2)
    if byp:
        sym = (off[idx] + rng.integers(-3, 1 << 30, n) % (nsym[idx] + 6)).astype(np.int32)
        sym[::13] = rng.integers(-70000, 70000, sym[::13].size)
    else:
        sym = (off[idx] + rng.integers(0, 1 << 30, n) % nsym[idx]).astype(np.int32)
    return L, freqs, nsym, off, byp, sym, idx


def run(mod, case):
    """(error text or None, bytes or None, decoded or None) of one case through one implementation."""
    L, freqs, nsym, off, byp, sym, idx = case
    try:
        enc = mod.TansEncoder(L, 255, byp, 4)
        enc.init_params(freqs, nsym, off)
        data = enc.encode_with_indexes(sym, idx)
    except ValueError as e:
        return str(e), None, None
    back = None
    if data:
        dec = mod.TansDecoder(L, 255, byp, 4)
        dec.init_params(freqs, nsym, off)
        back = dec.decode_with_indexes(data, idx)
    return None, data, back


# ---------------------------------------------------------------------------------------------------------------------------
# launch paths of csrc/tans.hip (tests/test_cpu_rans_cases.py, tests/test_gpu_rans_paths.py)
# ---------------------------------------------------------------------------------------------------------------------------
PATH_STREAMS = 37
# (table_log, distributions): with bypass coding on, the images hold nd + 1 rows of 2^L states -- decoder 4 bytes per state,
# encoder 2 -- and stay in the LDS up to 144 KiB (tans_lds_bytes): at L = 12 the decoder leaves it at 9 rows, the encoder at 18
PATH_CONFIGS = ((12, 8), (12, 9), (12, 17), (12, 18), (9, 5))


def path_kernels(L, nd, bypass=True):
    """(encoder, decoder) BASIC_TANS_KERNEL_* names of the batched entry points: tans_lds_bytes as launch_tans of tans.hip gets it, restated."""
    rows = nd + (1 if bypass else 0)
    fits = lambda per_state: rows * (1 << L) * per_state <= 144 * 1024
    return "ENC_LDS" if fits(2) else "ENC_GLOBAL", "DEC_LDS" if fits(4) else "DEC_GLOBAL"


def path_case(L, nd):
    """37 ragged streams (one empty, one of a single symbol) over nd distributions, bypass coding on: the shared table
    arguments and one `run` case per stream."""
    rng = np.random.default_rng(1000 * L + nd)
    ns = 90 if L >= 11 else 40
    freqs = rng.integers(1, 1024, (nd, ns)).astype(np.int32)
    freqs[0, : ns // 2] = 1                      # a row with many symbols of the smallest count
    nsym = rng.integers(ns // 2, ns + 1, nd).astype(np.int32)
    nsym[0] = ns
    off = rng.integers(-4, 4, nd).astype(np.int32)
    lens = rng.integers(2, 700, PATH_STREAMS)
    lens[[3, 5, 36]] = 0, 1, 64
    streams = []
    for n in lens.tolist():
        idx = rng.integers(0, nd, n).astype(np.int32)
        sym = (off[idx] + rng.integers(-2, 1 << 30, n) % (nsym[idx] + 3)).astype(np.int32)
        sym[::17] = rng.integers(-3000, 3000, sym[::17].size)
        streams.append((L, freqs, nsym, off, True, sym, idx))
    return streams


def run_raw(mod, case):
    """(bytes, symbols coded incl. bypass digits, decoded) of one case through the ORACLE module without the reference's
    output budget (capacity_syms: a stream that does not fit len(indexes) * table_log / 8 - 8 bytes comes back empty there, and
    five symbols or fewer are an error; `run` keeps that rule) -- the raw stream, which is what the batched entry points write."""
    L, freqs, nsym, off, byp, sym, idx = case
    enc = mod.TansEncoder(L, 255, byp, 4)
    enc.init_params(freqs, nsym, off)
    data = enc.encode_with_indexes(sym, idx, capacity_syms=1 << 40)
    dec = mod.TansDecoder(L, 255, byp, 4)
    dec.init_params(freqs, nsym, off)
    return data, enc.coded_symbols, dec.decode_with_indexes(data, idx)
