"""Rate control of the hyperprior y coder restated in NumPy (INTEGRATION.md "Rate control"): the cost table, the cost of a symbol
with its escape code, the byte bound, the first candidate grid, the select rule and the float32 refinement.  No library of the
project is behind any of it; the symbols and indexes of a step come from qstep_exact.quantize_index_q.

    cost table   out[r][v] = rint((precision - log2(cdf[r][v + 1] - cdf[r][v])) * 65536), v <= size[r] - 2, else 0   (2^-16 bit)
    symbol       value = sym - offset[row], max = size[row] - 2
                 value < 0: raw = -2 value - 1;  value >= max: raw = 2 (value - max);  either way escaped
                 cost = table[row][escaped ? max : value] + (escaped ? bprec (nb + 1 + nb // maxbv) 65536 : 0)
                 nb = digits of bprec bits in raw, maxbv = 2^bprec - 1
    byte bound   bytes <= 4 (2 + ((bits + 4 n) >> 21))  for a stream of n symbols whose costs sum to bits
"""
import numpy as np

import qstep_exact as QX

NO_FIT = 0x40000000


def cost_table(cdfs, sizes, precision=16):
    cdfs = np.asarray(cdfs, dtype=np.int64)
    out = np.zeros(cdfs.shape, dtype=np.uint32)
    for r, n in enumerate(np.asarray(sizes).reshape(-1)):
        f = np.diff(cdfs[r, :n]).astype(np.float64)
        assert (f > 0).all()
        out[r, :n - 1] = np.rint((precision - np.log2(f)) * 65536.0).astype(np.uint32)
    return out


def escape_digits(raw, bprec):
    raw = np.asarray(raw, dtype=np.uint64)
    nb = np.zeros(raw.shape, dtype=np.int64)
    for k in range((32 + bprec - 1) // bprec):   # digit k exists while k * bprec < 32 and raw >> (k * bprec) != 0
        nb += ((raw >> np.uint64(k * bprec)) != 0).astype(np.int64)
    return nb


def symbol_costs(sym, idx, table, sizes, offsets, bprec=4):
    """int64 cost (2^-16 bit) of every (symbol, row) under `table` (the cost table in use: the library's own, read back)."""
    sym, idx = np.asarray(sym, dtype=np.int64).reshape(-1), np.asarray(idx, dtype=np.int64).reshape(-1)
    sizes, offsets = np.asarray(sizes, dtype=np.int64).reshape(-1), np.asarray(offsets, dtype=np.int64).reshape(-1)
    row = np.clip(idx, 0, len(sizes) - 1)
    mx = sizes[row] - 2
    value = sym - offsets[row]
    low, high = value < 0, value >= mx
    raw = np.where(low, -2 * value - 1, np.where(high, 2 * (value - mx), 0))
    esc = low | high
    col = np.where(esc, mx, value)
    cost = np.asarray(table)[row, col].astype(np.int64)
    nb = escape_digits(raw, bprec)
    maxbv = (1 << bprec) - 1
    return cost + np.where(esc, bprec * (nb + 1 + nb // maxbv) * 65536, 0)


def rate_curve(y, scales, n_seg, per_seg, segs_per_image, cand, scale_table, bound, table, sizes, offsets, bprec=4):
    """int64 [n_seg][K]: the summed cost of every segment at every candidate (cand: [K], or [B][K] with a grid per image)."""
    y, scales = np.asarray(y, np.float32).reshape(-1), np.asarray(scales, np.float32).reshape(-1)
    cand = np.asarray(cand, dtype=np.float32)
    B = n_seg // segs_per_image
    K = cand.shape[-1]
    out = np.zeros((n_seg, K), dtype=np.int64)
    per_image = per_seg * segs_per_image
    for k in range(K):
        steps = cand[k:k + 1] if cand.ndim == 1 else cand[:, k]
        sym, idx, _ = QX.quantize_index_q(y, scales, steps, per_image, scale_table, bound)
        out[:, k] = symbol_costs(sym, idx, table, sizes, offsets, bprec).reshape(n_seg, per_seg).sum(1)
    assert B * per_image == y.size
    return out


def stream_bound(bits, n):
    """The byte bound of one stream, in Python integers."""
    return 4 * (2 + ((int(bits) + 4 * int(n)) >> 21))


def first_grid(K, step_range=(2.0 ** -4, 2.0 ** 6)):
    lo, hi = np.log2(np.float64(step_range[0])), np.log2(np.float64(step_range[1]))
    return np.array([np.float32(np.float64(2.0) ** (lo + (hi - lo) * k / (K - 1))) for k in range(K)], dtype=np.float32)


def select(bits, segs_per_image, per_seg, cand, budgets, extra_words=None):
    """-> (steps float32 [B], choice int32 [B], pred int64 [B]): the first candidate, in order, whose predicted payload fits."""
    bits, cand = np.asarray(bits, dtype=np.int64), np.asarray(cand, dtype=np.float32)
    B, K = bits.shape[0] // segs_per_image, bits.shape[1]
    steps, choice, preds = np.zeros(B, np.float32), np.zeros(B, np.int32), np.zeros(B, np.int64)
    for b in range(B):
        c = cand if cand.ndim == 1 else cand[b]
        extra = 4 * int(extra_words[b]) if extra_words is not None else 0
        pick = None
        for k in range(K):
            pred = extra + sum(stream_bound(bits[b * segs_per_image + l, k], per_seg) for l in range(segs_per_image))
            if pred <= int(budgets[b]):
                pick = k
                break
        k = K - 1 if pick is None else pick
        choice[b] = (k | NO_FIT) if pick is None else k
        steps[b], preds[b] = c[k], pred
    return steps, choice, preds


def refine(cand, choice, n_images):
    """float32 [B][K]: every line one float32 operation."""
    cand = np.asarray(cand, dtype=np.float32)
    K = cand.shape[-1]
    t = (np.arange(1, K + 1, dtype=np.float32) / np.float32(K)).astype(np.float32)
    out = np.zeros((n_images, K), dtype=np.float32)
    for b in range(n_images):
        c = cand if cand.ndim == 1 else cand[b]
        ch = int(choice[b])
        k = ch & ~NO_FIT
        if k == 0 or ch & NO_FIT:
            out[b, :] = c[k]
            continue
        lo, hi = c[k - 1], c[k]
        d = np.float32(hi - lo)
        for j in range(K - 1):
            out[b, j] = np.minimum(np.float32(lo + np.float32(d * t[j])), hi)
        out[b, K - 1] = hi
    return out
