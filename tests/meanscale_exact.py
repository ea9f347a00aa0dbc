"""The mean-scale y coder restated in NumPy float32 (INTEGRATION.md "Mean-scale hyperprior"): what basic_gc_quantize_index_ms_dev,
basic_gc_dequantize_ms_dev and basic_gc_rate_curve_ms_dev must give bit for bit.  Every line is one IEEE operation on float32
arrays, which NumPy rounds correctly: no kernel of the library is behind any of it.  The index rule is qstep_exact's, the cost of a
symbol rate_exact's.

    s    = fmax(scale, bound)                   (a NaN scale counts as the bound)
    s'   = s / step                             only with a step
    idx  = index rule on s (or s')
    r    = y - mu
    q    = rint(r)          or  rint(r / step)
    sym  = int32(q)
    yhat = q + mu           or  (q * step) + mu            two roundings with a step
    decoder: yhat = float(sym) + mu   or  (float(sym) * step) + mu

The parameters of element i = b * per_image + r are scales[b * param_stride + r] and means[b * param_stride + r]: with the chunked
prior [B][2 M][h][w] read in place, scales = prior.reshape(-1), means = the same array from per_image on, param_stride = 2 per_image.
"""
import numpy as np

import qstep_exact as QX
import rate_exact as RX


def gather_params(base, batch, per_image, param_stride):
    """float32 [batch * per_image]: base[b * param_stride + r] for b < batch, r < per_image."""
    base = np.asarray(base, dtype=np.float32).reshape(-1)
    pos = (np.arange(batch, dtype=np.int64)[:, None] * param_stride + np.arange(per_image, dtype=np.int64)[None, :]).reshape(-1)
    return base[pos]


def split_prior(prior, per_image):
    """(scales, means) of a chunked prior [B][2 * per_image], both flat float32 [B * per_image]: upstream's chunk(2, 1)."""
    prior = np.asarray(prior, dtype=np.float32)
    B = prior.size // (2 * per_image)
    flat = prior.reshape(-1)
    return gather_params(flat, B, per_image, 2 * per_image), gather_params(flat[per_image:], B, per_image, 2 * per_image)


def quantize_index_ms(y, scales, means, steps, per_image, table, bound):
    """-> (sym int32, idx int32, yhat float32), flat, for flat float32 `y`, `scales`, `means` of batch * per_image elements (already
    gathered).  `steps`: None (the step-less lines), one step, or one per image."""
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    scales = np.asarray(scales, dtype=np.float32).reshape(-1)
    means = np.asarray(means, dtype=np.float32).reshape(-1)
    assert y.size == scales.size == means.size and y.size % per_image == 0
    s = np.fmax(scales, np.float32(bound))
    r = (y - means).astype(np.float32)
    if steps is None:
        q = np.rint(r)
        return q.astype(np.int32), QX.index_rule(s, table), (q + means).astype(np.float32)
    d = QX.steps_per_element(steps, y.size // per_image, per_image)
    idx = QX.index_rule((s / d).astype(np.float32), table)
    q = np.rint((r / d).astype(np.float32))
    p = (q * d).astype(np.float32)
    return q.astype(np.int32), idx, (p + means).astype(np.float32)


def dequantize_ms(sym, means, steps, per_image):
    sym = np.asarray(sym, dtype=np.int32).reshape(-1)
    means = np.asarray(means, dtype=np.float32).reshape(-1)
    f = sym.astype(np.float32)
    if steps is None:
        return (f + means).astype(np.float32)
    d = QX.steps_per_element(steps, sym.size // per_image, per_image)
    p = (f * d).astype(np.float32)
    return (p + means).astype(np.float32)


def same_reconstruction(decoded, encoded, sym, means):
    """The decoder-bits rule: the encoder's bits wherever sym != 0 or mu != 0; at sym == 0 and mu == +-0 both are a zero (the
    encoder's rint may have left -0.0, as qstep_exact.same_reconstruction documents for the zero-mean path)."""
    decoded, encoded, sym, means = (np.asarray(a).reshape(-1) for a in (decoded, encoded, sym, means))
    free = (sym == 0) & (means == 0)
    return bool(np.array_equal(decoded[~free].view(np.int32), encoded[~free].view(np.int32))
                and (decoded[free] == 0).all() and (encoded[free] == 0).all())


def rate_curve_ms(y, scales, means, n_seg, per_seg, segs_per_image, cand, scale_table, bound, table, sizes, offsets, bprec=4):
    """int64 [n_seg][K]: the summed cost of every segment at every candidate (cand: [K], or [B][K] with a grid per image)."""
    cand = np.asarray(cand, dtype=np.float32)
    K = cand.shape[-1]
    out = np.zeros((n_seg, K), dtype=np.int64)
    per_image = per_seg * segs_per_image
    for k in range(K):
        steps = cand[k:k + 1] if cand.ndim == 1 else cand[:, k]
        sym, idx, _ = quantize_index_ms(y, scales, means, steps, per_image, scale_table, bound)
        out[:, k] = RX.symbol_costs(sym, idx, table, sizes, offsets, bprec).reshape(n_seg, per_seg).sum(1)
    return out
