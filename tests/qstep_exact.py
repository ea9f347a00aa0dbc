"""The quantiser step of the hyperprior y coder, restated in NumPy float32 (INTEGRATION.md "Quantiser step"): what
basic_gc_quantize_index_q_dev / basic_gc_dequantize_q_dev must give bit for bit, and the negative log-likelihood that
basic_gauss_nll_per_image_q_dev estimates, term by term in a chosen precision.  Every line is one IEEE operation on float32 arrays,
which NumPy rounds correctly: no kernel of the library is behind any of it.

    s   = fmax(scale, bound)          (a NaN scale counts as the bound, as C's fmaxf has it)
    s'  = s / step
    idx = first j in [0, len - 1) with table[j] >= s', else len - 1     == (len - 1) - #{j < len - 1 : s' <= table[j]}
    q   = rint(y / step),  sym = int32(q),  yhat = q * step
"""
import math

import numpy as np

SQRT2 = math.sqrt(2.0)


def steps_per_element(steps, batch, per_image):
    """float32 [batch * per_image]: the step of every element (one step broadcasts)."""
    steps = np.asarray(steps, dtype=np.float32).reshape(-1)
    assert steps.size in (1, batch)
    return np.repeat(np.broadcast_to(steps, (batch,)) if steps.size == 1 else steps, per_image)


def index_rule(s, table):
    """The index of float32 scales `s` in `table` by the counting definition; a NaN counts nothing (len - 1)."""
    table = np.asarray(table, dtype=np.float32)
    s = np.asarray(s, dtype=np.float32).reshape(-1)
    idx = np.full(s.shape, len(table) - 1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for t in table[:-1]:
            idx -= (s <= t).astype(np.int32)
    return idx


def quantize_index_q(y, scales, steps, per_image, table, bound):
    """-> (sym int32, idx int32, yhat float32), flat, for flat float32 `y`, `scales` of batch * per_image elements."""
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    scales = np.asarray(scales, dtype=np.float32).reshape(-1)
    assert y.size == scales.size and y.size % per_image == 0
    d = steps_per_element(steps, y.size // per_image, per_image)
    s = np.fmax(scales, np.float32(bound))
    sq = (s / d).astype(np.float32)
    idx = index_rule(sq, table)
    q = np.rint((y / d).astype(np.float32))
    return q.astype(np.int32), idx, (q * d).astype(np.float32)


def dequantize_q(sym, steps, per_image):
    sym = np.asarray(sym, dtype=np.int32).reshape(-1)
    d = steps_per_element(steps, sym.size // per_image, per_image)
    return (sym.astype(np.float32) * d).astype(np.float32)


def same_reconstruction(decoded, encoded, sym):
    """The decoder's float(sym) * step against the encoder's q * step: the same bits wherever the symbol is not 0.  A symbol 0 has no
    sign: the encoder's q = rint(y / step) is -0.0 for y in [-step / 2, 0) (as today's kernel writes rint(y)), an integer 0 decodes to
    +0.0 (as today's int32 -> float32 kernel does); there the two are equal as floats, and both are a zero."""
    decoded, encoded, sym = (np.asarray(a).reshape(-1) for a in (decoded, encoded, sym))
    nz = sym != 0
    return bool(np.array_equal(decoded[nz].view(np.int32), encoded[nz].view(np.int32))
                and (decoded[~nz] == 0).all() and (encoded[~nz] == 0).all() and not np.signbit(decoded[~nz]).any())


def nll_terms_q(q, scales, steps, bound, lik_bound, dtype):
    """-log(max(P, lik_bound)) per element of [B, ...] arrays, evaluated in torch `dtype` on the CPU: zero mean, v = |q|,
    P = Phi((.5 - v) / s') - Phi((-.5 - v) / s'), Phi(t) = .5 erfc(-t / sqrt 2), with s' = fmax(scale, bound) / step the float32
    quotient of the format in every precision (the division belongs to the format, not to the estimate)."""
    import torch
    q = np.asarray(q, dtype=np.float32)
    B, per = q.shape[0], q[0].size
    d = steps_per_element(steps, B, per).reshape(q.shape)
    sq = (np.fmax(np.asarray(scales, dtype=np.float32), np.float32(bound)) / d).astype(np.float32)
    s, v = torch.from_numpy(sq).to(dtype), torch.from_numpy(np.abs(q)).to(dtype)
    half = torch.tensor(0.5, dtype=dtype)
    phi = lambda t: half * torch.erfc(-t / SQRT2)
    p = phi((half - v) / s) - phi((-half - v) / s)
    return -torch.log(torch.clamp(p, min=lik_bound))
