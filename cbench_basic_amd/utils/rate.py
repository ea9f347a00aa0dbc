"""Rate control of the hyperprior y coder: the host side of ``compress_to_rate`` (INTEGRATION.md "Rate control").  Validation of a
request, the first candidate grid and the refinement's interpolation weights; nothing here launches anything.

A request states, per image, a byte budget for the image's payload (its z stream plus its y stream(s); the framing is not budgeted).
The kernels of csrc/entropy.hip rate K candidate steps from one read of y and sigma, pick the first (smallest) step whose predicted
payload fits, and refine between it and its lower neighbour ``passes - 1`` times.
"""
import math

import numpy as np

from .qstep import QSTEP_MAX, QSTEP_MIN

MAX_CANDIDATES, MAX_PASSES = 32, 3
NO_FIT = 0x40000000   # BASIC_RATE_NO_FIT in a choice word: no candidate fitted, the largest step was taken


def _vector(v, name, batch):
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or a sequence of numbers, got {v!r}")
    if a.ndim == 0:
        a = a.reshape(1)
    if a.ndim != 1 or a.size == 0 or (batch is not None and a.size not in (1, int(batch))):
        raise ValueError(f"{name}: give one value, or one per image of the batch of {batch} (got shape {a.shape})")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite, got {a.tolist()}")
    return a


def check_budgets(budgets, batch=None) -> np.ndarray:
    """Byte budgets (a number or one per image) as int64 [1 or batch]; ValueError unless every one is a whole number >= 1."""
    a = _vector(budgets, "target_bytes", batch)
    if np.any(a < 1) or np.any(a != np.floor(a)) or np.any(a >= 2.0 ** 62):
        raise ValueError(f"every byte budget must be a positive whole number, got {a.tolist()}")
    return np.ascontiguousarray(a.astype(np.int64))


def budgets_from(target_bytes, target_bpp, batch, height, width) -> np.ndarray:
    """Exactly one of the two targets -> int64 budgets; ``budget = floor(bpp * H * W / 8)``."""
    if (target_bytes is None) == (target_bpp is None):
        raise ValueError("give exactly one of target_bytes and target_bpp")
    if target_bytes is not None:
        return check_budgets(target_bytes, batch)
    bpp = _vector(target_bpp, "target_bpp", batch)
    if np.any(bpp <= 0):
        raise ValueError(f"target_bpp must be positive, got {bpp.tolist()}")
    return check_budgets(np.floor(bpp * int(height) * int(width) / 8.0), batch)


def check_passes(passes) -> int:
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= passes <= MAX_PASSES:
        raise ValueError(f"passes must be an integer in [1, {MAX_PASSES}], not {passes!r}")
    return int(passes)


def check_candidates(cand) -> np.ndarray:
    """A candidate grid as float32 [K], K in [2, 32], strictly ascending inside [2^-4, 2^6]; ValueError otherwise."""
    a = np.asarray(cand, dtype=np.float32).reshape(-1)
    if not 2 <= a.size <= MAX_CANDIDATES:
        raise ValueError(f"a candidate grid holds 2 to {MAX_CANDIDATES} steps, not {a.size}")
    if not np.all(np.isfinite(a)) or a[0] < QSTEP_MIN or a[-1] > QSTEP_MAX or np.any(np.diff(a) <= 0):
        raise ValueError(f"candidate steps must be strictly ascending and in [{QSTEP_MIN}, {QSTEP_MAX}], got {a.tolist()}")
    return np.ascontiguousarray(a)


def first_grid(candidates=16, step_range=(QSTEP_MIN, QSTEP_MAX)) -> np.ndarray:
    """``float32(2 ** (lo + (hi - lo) * k / (K - 1)))`` over ``log2(step_range)``, computed in float64."""
    if isinstance(candidates, bool) or not isinstance(candidates, (int, np.integer)) or not 2 <= candidates <= MAX_CANDIDATES:
        raise ValueError(f"candidates must be an integer in [2, {MAX_CANDIDATES}], not {candidates!r}")
    try:
        lo, hi = (float(v) for v in step_range)
    except (TypeError, ValueError):
        raise ValueError(f"step_range must be a pair (smallest step, largest step), got {step_range!r}")
    if not (math.isfinite(lo) and math.isfinite(hi) and QSTEP_MIN <= lo < hi <= QSTEP_MAX):
        raise ValueError(f"step_range must satisfy {QSTEP_MIN} <= lo < hi <= {QSTEP_MAX}, got {step_range!r}")
    l2lo, l2hi = math.log2(lo), math.log2(hi)
    K = int(candidates)
    grid = np.array([2.0 ** (l2lo + (l2hi - l2lo) * k / (K - 1)) for k in range(K)], dtype=np.float64).astype(np.float32)
    try:
        return check_candidates(grid)
    except ValueError:
        raise ValueError(f"step_range {step_range!r} is too narrow for {K} distinct float32 candidates")


class RateTarget:
    """A validated request, as ``encode(..., rate_target=)`` takes it: ``budgets`` int64 [1 or B], the first grid ``candidates``
    float32 [K] and ``passes``.  ``extra_words`` (int [B], optional): 32-bit words an image has already spent on other streams (the
    latent graph fills in the z streams').  The coder leaves its choices in ``steps`` / ``predicted_bytes`` / ``flags`` (NumPy, [B])."""

    def __init__(self, budgets, candidates=None, passes=2, batch=None):
        self.budgets = check_budgets(budgets, batch)
        self.candidates = first_grid() if candidates is None else check_candidates(candidates)
        self.passes = check_passes(passes)
        self.extra_words = None
        self.steps = self.predicted_bytes = self.flags = None

    def budgets_for(self, batch) -> np.ndarray:
        if self.budgets.size not in (1, int(batch)):
            raise ValueError(f"{self.budgets.size} byte budgets for a batch of {batch}: give one, or one per image")
        return np.array(np.broadcast_to(self.budgets, (int(batch),)), dtype=np.int64)   # a copy: writable, contiguous

    def set_result(self, steps, predicted_bytes, flags):
        self.steps = np.asarray(steps, dtype=np.float32).copy()
        self.predicted_bytes = np.asarray(predicted_bytes, dtype=np.int64).copy()
        self.flags = np.asarray(flags, dtype=np.int32).copy()

    def set_device_result(self, steps, predicted_bytes, flags):
        """The module path's choices as device tensors: brought to the host by resolve(), after the streams are."""
        self._pending = (steps, predicted_bytes, flags)

    def resolve(self):
        pending, self._pending = getattr(self, "_pending", None), None
        if pending is not None:
            self.set_result(*(t.cpu().numpy() for t in pending))
        return self

    @property
    def fits(self):
        """bool [B]: a candidate's predicted payload fitted the budget."""
        return (self.flags & NO_FIT) == 0


def as_rate_target(rate_target, batch=None) -> "RateTarget":
    """``rate_target`` of encode(): a RateTarget, or byte budgets (a number / one per image) under the default grid and passes."""
    if isinstance(rate_target, RateTarget):
        if batch is not None:
            rate_target.budgets_for(batch)   # ValueError when the count fits neither one nor the batch
        return rate_target
    return RateTarget(rate_target, batch=batch)


def refine_t(n_cand) -> np.ndarray:
    """``t[j] = float32(j + 1) / float32(K)``: the refinement's interpolation weights."""
    j = np.arange(1, int(n_cand) + 1, dtype=np.float32)
    return np.ascontiguousarray((j / np.float32(n_cand)).astype(np.float32))


def stream_bytes_bound(bits_q16, n_symbols):
    """The byte bound of a rANS64 stream of ``n_symbols`` symbols whose table costs sum to ``bits_q16`` (2^-16 bit):
    ``4 * (2 + ((bits + 4 n) >> 21))``."""
    return 4 * (2 + ((np.asarray(bits_q16).astype(np.int64) + 4 * int(n_symbols)) >> 21))
