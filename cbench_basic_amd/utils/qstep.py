"""Quantiser step of the hyperprior y coder: validation of the steps and the container that carries them (host code only).

A step d codes ``round(y / d)`` under ``N(0, sigma / d)`` and reconstructs ``round(y / d) * d`` (INTEGRATION.md "Quantiser
step"; the arithmetic is the kernels', csrc/entropy.hip).  The coded stream does not hold the steps; ``compress_q`` wraps it:

    b"BQS1" | uint32 LE n | n float32 LE steps | inner stream

with n = 1 (one step for every image) or the batch.  The inner stream is exactly what ``encode(x, qstep=)`` returned.
"""
import struct

import numpy as np

QSTEP_MAGIC = b"BQS1"
QSTEP_MIN, QSTEP_MAX = 2.0 ** -4, 2.0 ** 6   # BASIC_QSTEP_MIN / BASIC_QSTEP_MAX


def check_qsteps(qstep, batch=None) -> np.ndarray:
    """``qstep`` (a number, or a sequence / array / tensor of them) as a float32 vector of 1 or ``batch`` steps.
    ValueError for anything else: an empty or nested sequence, a step that is not finite or lies outside [2^-4, 2^6], a
    count that is neither 1 nor the batch."""
    if hasattr(qstep, "detach"):
        qstep = qstep.detach().cpu().numpy()
    try:
        steps = np.asarray(qstep, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"qstep must be a number or a sequence of numbers, got {qstep!r}")
    if steps.ndim == 0:
        steps = steps.reshape(1)
    if steps.ndim != 1 or steps.size == 0:
        raise ValueError(f"qstep must be one step or one per image, got an array of shape {steps.shape}")
    steps32 = steps.astype(np.float32)
    if not np.all(np.isfinite(steps32)) or np.any(steps32 < QSTEP_MIN) or np.any(steps32 > QSTEP_MAX):
        raise ValueError(f"every quantiser step must be finite and in [{QSTEP_MIN}, {QSTEP_MAX}], got {steps.tolist()}")
    if batch is not None and steps32.size not in (1, int(batch)):
        raise ValueError(f"{steps32.size} quantiser steps for a batch of {batch}: give one, or one per image")
    return np.ascontiguousarray(steps32)


def pack_qsteps(steps, inner: bytes) -> bytes:
    steps = check_qsteps(steps)
    return b"".join((QSTEP_MAGIC, struct.pack("<I", steps.size), steps.astype("<f4").tobytes(), bytes(inner)))


def unpack_qsteps(data, batch=None):
    """-> (steps float32 [n], inner stream as a memoryview into ``data``).  ValueError for a wrong magic, a buffer shorter
    than its header states, or invalid steps (check_qsteps, with ``batch`` when the caller knows it)."""
    view = memoryview(data)
    if len(view) < 8 or bytes(view[:4]) != QSTEP_MAGIC:
        raise ValueError("not a quantiser-step container: it does not start with b'BQS1' and a step count")
    (n,) = struct.unpack_from("<I", view, 4)
    if n < 1 or len(view) < 8 + 4 * n:
        raise ValueError(f"truncated quantiser-step container: {n} steps stated, {len(view)} bytes held")
    steps = check_qsteps(np.frombuffer(view[8:8 + 4 * n], dtype="<f4"), batch)
    return steps, view[8 + 4 * n:]
