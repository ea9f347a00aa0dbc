"""Skip coding of the hyperprior y coder: the rule's one parameter and the container that carries it (host code only).

``skip_rows = r`` in [0, T], T the rows of the scale table: an element whose table row (what the index kernels write; with a
quantiser step the row of sigma / step) is below r is not coded, and the decoder rebuilds it as symbol 0 (INTEGRATION.md "Skip
coding"; the compaction is the kernels', csrc/entropy.hip).  The coded stream holds neither r nor the steps; ``compress_skip``
wraps it:

    b"BSK1" | uint32 LE skip_rows | uint32 LE n_steps | n_steps float32 LE steps | inner stream

with n_steps = 0 (no quantiser step), 1 (one step for every image) or the batch.  The inner stream is exactly what
``encode(x, skip_rows=, qstep=)`` returned.
"""
import struct

import numpy as np

from .qstep import check_qsteps

SKIP_MAGIC = b"BSK1"
SKIP_TABLE_ROWS = 64   # SCALES_LEVELS of the GaussianConditional coders' scale table


def check_skip_rows(skip_rows, table_rows=SKIP_TABLE_ROWS) -> int:
    """``skip_rows`` as an int in [0, table_rows]; ValueError for anything else (a bool, a float, a sequence, out of range)."""
    if isinstance(skip_rows, bool) or not isinstance(skip_rows, (int, np.integer)):
        raise ValueError(f"skip_rows must be an integer in [0, {table_rows}], got {skip_rows!r}")
    if not 0 <= int(skip_rows) <= int(table_rows):
        raise ValueError(f"skip_rows must be an integer in [0, {table_rows}], got {int(skip_rows)}")
    return int(skip_rows)


def skip_rows_for_sigma(scale_table, sigma) -> int:
    """The number of table entries <= sigma: ``skip_rows`` that skips every element whose row's scale is at most sigma
    ("skip sigma <= 0.3").  0 below the table's first entry, its length from the last entry on."""
    if hasattr(scale_table, "detach"):
        scale_table = scale_table.detach().cpu().numpy()
    table = np.asarray(scale_table, dtype=np.float64).reshape(-1)
    sigma = float(sigma)
    if table.size == 0 or sigma != sigma:
        raise ValueError("skip_rows_for_sigma takes a non-empty scale table and a sigma that is a number")
    return int(np.count_nonzero(table <= sigma))


def pack_skip(skip_rows, steps, inner, table_rows=SKIP_TABLE_ROWS) -> bytes:
    """``steps``: None (no quantiser step) or what check_qsteps accepts."""
    r = check_skip_rows(skip_rows, table_rows)
    steps = np.zeros(0, dtype=np.float32) if steps is None else check_qsteps(steps)
    return b"".join((SKIP_MAGIC, struct.pack("<II", r, steps.size), steps.astype("<f4").tobytes(), bytes(inner)))


def unpack_skip(data, batch=None, table_rows=SKIP_TABLE_ROWS):
    """-> (skip_rows, steps float32 [n] or None, inner stream as a memoryview into ``data``).  ValueError for a wrong magic, a buffer
    shorter than its header states, skip_rows past the table, or invalid steps (check_qsteps, with ``batch`` when known)."""
    view = memoryview(data)
    if len(view) < 12 or bytes(view[:4]) != SKIP_MAGIC:
        raise ValueError("not a skip-coding container: it does not start with b'BSK1', the skip rows and a step count")
    r, n = struct.unpack_from("<II", view, 4)
    if r > table_rows:
        raise ValueError(f"skip-coding container states skip_rows = {r}, the scale table has {table_rows} rows")
    if len(view) < 12 + 4 * n:
        raise ValueError(f"truncated skip-coding container: {n} steps stated, {len(view)} bytes held")
    steps = None if n == 0 else check_qsteps(np.frombuffer(view[12:12 + 4 * n], dtype="<f4"), batch)
    return int(r), steps, view[12 + 4 * n:]
