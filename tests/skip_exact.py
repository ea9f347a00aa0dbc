"""NumPy restatement of skip coding (INTEGRATION.md "Skip coding"), what the GPU tests compare the kernels and the codec against.

keep = idx >= r; a stream's compaction is boolean indexing (order kept); seg is the running sum of the kept counts; expansion
scatters a stream's run back to the kept positions and writes 0 elsewhere; the container is
b"BSK1" | uint32 LE skip_rows | uint32 LE n_steps | n_steps float32 LE | inner stream."""
import struct

import numpy as np


def keep_mask(idx, r):
    return np.asarray(idx) >= int(r)


def compact(sym, idx, nstreams, r):
    """Dense int32 arrays of ``nstreams`` equal streams -> (sym_c or None, idx_c, seg int64 [nstreams + 1]); only the kept
    elements come back (seg[-1] of them), stream after stream."""
    idx = np.asarray(idx, dtype=np.int32).reshape(nstreams, -1)
    keep = keep_mask(idx, r)
    seg = np.zeros(nstreams + 1, dtype=np.int64)
    np.cumsum(keep.sum(1), out=seg[1:])
    idx_c = np.concatenate([idx[s][keep[s]] for s in range(nstreams)]).astype(np.int32)
    sym_c = None
    if sym is not None:
        sym = np.asarray(sym, dtype=np.int32).reshape(nstreams, -1)
        sym_c = np.concatenate([sym[s][keep[s]] for s in range(nstreams)]).astype(np.int32)
    return sym_c, idx_c, seg


def expand(sym_c, idx, nstreams, r):
    """The inverse: int32 [nstreams][per], the j-th kept element of stream s = sym_c[seg[s] + j], every skipped one 0."""
    idx = np.asarray(idx, dtype=np.int32).reshape(nstreams, -1)
    keep = keep_mask(idx, r)
    out = np.zeros(idx.shape, dtype=np.int32)
    out[keep] = np.asarray(sym_c, dtype=np.int32)[: int(keep.sum())]   # row-major boolean scatter = stream after stream, in order
    return out


def streams(sym_c, idx_c, seg):
    """The (symbols, indexes) of every stream of a compaction."""
    return [(sym_c[seg[s]:seg[s + 1]], idx_c[seg[s]:seg[s + 1]]) for s in range(len(seg) - 1)]


def pack(skip_rows, steps, inner):
    steps = np.zeros(0, np.float32) if steps is None else np.asarray(steps, dtype=np.float32).reshape(-1)
    return b"BSK1" + struct.pack("<II", int(skip_rows), steps.size) + steps.astype("<f4").tobytes() + bytes(inner)


def unpack(data):
    data = bytes(data)
    assert data[:4] == b"BSK1"
    r, n = struct.unpack_from("<II", data, 4)
    steps = np.frombuffer(data[12:12 + 4 * n], dtype="<f4").copy() if n else None
    return r, steps, data[12 + 4 * n:]
