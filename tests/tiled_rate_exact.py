"""The joint step choice of a tiled picture restated in NumPy (INTEGRATION.md "Tiled pictures: step and byte budget"), on top of
tests/rate_exact.py: the select rule over GROUPS of tiles, and the curve -> select -> refine loop with groups in the place of images.
No library of the project is behind any of it.

    pred(g, k) = sum over the tiles t of group g of (4 extra[t] + sum over the lanes l of 4 (2 + ((bits[first[t] + l][k] + 4 per_seg[t]) >> 21)))
    choice[g]  = the first k in candidate order with pred(g, k) <= budget[g];  none: (K - 1) | NO_FIT, the largest step
"""
import numpy as np

import rate_exact as RX

NO_FIT = RX.NO_FIT


def tile_pred(bits, first_seg, lanes, per_seg, extra_words, k):
    """The byte bound of one tile at candidate k, in Python integers."""
    return 4 * int(extra_words) + sum(RX.stream_bound(bits[first_seg + l][k], per_seg) for l in range(lanes))


def select_groups(bits, tile_first_seg, lanes, tile_per_seg, tile_extra_words, groups, cand, budgets):
    """-> (steps float32 [G], choice int32 [G], pred int64 [G], tile_steps float32 [T], tile_pred int64 [T]).  ``groups``: a list of
    lists of tile numbers; ``cand`` [K] or [G][K].  A tile in no group keeps step 1 and prediction 0."""
    bits = [[int(v) for v in row] for row in np.asarray(bits)]
    cand = np.asarray(cand, dtype=np.float32)
    T, G, K = len(tile_first_seg), len(groups), cand.shape[-1]
    extra = [0] * T if tile_extra_words is None else [int(v) for v in tile_extra_words]
    steps, choice, preds = np.zeros(G, np.float32), np.zeros(G, np.int32), np.zeros(G, np.int64)
    tile_steps, tile_preds = np.ones(T, np.float32), np.zeros(T, np.int64)
    for g, members in enumerate(groups):
        c = cand if cand.ndim == 1 else cand[g]
        pick = None
        for k in range(K):
            pred = sum(tile_pred(bits, int(tile_first_seg[t]), lanes, int(tile_per_seg[t]), extra[t], k) for t in members)
            if pred <= int(budgets[g]):
                pick = k
                break
        k = K - 1 if pick is None else pick
        choice[g] = (k | NO_FIT) if pick is None else k
        steps[g], preds[g] = c[k], pred
        for t in members:
            tile_steps[t] = c[k]
            tile_preds[t] = tile_pred(bits, int(tile_first_seg[t]), lanes, int(tile_per_seg[t]), extra[t], k)
    return steps, choice, preds, tile_steps, tile_preds


def steps_groups(chunks, groups, budgets, tile_extra_words, cand0, passes, lanes, scale_table, bound, table, sizes, offsets, bprec=4):
    """The whole loop.  ``chunks``: a list of (y, sigma) float32 arrays [B_c][n_c], one per pooled coding call; the tiles are numbered
    through the chunks in order, tile t owns rows t * lanes .. of the curve tensor.  -> (steps, choice, pred, tile_steps, tile_pred,
    trace), ``trace`` the list of every pass's (candidates, bits, choice)."""
    first_seg, per_seg, tile_group = [], [], {}
    for y, _ in chunks:
        B, n = y.shape[0], y[0].size
        assert n % lanes == 0
        for _ in range(B):
            first_seg.append(len(per_seg) * lanes)
            per_seg.append(n // lanes)
    for g, members in enumerate(groups):
        for t in members:
            tile_group[t] = g
    cand, trace = np.asarray(cand0, dtype=np.float32), []
    for p in range(passes):
        if p:
            cand = RX.refine(cand, choice, len(groups))
        rows, t0 = [], 0
        for y, sigma in chunks:
            B, n = y.shape[0], y[0].size
            mine = cand if cand.ndim == 1 else np.stack([cand[tile_group[t0 + j]] for j in range(B)])
            rows.append(RX.rate_curve(y.reshape(B, n), sigma.reshape(B, n), B * lanes, n // lanes, lanes, mine, scale_table, bound, table,
                                      sizes, offsets, bprec))
            t0 += B
        bits = np.concatenate(rows)
        steps, choice, pred, tile_steps, tile_preds = select_groups(bits, first_seg, lanes, per_seg, tile_extra_words, groups, cand, budgets)
        trace.append((cand, bits, choice))
    return steps, choice, pred, tile_steps, tile_preds, trace
