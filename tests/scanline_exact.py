"""An exact reference for the whole scan-line operator (include/basic_hip.h section 9) at the BaSIC shape: C = 192, a k x k causal
context convolution 192 -> 384 and the merger 768 -> 640 -> 512 -> 384 on cat(ctx, prior), then the Gaussian step.

The layers are overwritten so that ALL arithmetic is exact in fp32 in any summation order: weights are sparse small non-negative
integers, biases, the latent and the prior non-negative multiples of 1/4, the latent in [1, 8] (so the coded latent sym + mu, within
1/2 of it, stays positive).  Every pre-activation is then non-negative -- LeakyReLU is the identity -- and every intermediate a
multiple of 1/4 far below 2^22.  Any kernel, whatever its tiling, summation order or FMA contraction, must produce the integers and
the float bits of the plain NumPy fp64 raster loop below; test_cpu_scanline_exact.py asserts these premises and that the loop
notices a wrong causal window.  The scale table is 0.5 * (1 .. 64), so that a scale (a multiple of 1/4) often equals an entry or lies
exactly halfway between two, and a residual y - mu often lies at k + 1/2: the ties continuous inputs never produce.

The loop is written from the operator's description, not from any kernel:
  * the context layer at position p = (py, px) sums weight[co, ci, dy, dx] * ybuf[ci, py + dy - k/2, px + dx - k/2] over the taps of
    the k x k window whose raster index is strictly earlier than p's and that lie inside the image (zero padding);
  * the merger's 1 x 1 layers see cat(ctx, prior) at p -- context channels first --, LeakyReLU(0.01) after the first two;
  * the last layer's channel 2c is the mean of channel c and 2c + 1 its scale; idx = the FIRST argmin of |float32(scale) -
    float32(table)|, sym = rint(y - mu) (round half to even), ybuf = sym + mu;
  * symbols and table rows leave in coding order, element p * C + c of an image."""
import functools

import numpy as np

C = 192
TABLE = (0.5 * np.arange(1, 65)).astype(np.float32)


def causal_taps(ks):
    """(dy, dx) window offsets (0 .. ks - 1) whose raster index is strictly earlier than the centre's."""
    h = ks // 2
    return [(dy, dx) for dy in range(ks) for dx in range(ks) if dy < h or (dy == h and dx < h)]


def layer_sizes(channels=C):
    c2 = 2 * channels
    return [2 * c2, c2 * 5 // 3, c2 * 4 // 3, c2]   # cat(ctx, prior) -> the merger's layers


def _sparse_rows(rng, rows, cols, fan_in, p_zero, picks=None):
    """[rows, cols]: a row is zero with probability p_zero, the others hold `fan_in` weights of 1 or 2.  The columns are dealt from
    `picks` (a shuffled deck of all columns by default, shuffled again when it runs out), so the inputs are used evenly: no input is
    left without a path to the output by bad luck."""
    w = np.zeros((rows, cols), dtype=np.float64)
    deck = []
    for r in range(rows):
        if rng.random() < p_zero:
            continue
        while len(set(deck[:fan_in])) < fan_in:
            deck = deck[fan_in:] if len(deck) >= fan_in else []
            deck = deck + list(rng.permutation(cols) if picks is None else picks(rng))
        w[r, deck[:fan_in]] = rng.integers(1, 3, size=fan_in)
        deck = deck[fan_in:]
    return w


@functools.lru_cache(maxsize=None)
def exact_params(ks, seed=2024, channels=C):
    """The layers: dict(ctx_w [2C, C, ks, ks], ctx_b [2C], w = [three [out, in]], b = [three [out]]), fp64 holding exact fp32 values.
    A quarter of the context layer's rows are zero, half of the first merger layer's, none of the second's, three in ten of the
    last's (their mean or scale is the bias alone: scales below the table); the others have a fan-in of 2 (context layer: dealt
    evenly over ALL ks * ks taps, the non-causal ones included -- a kernel that reads one of them reads a non-zero weight -- with
    random channels), 2, 1 and 1, with weights 1 or 2.  Denser than this and the scales leave the table; sparser and a single tap
    no longer reaches a coded integer."""
    rng = np.random.default_rng(seed + 1000 * ks)
    c2 = 2 * channels
    sizes = layer_sizes(channels)
    p = dict(ks=ks, channels=channels)
    taps = lambda g: g.integers(0, channels, size=ks * ks) * (ks * ks) + g.permutation(ks * ks)   # every tap once, any channel
    p["ctx_w"] = _sparse_rows(rng, c2, channels * ks * ks, 2, 0.25, picks=taps).reshape(c2, channels, ks, ks)
    p["ctx_b"] = rng.integers(0, 4, size=c2) / 4.0
    p["w"] = [_sparse_rows(rng, sizes[i + 1], sizes[i], (2, 1, 1)[i], (0.5, 0.0, 0.3)[i]) for i in range(3)]
    p["b"] = [rng.integers(0, 8 if i == 2 else 4, size=sizes[i + 1]) / 4.0 for i in range(3)]
    return p


@functools.lru_cache(maxsize=None)
def exact_inputs(B, H, W, seed, channels=C):
    """(y [B, C, H, W] multiples of 1/4 in [1, 8], prior [B, 2C, H, W] multiples of 1/4 in [0, 2]) as float32."""
    rng = np.random.default_rng(seed)
    y = rng.integers(4, 33, size=(B, channels, H, W)) / 4.0
    prior = rng.integers(0, 9, size=(B, 2 * channels, H, W)) / 4.0
    return y.astype(np.float32), prior.astype(np.float32)


def reference(params, y, prior, taps=None, unwritten=None, table=TABLE):
    """The raster loop in fp64.  -> dict(sym, idx int32 [B, H * W * C] in coding order, ybuf float32 [B, C, H, W], and what the CPU
    test looks at: scale, resid fp64 [B, H * W, C], lo / hi = the smallest / largest intermediate, quarter = every intermediate is
    a multiple of 1/4).  `taps` replaces the causal window (a list of (dy, dx)) and `unwritten` what a position holds before it is
    coded (zeros): both only to show that the loop notices a wrong window."""
    ks, ch = params["ks"], params["channels"]
    y, prior = np.asarray(y, dtype=np.float64), np.asarray(prior, dtype=np.float64)
    B, _, H, W = y.shape
    half = ks // 2
    use = np.zeros((ks, ks), dtype=bool)
    for dy, dx in (causal_taps(ks) if taps is None else taps):
        use[dy, dx] = True
    wc = (params["ctx_w"] * use[None, None]).reshape(2 * ch, -1).T   # [C * ks * ks, 2C]
    buf = np.zeros((B, ch, H + 2 * half, W + 2 * half), dtype=np.float64)   # the coded latent inside its zero padding
    if unwritten is not None:
        buf[:, :, half: half + H, half: half + W] = unwritten
    tab = np.asarray(table, dtype=np.float32)
    sym = np.zeros((B, H * W, ch), dtype=np.int32)
    idx = np.zeros((B, H * W, ch), dtype=np.int32)
    scale, resid = np.zeros((B, H * W, ch)), np.zeros((B, H * W, ch))
    lo, hi, quarter = np.inf, -np.inf, True

    def note(v):
        nonlocal lo, hi, quarter
        lo, hi = min(lo, float(v.min())), max(hi, float(v.max()))
        quarter = quarter and bool((v * 4 == np.rint(v * 4)).all())

    for py in range(H):
        for px in range(W):
            p = py * W + px
            x = buf[:, :, py: py + ks, px: px + ks].reshape(B, -1) @ wc + params["ctx_b"]
            note(x)
            x = np.concatenate([x, prior[:, :, py, px]], axis=1)
            for i in range(3):
                x = x @ params["w"][i].T + params["b"][i]
                note(x)
                if i < 2:
                    x = np.where(x > 0, x, 0.01 * x)
            mu, sg = x[:, 0::2], x[:, 1::2]
            d = np.abs(sg.astype(np.float32)[:, :, None] - tab[None, None, :])
            idx[:, p] = np.argmin(d, axis=2)   # the first minimum
            r = y[:, :, py, px] - mu
            q = np.rint(r)                     # round half to even
            sym[:, p] = q.astype(np.int32)
            out = q + mu
            note(out)
            buf[:, :, half + py, half + px] = out
            scale[:, p], resid[:, p] = sg, r
    ybuf = buf[:, :, half: half + H, half: half + W].astype(np.float32)
    return dict(sym=sym.reshape(B, -1), idx=idx.reshape(B, -1), ybuf=np.ascontiguousarray(ybuf), scale=scale, resid=resid,
                lo=lo, hi=hi, quarter=quarter)


@functools.lru_cache(maxsize=None)
def exact_case(ks, B, H, W, seed):
    """(y, prior, reference) of a seeded case: computed once, shared by every test that needs it, never changed."""
    y, prior = exact_inputs(B, H, W, seed)
    ref = reference(exact_params(ks), y, prior)
    for a in (y, prior, ref["sym"], ref["idx"], ref["ybuf"]):
        a.setflags(write=False)
    return y, prior, ref


def install(coder, params):
    """Overwrites every parameter of a context-model coder (scanline_cases._coder("ctxmodel...", C)) with the exact layers and
    gives it the 0.5-step scale table; update_state() must follow (the rANS tables are built from the scale table)."""
    import torch
    cm = coder.topo_group_context_model
    convs = [cm.param_merger_in] + [m for m in cm.param_merger_out if hasattr(m, "weight")]
    assert len(convs) == 3
    done = set()
    with torch.no_grad():
        for conv, w, b in [(cm.context_prediction, params["ctx_w"], params["ctx_b"])] + list(zip(convs, params["w"], params["b"])):
            assert conv.weight.numel() == w.size and conv.bias.numel() == b.size
            conv.weight.copy_(torch.from_numpy(w.astype(np.float32)).reshape(conv.weight.shape))
            conv.bias.copy_(torch.from_numpy(b.astype(np.float32)))
            done.update((id(conv.weight), id(conv.bias)))
    assert all(id(p) in done for p in coder.parameters()), "a parameter of the coder was left random"
    coder.scale_table = torch.from_numpy(TABLE.copy())
