"""An exact reference for the topo-group masked convolution (include/basic_hip.h section 6), written from the operator's description
in the header comment of csrc/mconv.hip, not from any of its kernels:

    out[b, co, p] = act(bias[co] + sum_{ci, tap} W[co, ci, tap] * x[b, ci, p + tap]
                                     * [ p + tap inside the map  and  topo_in[g_in(ci), p + tap]  (< or <=)  topo_out[g_out(co), p] ])

with g_in(ci) = ci // (Cin / Gi), g_out(co) = co // (Cout / Go), "<=" for allow_same layers; a masked or padded element is NOT READ
(a select, not a product with zero: it may hold NaN); in the coding loop (a `step`) an (output group, position) pair is evaluated
only when its id equals the step, or -- for an id-less (-1) output group -- at the first step that visits the position; in_perm /
out_perm say where position p of a plane of x / out is stored.

The case builders make every sum exact in fp32 IN ANY ORDER: weights and inputs are small signed integers, biases multiples of
1/4, and the sum of the magnitudes of all terms of an output (`peak`) stays far below 2^22, so every partial sum of every tiling is
a multiple of 1/4 that fp32 holds exactly.  The expected output is then unique to the bit.  The negative branch of LeakyReLU is
the single fp32 product float32(0.01) * v of an exact v.  The chain (chain_case: context layer + three merger layers as the coder
drives them) follows scanline_exact.py instead: non-negative sparse layers, so LeakyReLU is the identity and every intermediate is
a non-negative multiple of 1/4.  test_cpu_mconv_exact.py asserts these premises and that the reference notices a wrong operator."""
import functools
import zlib

import numpy as np

from scanline_exact import _sparse_rows

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
GATHER, BLOCK, DMA = 0, 1, 2                       # BASIC_MCONV_KERNEL_*
KERNEL_ENV = {GATHER: "gather", BLOCK: "block", DMA: "dma"}
CLOSED = 9                                          # an input id above every output id the cases use: never open
NAN_BAND = np.uint32(0x7FC0BEEF)                    # guard bands around x and out
NAN_SENTINEL = np.uint32(0x7FC0A5A5)                # what out holds before a launch
NAN_POISON = np.uint32(0x7FC0DEAD)                  # elements of x no listed output reads


def planes(a, perm):
    """[..., H, W] logical (row-major) -> stored: element p of a plane sits at perm[p]."""
    if perm is None:
        return a
    flat = a.reshape(a.shape[:-2] + (-1,))
    out = np.empty_like(flat)
    out[..., perm] = flat
    return out.reshape(a.shape)


def unplanes(a, perm):
    """Stored -> logical: the inverse of planes()."""
    if perm is None:
        return a
    return a.reshape(a.shape[:-2] + (-1,))[..., perm].reshape(a.shape)


def activate(v, act):
    """fp64 exact v -> float32."""
    v32 = v.astype(np.float32)
    if act == ACT_RELU:
        return np.where(v32 > 0, v32, np.float32(0))
    if act == ACT_LEAKY:
        return np.where(v32 > 0, v32, np.float32(0.01) * v32)   # one fp32 product
    return v32


def reference(w, b, x, topo_in, topo_out, same, act=ACT_NONE, pos=None, step=None, first=None, in_perm=None, out_perm=None, *,
              swap_compare=False, pad_open=False, mirror=False, group_mod=False, idless_every_step=False):
    """-> dict(out float32 [B, Cout, H, W] in out's plane order, the whole map evaluated; needs bool [B, Go, H, W] (row-major): the
    (output group, position) pairs a launch over `pos` (flat b * H * W + p; None = all) at `step` must evaluate; reads bool [B, Cin, H,
    W] in x's plane order: the elements some LISTED output reads; peak: the largest sum of |term| over an output, bias included).
    The keyword-only arguments restate common mistakes, only to show that the reference tells them apart: `<` and `<=` swapped,
    a tap off the left / right edge read from the neighbouring row (padding counted as open), the window mirrored, g_in(ci) = ci %
    Gi, and an id-less output group evaluated at every step."""
    w, x = np.asarray(w, dtype=np.float64), np.asarray(x, dtype=np.float64)
    topo_in, topo_out = np.asarray(topo_in), np.asarray(topo_out)
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    Gi, Go, HW, pad = topo_in.shape[0], topo_out.shape[0], H * W, k // 2
    gs_i, gs_o = Cin // Gi, Cout // Go
    assert gs_i * Gi == Cin and gs_o * Go == Cout and w.shape[1] == Cin
    bias = np.zeros(Cout) if b is None else np.asarray(b, dtype=np.float64)
    xl = unplanes(x, in_perm).reshape(B, Cin, HW)
    g_in = np.arange(Cin) % Gi if group_mod else np.arange(Cin) // gs_i
    listed = np.zeros(B * HW, dtype=bool)
    listed[np.arange(B * HW) if pos is None else np.asarray(pos)] = True
    listed = listed.reshape(B, 1, H, W)
    if step is None:
        needs = np.broadcast_to(listed, (B, Go, H, W)).copy()
    else:
        idless = topo_out < 0
        own = (topo_out == step) | (idless & (True if idless_every_step else (np.asarray(first) == step)[None]))
        needs = listed & own[None]
    total, peak = np.zeros((B, Cout, HW)), np.zeros((B, Cout, HW))
    reads = np.zeros((B, Cin, HW), dtype=bool)
    py, px = np.mgrid[0:H, 0:W]
    for ty in range(k):
        for tx in range(k):
            dy, dx = (pad - ty, pad - tx) if mirror else (ty - pad, tx - pad)
            yy, xx = py + dy, px + dx
            flat = (yy * W + xx).ravel()
            inside = (flat >= 0) & (flat < HW) if pad_open else ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).ravel()
            q = np.where(inside, flat, 0)
            xn, tn = xl[:, :, q], topo_in.reshape(Gi, HW)[:, q]
            for go in range(Go):
                c = topo_out[go].reshape(1, HW)
                open_ = ((tn <= c) if bool(same) != swap_compare else (tn < c)) & inside[None]   # [Gi, HW]
                m = open_[g_in]                                                                   # [Cin, HW]
                xm = np.where(m[None], xn, 0.0)                                                  # a select: a closed element is not read
                rows = slice(go * gs_o, (go + 1) * gs_o)
                wt = w[rows, :, ty, tx]
                total[:, rows] += wt @ xm
                peak[:, rows] += np.abs(wt) @ np.abs(xm)
                rd = listed.reshape(B, 1, HW) & m[None]                                          # output p reads neighbour q[p]
                reads[:, :, q[inside]] |= rd[:, :, inside]
    v = total + bias.reshape(1, Cout, 1)
    out = activate(v, act) + np.float32(0)                                                       # no -0
    return dict(out=planes(out.reshape(B, Cout, H, W), out_perm), needs=needs, reads=planes(reads.reshape(B, Cin, H, W), in_perm),
                peak=float((peak + np.abs(bias).reshape(1, Cout, 1)).max()))


# ------------------------------------------------------------------------------------------------------------- single launches
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _specs():
    """name -> the arguments of build_case.  `kernels`: the kernels the case is MEANT for (it runs every kernel that takes it)."""
    S = {}

    def add(name, kernels, cin, cout, k, gi, go, B, H, W, **kw):
        S[name] = dict(kernels=kernels, cin=cin, cout=cout, k=k, gi=gi, go=go, B=B, H=H, W=W, **kw)

    # gather kernel: 1 .. 8 row tiles per output group -> 1, 2, 3, 4 tiles per wave, 1 again at 5 and 7 (3 at 6, 4 at 8)
    for t in range(1, 9):
        add(f"gather-rowtiles{t}", (GATHER,), 8, 64 * t, 1, 2, 2, 1, 3, 3, same=bool(t % 2))
    for gs_out, go in ((1, 4), (33, 2), (40, 3)):       # ragged row tiles, more than one output group
        add(f"gather-gsout{gs_out}", (GATHER,), 6, gs_out * go, 3, 3, go, 2, 4, 5, pos=27)
    for gs_in in (1, 2, 7, 63, 64, 65, 129):            # pair tail, 8-channel unroll tail, short last block
        add(f"gather-gsin{gs_in}", (GATHER,), 2 * gs_in, 24, 3, 2, 2, 1, 4, 4, pos=13, same=bool(gs_in % 2))
    for n in (1, 31, 32, 33):
        add(f"gather-npos{n}", (GATHER,), 6, 10, 3, 2, 1, 1, 6, 7, pos=n)
    # block + reduce kernels: units = taps * input groups * blocks per slab; the reduce kernel reads flags 128 at a time
    for units, (cin, k, gi) in {1: (5, 1, 1), 64: (64, 1, 64), 65: (65, 1, 65), 128: (64 * 65, 1, 64), 129: (129, 1, 129),
                                150: (258, 5, 2)}.items():
        add(f"block-units{units}", (BLOCK,), cin, 40, k, gi, 1, 2, 4, 5, pos=37, units=units)
    for n in (16, 17, 33):                               # exactly n open units of 100 (batches of 16 in the reduce kernel)
        add(f"block-open{n}", (BLOCK,), 100, 8, 1, 100, 1, 1, 3, 4, open_units=n, units=100)
    # the same layer twice on one plan: a large launch with everything open, then fewer tiles with 3 of 100 units open
    add("block-stale-big", (BLOCK,), 100, 40, 1, 100, 1, 2, 6, 7, layer="block-stale", open_units=100, units=100)
    add("block-stale-small", (BLOCK,), 100, 40, 1, 100, 1, 2, 6, 7, layer="block-stale", open_units=3, pos=5, units=100)
    # LDS-DMA kernel: 128 positions per workgroup, 32-channel stages, a 64-bit slab mask, workgroups dealt to 8 XCDs
    for n in (1, 127, 128, 129):
        add(f"dma-npos{n}", (DMA,), 64, 128, 1, 1, 1, 1, 12, 11, pos=n)
    add("dma-chunks9", (DMA,), 64, 512, 1, 1, 2, 5, 16, 16, pos=8 * 128 + 1, chunks=9)
    add("dma-chunks17", (DMA,), 64, 512, 1, 1, 2, 9, 16, 16, pos=16 * 128 + 5, chunks=17)
    for gs_in in (64, 128, 192):
        add(f"dma-gsin{gs_in}", (DMA,), gs_in, 128, 3, 1, 1, 1, 5, 6)
    for gi in (32, 33, 64):
        add(f"dma-slabs{gi}", (DMA,), 64 * gi, 128, 1, gi, 1, 1, 4, 4, slabs=gi)
    add("dma-top-slab-alone", (DMA,), 64 * 64, 128, 1, 64, 1, 1, 12, 11, top_slab_alone=True, slabs=64, chunks=2)
    add("dma-slabs63", (DMA,), 7 * 64, 128, 3, 7, 1, 1, 5, 5, slabs=63)
    add("dma-slabs50", (DMA,), 2 * 64, 128, 5, 2, 1, 1, 5, 5, slabs=50)
    add("dma-last-image", (DMA,), 64, 128, 3, 1, 1, 3, 5, 6, pos=np.arange(60, 90))
    # every kernel
    all3 = (GATHER, BLOCK, DMA)
    add("all-k5-on-2x3", all3, 64, 128, 5, 1, 1, 2, 2, 3)
    add("all-k3-on-1x1", all3, 64, 128, 3, 1, 1, 3, 1, 1, same=True)
    add("all-perms-1x1", all3, 128, 256, 1, 2, 2, 2, 5, 7, same=True, in_perm=True, out_perm=True, pos=60)
    add("all-outperm-k3", all3, 128, 256, 3, 2, 2, 2, 5, 7, out_perm=True, pos=60)
    for act in (ACT_NONE, ACT_RELU, ACT_LEAKY):
        add(f"all-act{act}", all3, 64, 128, 3, 1, 1, 1, 5, 5, act=act)
    add("all-no-bias", all3, 64, 128, 3, 1, 1, 1, 5, 5, act=ACT_LEAKY, bias=False)
    # the step rule in one launch: a tile that mixes positions that need the step with positions that do not; id-less groups
    add("all-step-mixed", all3, 128, 256, 3, 2, 2, 2, 6, 7, step=2, ids=4)
    add("all-step-idless", all3, 256, 512, 1, 4, 4, 2, 6, 7, same=True, step=1, ids=4, idless=2, in_perm=True, out_perm=True,
        act=ACT_LEAKY)
    return S


SPECS = _specs()
X_OFFSET, OUT_OFFSET, BAND = 37, 101, 64      # floats in front of x / out inside their buffers; band floats behind them
OUT_CH_BELOW, OUT_CH_ABOVE = 3, 2             # channels of out outside the layer's window


@functools.lru_cache(maxsize=None)
def layer_weights(layer, cin, cout, k, bias):
    rng = _rng("layer:" + layer)
    w = rng.integers(-2, 3, size=(cout, cin, k, k)).astype(np.float32)
    b = (rng.integers(-8, 9, size=cout) / 4.0).astype(np.float32) if bias else None
    return w, b


@functools.lru_cache(maxsize=None)
def build_case(name):
    """Everything of a seeded case, computed once and never changed: dict(spec entries, w, b, x (poisoned, in its plane order),
    topo_in, topo_out, pos int32, first, in_perm, out_perm, ref = reference(...))."""
    s = dict(SPECS[name])
    rng = _rng(name)
    cin, cout, k, gi, go, B, H, W = (s[n] for n in ("cin", "cout", "k", "gi", "go", "B", "H", "W"))
    HW = H * W
    s.setdefault("same", False), s.setdefault("act", ACT_NONE), s.setdefault("step", None)
    s["w"], s["b"] = layer_weights(s.get("layer", name), cin, cout, k, s.get("bias", True))
    ids = s.get("ids", 5)
    topo_in = rng.integers(-1, ids, size=(gi, H, W))
    topo_out = rng.integers(0, ids, size=(go, H, W))
    if "open_units" in s:       # k = 1, one channel per input group: an input group is a unit, open where its id is below the output's
        topo_out[:] = 5
        topo_in[:] = CLOSED
        for g in rng.choice(gi, size=s["open_units"], replace=False):
            some = rng.random(HW) < 0.3
            some[rng.integers(0, HW)] = True
            topo_in[g].reshape(-1)[some] = 0
    if s.get("top_slab_alone"):  # the first 128 listed positions (one position chunk of the LDS-DMA kernel) see input group 63 alone
        topo_out[:] = 5
        flat = topo_in.reshape(gi, HW)
        flat[:, :128] = CLOSED
        flat[gi - 1, :128] = 0
    if s.get("idless"):          # the merger's maps: the id-less (-1) half after the id'd half, on both sides
        n = s["idless"]
        topo_in[gi - n:] = -1
        topo_in[: gi - n] = rng.integers(0, ids, size=(gi - n, H, W))
        topo_out = topo_in.copy()
    pos = s.get("pos")
    if pos is None:
        pos = np.arange(B * HW)
    elif np.isscalar(pos):
        pos = np.sort(rng.choice(B * HW, size=int(pos), replace=False))
    s["pos"] = np.asarray(pos, dtype=np.int32)
    s["topo_in"], s["topo_out"] = topo_in.astype(np.int32), topo_out.astype(np.int32)
    idd = topo_out[(topo_out >= 0).all(axis=(1, 2))]
    s["first"] = idd.min(axis=0).astype(np.int32) if s["step"] is not None else None
    s["in_perm"] = rng.permutation(HW).astype(np.int32) if s.get("in_perm") else None
    s["out_perm"] = rng.permutation(HW).astype(np.int32) if s.get("out_perm") else None
    x = planes(rng.integers(-3, 4, size=(B, cin, H, W)).astype(np.float32), s["in_perm"])
    args = (s["topo_in"], s["topo_out"], s["same"], s["act"], s["pos"], s["step"], s["first"], s["in_perm"], s["out_perm"])
    s["ref"] = reference(s["w"], s["b"], x, *args)
    s["x_clean"] = x
    s["x"] = np.where(s["ref"]["reads"], x, NAN_POISON.view(np.float32))
    if s["step"] is not None:    # what a listed position that does not need the step may ALSO hold: the value of a plain launch
        s["ref_full"] = reference(s["w"], s["b"], x, *args[:5], None, None, *args[7:])["out"]
    s["args"] = args
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def out_image(c):
    """What the out buffer of case c must hold after a launch, as bit patterns in its plane order: (expected uint32 [B, out_total, H,
    W], strict bool: where the bits must equal `expected`, alt uint32: what the other elements may hold instead of the sentinel --
    listed positions of an output group that does not need the step, which a kernel evaluates when they share a tile with one that
    does)."""
    B, H, W, cout, go = c["B"], c["H"], c["W"], c["cout"], c["go"]
    total = cout + OUT_CH_BELOW + OUT_CH_ABOVE
    expected = np.full((B, total, H, W), NAN_SENTINEL, dtype=np.uint32)
    alt = expected.copy()
    strict = np.ones(expected.shape, dtype=bool)
    win = slice(OUT_CH_BELOW, OUT_CH_BELOW + cout)
    listed = np.zeros(B * H * W, dtype=bool)
    listed[c["pos"]] = True
    listed = planes(np.broadcast_to(listed.reshape(B, 1, H, W), (B, cout, H, W)).copy(), c["out_perm"])
    needs = planes(np.repeat(c["ref"]["needs"], cout // go, axis=1), c["out_perm"])
    bits = c["ref"]["out"].view(np.uint32)
    expected[:, win] = np.where(needs, bits, NAN_SENTINEL)
    strict[:, win] = needs | ~listed
    if c["step"] is not None:
        alt[:, win] = np.where(listed & ~needs, c["ref_full"].view(np.uint32), NAN_SENTINEL)
    return expected, strict, alt


def fuzz_geometry(seed):
    """The random layer / launch geometry of test_gpu_conv.py::test_masked_conv_fuzz (its NumPy draws, in their order)."""
    rng = np.random.default_rng(900 + seed)
    gi, go = int(rng.choice([1, 2, 3, 4, 6])), int(rng.choice([1, 2, 3, 4, 6]))
    cin, cout = gi * int(rng.integers(1, 40)), go * int(rng.integers(1, 40))
    if seed % 2:  # whole 32-row tiles per group: 1..6 tiles -> the 1/2/3/4-tiles-per-wave variants
        cout = go * 32 * int(rng.integers(1, 7))
    if seed % 4 == 3:  # a layer the LDS-DMA kernel takes: 128-row chunks, 32-channel stages (blocks of 64 and a 32 / 96 remainder)
        gi, go = int(rng.choice([1, 2])), int(rng.choice([1, 2]))
        cin, cout = gi * 32 * int(rng.integers(1, 6)), go * 128 * int(rng.integers(1, 3))
    k = int(rng.choice([1, 3, 5]))
    same = bool(rng.integers(0, 2))
    B, H, W = int(rng.integers(1, 4)), int(rng.integers(2, 20)), int(rng.integers(2, 20))
    npos = int(rng.integers(1, B * H * W + 1))
    off = int(rng.choice([0, 3]))
    return dict(gi=gi, go=go, cin=cin, cout=cout, k=k, same=same, B=B, H=H, W=W, npos=npos, off=off)


# ------------------------------------------------------------------------------------------------------------------ the chain
CHAINS = {"big": (128, 2, 2, 12, 11), "small": (32, 2, 1, 5, 5)}   # C, G, B, H, W
CHAIN_STEPS = 4


@functools.lru_cache(maxsize=None)
def chain_case(size, kind):
    """The coder's four launches per coding step (pgm_coder.py::_context_at) on exact layers: a 3 x 3 context layer C -> 2C over G
    channel groups, and the merger cat(ctx, prior) 4C -> 4C -> 4C over 2G groups (the prior half id-less) -> 2C over G groups.
    kind "checker": ids checkerboard + 2 * group; "random": an independent id 0 .. 3 per (group, position).  -> dict(layers,
    topo, topo_cat, first, perm / order, y, prior, and the ONE-SHOT reference: every layer evaluated once on the complete latent --
    ctx, hidden [2], params, all row-major float32)."""
    C, G, B, H, W = CHAINS[size]
    C2 = 2 * C
    rng = _rng(f"chain:{size}:{kind}")
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "checker":
        topo = np.stack([(yy + xx) % 2 + 2 * g for g in range(G)])
    else:
        topo = rng.integers(0, CHAIN_STEPS, size=(G, H, W))
    topo = topo.astype(np.int32)
    topo_cat = np.concatenate([topo, np.full_like(topo, -1)])
    first = topo.min(axis=0).astype(np.int32)
    order = np.argsort(first.reshape(-1), kind="stable")
    perm = np.empty(H * W, dtype=np.int32)
    perm[order] = np.arange(H * W, dtype=np.int32)
    L = [dict(w=_sparse_rows(rng, C2, C * 9, 6, 0.1).reshape(C2, C, 3, 3), gi=G, go=G, same=False, act=ACT_NONE),
         dict(w=_sparse_rows(rng, 2 * C2, 2 * C2, 4, 0.1).reshape(2 * C2, 2 * C2, 1, 1), gi=2 * G, go=2 * G, same=True, act=ACT_LEAKY),
         dict(w=_sparse_rows(rng, 2 * C2, 2 * C2, 3, 0.0).reshape(2 * C2, 2 * C2, 1, 1), gi=2 * G, go=2 * G, same=True, act=ACT_LEAKY),
         dict(w=_sparse_rows(rng, C2, 2 * C2, 3, 0.1).reshape(C2, 2 * C2, 1, 1), gi=2 * G, go=G, same=True, act=ACT_NONE)]
    for layer in L:
        layer["w"] = layer["w"].astype(np.float32)
        layer["b"] = (rng.integers(0, 4, size=layer["w"].shape[0]) / 4.0).astype(np.float32)
    y = (rng.integers(4, 33, size=(B, C, H, W)) / 4.0).astype(np.float32)
    prior = (rng.integers(0, 9, size=(B, C2, H, W)) / 4.0).astype(np.float32)
    maps = [(topo, topo), (topo_cat, topo_cat), (topo_cat, topo_cat), (topo_cat, topo)]
    x, outs, peak, lo = y, [], 0.0, np.inf
    for i, (layer, (tin, tout)) in enumerate(zip(L, maps)):
        r = reference(layer["w"], layer["b"], x, tin, tout, layer["same"], layer["act"])
        peak, lo = max(peak, r["peak"]), min(lo, float(r["out"].min()))
        outs.append(r["out"])
        x = np.concatenate([r["out"], prior], axis=1) if i == 0 else r["out"]
    c = dict(C=C, G=G, B=B, H=H, W=W, layers=L, maps=maps, topo=topo, topo_cat=topo_cat, first=first, perm=perm, order=order, y=y,
             prior=prior, ctx=outs[0], hidden=outs[1:3], params=outs[3], peak=peak, lo=lo)
    for v in [topo, topo_cat, first, perm, order, y, prior] + outs + [a for layer in L for a in (layer["w"], layer["b"])]:
        v.setflags(write=False)
    return c


def chain_positions(c, step):
    """Flat positions (all images) some channel group codes at `step`, ascending: _GroupPlan.positions."""
    hw = c["H"] * c["W"]
    p = np.nonzero((c["topo"] == step).any(axis=0).reshape(-1))[0]
    return (np.arange(c["B"])[:, None] * hw + p[None, :]).reshape(-1).astype(np.int32)
