"""The masked convolution (csrc/mconv.hip) against the exact fp64 reference of tests/mconv_exact.py, bit for bit: every kernel that
takes a case is forced in turn (and the library's own choice runs once more), basic_mconv_last_kernel says which kernel really
ran, the operands sit inside NaN guard bands, and every element of x that no listed output reads holds NaN.  Then the coding loop:
the coder's four launches per step on buffers that start as NaN and fill in as coding proceeds, against the chain evaluated once
on the complete latent."""

import numpy as np
import pytest
import torch

import mconv_exact as E

pytestmark = pytest.mark.gpu

KERNELS = (E.GATHER, E.BLOCK, E.DMA)


def _force(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("BASIC_MCONV_KERNEL", raising=False)
    else:
        monkeypatch.setenv("BASIC_MCONV_KERNEL", E.KERNEL_ENV[kernel])


def _choose(c, n_pos=None):
    from cbench_basic_amd.nn import kernels as K
    return K.mconv_choose(c["cin"], c["cout"], c["k"], c["gi"], c["go"], c["B"], c["H"], c["W"], len(c["pos"]) if n_pos is None else n_pos)


def _plan(c):
    from cbench_basic_amd.nn import kernels as K
    return K.MaskedConvPlan(c["w"], c["b"], c["gi"], c["go"], c["same"], c["act"])


def _banded(payload, front, fill):
    """A device buffer of bit patterns: `front` floats of NaN band, the payload (uint32 array), E.BAND floats of NaN band."""
    buf = np.full(front + payload.size + E.BAND, fill, dtype=np.uint32)
    buf[front: front + payload.size] = payload.ravel()
    return torch.from_numpy(buf.view(np.int32)).cuda()


def _dev(a, dtype=None):
    """A device copy of a (read-only) NumPy array."""
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def _dev_i32(a):
    return _dev(a, np.int32)


def _launch(c, plan):
    """One launch of case c with x and out as views at odd offsets inside banded buffers.  -> the out window's bits [B, total, H, W];
    asserts that the bands and x are untouched."""
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    total = cout + E.OUT_CH_BELOW + E.OUT_CH_ABOVE
    xbits = c["x"].view(np.uint32)
    d_x = _banded(xbits, E.X_OFFSET, E.NAN_BAND)
    d_out = _banded(np.full(B * total * H * W, E.NAN_SENTINEL, dtype=np.uint32), E.OUT_OFFSET, E.NAN_BAND)
    x = d_x[E.X_OFFSET: E.X_OFFSET + xbits.size].view(torch.float32).view(B, cin, H, W)
    out = d_out[E.OUT_OFFSET: E.OUT_OFFSET + B * total * H * W].view(torch.float32).view(B, total, H, W)
    call = {}
    if c["step"] is not None:
        call = dict(step=c["step"], first_step=_dev_i32(c["first"]))
    plan(x, _dev_i32(c["topo_in"]), _dev_i32(c["topo_out"]), _dev_i32(c["pos"]), out, out_offset=E.OUT_CH_BELOW,
         in_perm=_dev_i32(c["in_perm"]), out_perm=_dev_i32(c["out_perm"]), **call)
    torch.cuda.synchronize()
    got_x, got = d_x.cpu().numpy().view(np.uint32), d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_x[: E.X_OFFSET], np.full(E.X_OFFSET, E.NAN_BAND)) and np.array_equal(got_x[-E.BAND:], np.full(E.BAND, E.NAN_BAND))
    assert np.array_equal(got_x[E.X_OFFSET: -E.BAND], xbits.ravel()), "x was written"
    assert np.array_equal(got[: E.OUT_OFFSET], np.full(E.OUT_OFFSET, E.NAN_BAND)), "the band in front of out was written"
    assert np.array_equal(got[-E.BAND:], np.full(E.BAND, E.NAN_BAND)), "the band behind out was written"
    return got[E.OUT_OFFSET: -E.BAND].reshape(B, total, H, W)


def _check(c, got, what):
    expected, strict, alt = E.out_image(c)
    bad = strict & (got != expected)
    if bad.any():   # say what kind of wrong: untouched, NaN, which channels and positions, a few values
        g, e = got[bad].view(np.float32), expected[bad].view(np.float32)
        where = np.argwhere(bad)
        raise AssertionError(
            f"{what}: {int(bad.sum())} elements differ from the exact reference, first at {where[0]}; {int((got[bad] == E.NAN_SENTINEL).sum())} "
            f"still hold the sentinel, {int(np.isnan(g).sum())} are NaN; {len(np.unique(where[:, 1]))} channels, "
            f"{len(np.unique(where[:, [0, 2, 3]], axis=0))} positions; got {g[:6]} expected {e[:6]}")
    loose = ~strict
    assert ((got == E.NAN_SENTINEL) | (got == alt))[loose].all(), f"{what}: a listed element outside the step holds a third value"
    win = got[:, E.OUT_CH_BELOW: E.OUT_CH_BELOW + c["cout"]].view(np.float32)
    wrote = win.view(np.uint32) != E.NAN_SENTINEL
    assert not np.isnan(win[wrote]).any(), f"{what}: NaN in the output"


def _run_all_kernels(c, plan, monkeypatch):
    """Every kernel that takes the case when forced, then the library's own choice.  -> {kernel or None: bits}."""
    outs = {}
    for kernel in KERNELS + (None,):
        _force(monkeypatch, kernel)
        predicted = _choose(c)
        if kernel is not None and predicted != kernel:
            assert kernel not in c["kernels"], f"{c['kernels']} were meant to run, {kernel} does not take the case"
            continue
        got = _launch(c, plan)
        assert plan.last_kernel == predicted, f"forced {kernel}: kernel {plan.last_kernel} ran, {predicted} was chosen"
        _check(c, got, f"kernel {kernel}")
        outs[kernel] = got
    _force(monkeypatch, None)
    strict = E.out_image(c)[1]
    for kernel, got in outs.items():
        assert np.array_equal(got[strict], outs[E.GATHER][strict]), f"kernel {kernel} differs from the gather kernel"
    return outs


@pytest.mark.parametrize("name", [n for n in E.SPECS if not n.startswith("block-stale")])
def test_single_launch_is_exact(name, monkeypatch):
    c = E.build_case(name)
    plan = _plan(c)
    assert plan.last_kernel == -1
    outs = _run_all_kernels(c, plan, monkeypatch)
    assert set(c["kernels"]) <= set(outs) and None in outs


def test_block_kernel_leaves_nothing_behind(monkeypatch):
    """One plan, forced block kernel: a launch with 100 open units in 6 tiles, then one with 3 open units in 2 tiles.  Flags or
    scratch partials the first launch left would join the second one's sums."""
    big, small = E.build_case("block-stale-big"), E.build_case("block-stale-small")
    assert big["w"] is small["w"] and len(small["pos"]) < len(big["pos"])
    plan = _plan(big)
    _force(monkeypatch, E.BLOCK)
    for c in (big, small, big):
        got = _launch(c, plan)
        assert plan.last_kernel == E.BLOCK
        _check(c, got, "block kernel")


def test_empty_position_list_is_a_no_op():
    c = E.build_case("all-act0")
    plan = _plan(c)
    x = _dev(c["x_clean"])
    out = torch.full((c["B"], c["cout"], c["H"], c["W"]), -7.0).cuda()
    plan(x, _dev_i32(c["topo_in"]), _dev_i32(c["topo_out"]), torch.empty(0, dtype=torch.int32).cuda(), out)
    torch.cuda.synchronize()
    assert plan.last_kernel == -1 and bool((out == -7.0).all())


def test_refused_calls_raise():
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    c = E.build_case("all-act0")   # 64 -> 128, k = 3
    plan = _plan(c)
    x = _dev(c["x_clean"])
    tin, tout, pos = _dev_i32(c["topo_in"]), _dev_i32(c["topo_out"]), _dev_i32(c["pos"])
    out = torch.full((c["B"], c["cout"] + 2, c["H"], c["W"]), -7.0).cuda()
    perm = _dev_i32(np.arange(c["H"] * c["W"]))
    with pytest.raises(_lib.BasicHipError, match="1x1"):
        plan(x, tin, tout, pos, out, in_perm=perm)
    with pytest.raises(_lib.BasicHipError, match="window"):
        plan(x, tin, tout, pos, out, out_offset=3)
    with pytest.raises(_lib.BasicHipError, match="first-step"):
        _lib.check(_lib.lib().basic_mconv_forward_ex_dev(
            plan._h, x.data_ptr(), tin.data_ptr(), tout.data_ptr(), c["B"], c["H"], c["W"], pos.data_ptr(), pos.numel(), out.data_ptr(),
            out.shape[1], 0, 1, 0, None, None, None, None))
    with pytest.raises(_lib.BasicHipError, match="first-step"):
        _lib.check(_lib.lib().basic_mconv_forward_step_dev(
            plan._h, x.data_ptr(), tin.data_ptr(), tout.data_ptr(), c["B"], c["H"], c["W"], pos.data_ptr(), pos.numel(), out.data_ptr(),
            out.shape[1], 0, 0, None, None))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and plan.last_kernel == -1, "a refused call launched something"
    with pytest.raises(_lib.BasicHipError, match="divide"):
        K.MaskedConvPlan(torch.zeros(10, 6, 1, 1), None, 4, 2, False)
    with pytest.raises(_lib.BasicHipError, match="divide"):
        K.MaskedConvPlan(torch.zeros(10, 6, 1, 1), None, 2, 4, False)
    with pytest.raises(_lib.BasicHipError, match="geometry"):
        K.MaskedConvPlan(torch.zeros(4, 4, 7, 7), None, 1, 1, False)


# ------------------------------------------------------------------------------------------------------------- the coding loop
def _chain_plans(c):
    from cbench_basic_amd.nn import kernels as K
    return [K.MaskedConvPlan(L["w"], L["b"], L["gi"], L["go"], L["same"], L["act"]) for L in c["layers"]]


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _run_chain(c, kernel, monkeypatch):
    """The coder's loop (pgm_coder.py::_context_at, one call per step) with everything the coder leaves uninitialised or zero
    holding NaN.  Asserts what the test's docstring says; -> the kernels that ran, one per launch."""
    from cbench_basic_amd.nn import kernels as K
    C, G, B, H, W = (c[n] for n in "CGBHW")
    C2, HW = 2 * C, H * W
    nan = float("nan")
    dev = dict(device="cuda")
    ybuf = torch.full((B, C, H, W), nan, **dev)
    cat = torch.full((B, 2 * C2, H, W), nan, **dev)
    cat[:, C2:] = _dev(E.planes(c["prior"], c["perm"]))
    hidden = [torch.full((B, 2 * C2, H, W), nan, **dev) for _ in range(2)]
    params = torch.full((B, C2, H, W), nan, **dev)
    topo, tcat, first, hp = (_dev_i32(c[n]) for n in ("topo", "topo_cat", "first", "perm"))
    y = _dev(c["y"])
    plans = _chain_plans(c)
    want = c["params"].view(np.uint32)
    per = C2 // G
    ran = []
    _force(monkeypatch, kernel)
    for step in range(E.CHAIN_STEPS):
        pos_np = E.chain_positions(c, step)
        pos = _dev_i32(pos_np)
        sk = dict(step=step, first_step=first)
        launches = [(plans[0], ybuf, topo, topo, cat, dict(out_offset=0, out_perm=hp)),
                    (plans[1], cat, tcat, tcat, hidden[0], dict(in_perm=hp, out_perm=hp)),
                    (plans[2], hidden[0], tcat, tcat, hidden[1], dict(in_perm=hp, out_perm=hp)),
                    (plans[3], hidden[1], tcat, topo, params, dict(in_perm=hp))]
        for i, (pl, x, tin, tout, out, kw) in enumerate(launches):
            pl(x, tin, tout, pos, out, **kw, **sk)
            L = c["layers"][i]
            predicted = K.mconv_choose(pl.cin, pl.cout, pl.k, L["gi"], L["go"], B, H, W, len(pos_np))
            assert pl.last_kernel == predicted, f"step {step}, layer {i}: kernel {pl.last_kernel} ran, {predicted} was chosen"
            ran.append(pl.last_kernel)
        torch.cuda.synchronize()
        # the parameters of this step's elements, BEFORE the latent they code is known
        now = np.repeat(c["topo"] == step, per, axis=0)[None].repeat(B, axis=0)
        got = _bits(params)
        assert now.any() and np.array_equal(got[now], want[now]), f"step {step}: {int((got[now] != want[now]).sum())} parameters differ"
        coded = torch.from_numpy(np.repeat(c["topo"] == step, C // G, axis=0)[None].repeat(B, axis=0)).cuda()
        ybuf[coded] = y[coded]
    _force(monkeypatch, None)
    assert np.array_equal(_bits(params), want), "a parameter changed after its step"
    assert np.array_equal(_bits(ybuf), c["y"].view(np.uint32))
    for i in range(2):   # the id-less halves: written once, at a position's first step, read at every later one
        got = E.unplanes(hidden[i].cpu().numpy(), c["perm"])[:, C2:]
        assert not np.isnan(got).any(), f"hidden layer {i}: NaN in the id-less half"
        assert np.array_equal(got.view(np.uint32), c["hidden"][i][:, C2:].view(np.uint32)), f"hidden layer {i}: id-less half differs"
    return ran


@pytest.mark.parametrize("kernel", [E.GATHER, E.BLOCK, E.DMA, None], ids=["gather", "block", "dma", "auto"])
@pytest.mark.parametrize("kind", ["checker", "random"])
def test_coding_loop_matches_the_one_shot_reference(kind, kernel, monkeypatch):
    """C = 128, G = 2, two images 12 x 11: every layer qualifies for the LDS-DMA kernel.  After step s the parameters of every (group,
    position) with id s equal the chain evaluated ONCE on the complete latent, bit for bit -- although the latent buffer, the
    context half of cat, both hidden buffers and the parameters started as NaN; at the end every parameter does, and the id-less
    hidden halves are NaN-free and exact.  A forced kernel that does not take a launch falls back to the gather kernel, and
    last_kernel says so."""
    ran = _run_chain(E.chain_case("big", kind), kernel, monkeypatch)
    if kernel in (E.GATHER, E.DMA):
        assert set(ran) == {kernel}
    elif kernel == E.BLOCK:
        assert set(ran) <= {E.BLOCK, E.GATHER} and E.BLOCK in ran


@pytest.mark.parametrize("kind", ["checker", "random"])
def test_coding_loop_block_kernel_serves_every_launch(kind, monkeypatch):
    """C = 32, G = 2, one image 5 x 5: the block kernel takes all sixteen launches."""
    ran = _run_chain(E.chain_case("small", kind), E.BLOCK, monkeypatch)
    assert set(ran) == {E.BLOCK} and len(ran) == 4 * E.CHAIN_STEPS
