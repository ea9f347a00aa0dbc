"""The premises of the exact masked-convolution reference (mconv_exact.py), checked without a GPU: its arithmetic is exact in fp32 in
any order, it has power -- each common mistake changes what it expects --, and the cases of test_gpu_mconv_exact.py reach the kernel
each of them is meant for (basic_mconv_choose is host code: no device needed)."""
import os

import numpy as np
import pytest

import mconv_exact as E


@pytest.fixture(scope="module")
def K():
    from cbench_basic_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from cbench_basic_amd.nn import kernels
    return kernels


def _quarters(a):
    return bool((a * 4 == np.rint(a * 4)).all())


def _integers(a):
    return bool((a == np.rint(a)).all())


def test_single_launch_arithmetic_is_exact_in_fp32():
    """Weights and inputs are small integers, biases quarters, and the sum of the MAGNITUDES of an output's terms stays below
    2^22: every partial sum of any tiling is a multiple of 1/4 that fp32 holds.  No expected output is NaN, although every element
    of x that no listed output reads is; the reference itself gives the same bits with and without the poison."""
    worst = ("", 0.0)
    for name in E.SPECS:
        c = E.build_case(name)
        assert _integers(c["w"]) and np.abs(c["w"]).max() <= 2 and _integers(c["x_clean"]) and np.abs(c["x_clean"]).max() <= 3
        assert c["b"] is None or (_quarters(c["b"]) and np.abs(c["b"]).max() <= 2)
        peak = c["ref"]["peak"]
        worst = max(worst, (name, peak), key=lambda t: t[1])
        assert peak < 2 ** 22, (name, peak)
        out = c["ref"]["out"]
        assert out.dtype == np.float32 and np.isfinite(out).all()
        if c["act"] != E.ACT_LEAKY:
            assert _quarters(out)
        else:
            assert (out < 0).any() and _quarters(out[out >= 0])
        assert np.isnan(c["x"]).any() or c["ref"]["reads"].all()
        assert np.array_equal(np.isnan(c["x"]), ~c["ref"]["reads"])
        again = E.reference(c["w"], c["b"], c["x"], *c["args"])
        listed = E.planes(np.repeat(c["ref"]["needs"] if c["step"] is None else E.reference(c["w"], c["b"], c["x_clean"], *c["args"][:5])["needs"],
                                    c["cout"] // c["go"], axis=1), c["out_perm"])
        assert np.array_equal(again["out"].view(np.uint32)[listed], out.view(np.uint32)[listed]), name   # at every listed position
        expected, strict, _ = E.out_image(c)
        assert (expected != E.NAN_SENTINEL).sum() == c["ref"]["needs"].sum() * (c["cout"] // c["go"])
        assert strict.all() == (c["step"] is None)
    print(f"largest sum of magnitudes: {worst[1]} in {worst[0]}")


def test_leaky_relu_negative_branch_is_one_fp32_product():
    v = np.array([-3.25, -1.0, -0.25, 0.0, 0.25, 7.0])
    got = E.activate(v, E.ACT_LEAKY)
    want = np.array([np.float32(0.01) * np.float32(t) if t <= 0 else np.float32(t) for t in v], dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert float(got[0]) != -3.25 * 0.01    # not the fp64 product
    assert np.array_equal(E.activate(v, E.ACT_RELU), np.maximum(v, 0).astype(np.float32))
    assert np.array_equal(E.activate(v, E.ACT_NONE), v.astype(np.float32))


@pytest.mark.parametrize("size", list(E.CHAINS))
@pytest.mark.parametrize("kind", ["checker", "random"])
def test_chain_arithmetic_is_exact_in_fp32(size, kind):
    """Non-negative sparse layers: LeakyReLU is the identity, every intermediate a non-negative multiple of 1/4 below 2^22."""
    c = E.chain_case(size, kind)
    print(f"{size} / {kind}: intermediates in [{c['lo']}, {c['peak']}]")
    assert c["lo"] >= 0 and c["peak"] < 2 ** 22
    for L in c["layers"]:
        assert _integers(L["w"]) and (L["w"] >= 0).all() and _quarters(L["b"]) and (L["b"] >= 0).all()
    for a in [c["y"], c["prior"], c["ctx"], c["params"]] + c["hidden"]:
        assert _quarters(a) and (a >= 0).all()
    assert c["params"].max() > 16   # the layers are dense enough for the latent to reach the parameters
    topo, first = c["topo"], c["first"]
    assert topo.min() == 0 and topo.max() == E.CHAIN_STEPS - 1 and np.array_equal(first, topo.min(0))
    if kind == "random":   # some 32-position tile of a step's list mixes positions whose group 0 needs the step with others
        mixed = 0
        for s in range(E.CHAIN_STEPS):
            p = E.chain_positions(c, s) % (c["H"] * c["W"])
            need = topo[0].reshape(-1)[p] == s
            mixed += sum(0 < need[i: i + 32].sum() < len(need[i: i + 32]) for i in range(0, len(p), 32))
        assert mixed >= E.CHAIN_STEPS
    else:
        assert sorted(np.unique(topo[1])) == [2, 3]
    for s in range(E.CHAIN_STEPS):
        assert len(E.chain_positions(c, s)) > 0


def _listed(c, r):
    """The expected bits at the elements a launch must write."""
    needs = E.planes(np.repeat(c["ref"]["needs"], c["cout"] // c["go"], axis=1), c["out_perm"])
    return r["out"].view(np.uint32)[needs]


@pytest.mark.parametrize("mistake", ["swap_compare", "pad_open", "mirror", "group_mod"])
def test_reference_notices_a_wrong_operator(mistake):
    """`<` for `<=`, a tap off the edge read from the neighbouring row, a mirrored window, ci % Gi for ci / (Cin / Gi): each changes
    expected values of a 3 x 3 layer with two 7-channel input groups."""
    c = E.build_case("gather-gsin7")
    bad = E.reference(c["w"], c["b"], c["x_clean"], *c["args"], **{mistake: True})
    n = int((_listed(c, bad) != _listed(c, c["ref"])).sum())
    print(f"{mistake}: {n} expected values differ")
    assert n > 0


def test_reference_notices_a_wrong_step_rule():
    """An id-less output group evaluated at every step instead of its position's first: the set of elements a launch must write
    differs.  (The values do not: an id-less group reads id-less inputs only.)  And `<` for `<=` changes the merger's values."""
    c = E.build_case("all-step-idless")
    bad = E.reference(c["w"], c["b"], c["x_clean"], *c["args"], idless_every_step=True)
    good = c["ref"]["needs"]
    assert (bad["needs"] & ~good).any() and not (good & ~bad["needs"]).any()
    idless = (c["topo_out"] < 0)[None]
    assert (good & idless).any() and (good & ~idless).any()
    assert np.array_equal(bad["out"].view(np.uint32), c["ref"]["out"].view(np.uint32))
    swapped = E.reference(c["w"], c["b"], c["x_clean"], *c["args"], swap_compare=True)
    assert (_listed(c, swapped) != _listed(c, c["ref"])).any()
    # the mixed case: some 32-position tile of the list holds positions that need the step and positions that do not
    m = E.build_case("all-step-mixed")
    hw = m["H"] * m["W"]
    for go in range(m["go"]):
        need = m["ref"]["needs"][:, go].reshape(-1)[m["pos"]]
        assert any(0 < need[i: i + 32].sum() < len(need[i: i + 32]) for i in range(0, len(need), 32)), go
    assert hw * m["B"] == len(m["pos"])


# ---------------------------------------------------------------------------------------------------------------- the chooser
def _choose(K, monkeypatch, force, cin, cout, k, gi, go, n_pos, B=8, H=64, W=64):
    if force is None:
        monkeypatch.delenv("BASIC_MCONV_KERNEL", raising=False)
    else:
        monkeypatch.setenv("BASIC_MCONV_KERNEL", force)
    return K.mconv_choose(cin, cout, k, gi, go, B, H, W, n_pos)


def test_chooser_thresholds(K, monkeypatch):
    G, Bk, D = K.MCONV_KERNEL_GATHER, K.MCONV_KERNEL_BLOCK, K.MCONV_KERNEL_DMA
    assert (G, Bk, D) == (E.GATHER, E.BLOCK, E.DMA)
    ch = lambda force, *a, **kw: _choose(K, monkeypatch, force, *a, **kw)
    # block kernel: at most 4096 (tile, unit) pairs -- 64 x 64 tiles x 1 unit = 4096; 17 x 241 tiles = 4097
    assert ch("block", 8, 64 * 32, 1, 1, 1, 64 * 32) == Bk
    assert ch("block", 8, 241 * 32, 1, 1, 1, 17 * 32) == G
    assert ch("block", 8, 241 * 32, 1, 1, 1, 17 * 32 - 32) == Bk
    assert ch("block", 65, 64 * 32, 1, 1, 1, 32 * 32) == Bk and ch("block", 65, 64 * 32, 1, 1, 1, 32 * 32 + 1) == G   # 2 units
    # auto: block below 256 tiles, gather from 256, LDS-DMA from 4096 (where the layer has it)
    assert ch(None, 8, 32, 1, 1, 1, 255 * 32) == Bk and ch(None, 8, 32, 1, 1, 1, 255 * 32 + 1) == G
    assert ch(None, 8, 32, 5, 1, 1, 255 * 32) == G          # 255 tiles x 25 units do not fit the block kernel
    assert ch(None, 64, 128, 1, 1, 1, 1023 * 32) == G and ch(None, 64, 128, 1, 1, 1, 1023 * 32 + 1) == D
    assert ch(None, 64, 96, 1, 1, 1, 8 * 4096) == G         # no LDS-DMA kernel for 96-row groups, whatever the size
    # LDS-DMA kernel: 64-channel input groups, 128-row output groups, at most 64 (tap, input group) slabs, x below 2 GiB
    assert ch("dma", 64 * 64, 128, 1, 64, 1, 5, H=4, W=4) == D
    assert ch("dma", 3 * 64, 128, 5, 3, 1, 5) == G          # 75 slabs
    assert ch("dma", 7 * 64, 128, 3, 7, 1, 5) == D          # 63
    assert ch("dma", 96, 128, 1, 1, 1, 5) == G and ch("dma", 2 * 96, 128, 1, 2, 1, 5) == G and ch("dma", 192, 128, 1, 1, 1, 5) == D
    assert ch("dma", 64, 64, 1, 1, 1, 5) == G and ch("dma", 64, 384, 1, 1, 2, 5) == G and ch("dma", 64, 256, 1, 1, 2, 5) == D
    assert ch("dma", 64, 128, 1, 1, 1, 5, B=2048, H=64, W=64) == G and ch("dma", 64, 128, 1, 1, 1, 5, B=2047, H=64, W=64) == D
    assert ch("gather", 64, 128, 1, 1, 1, 5) == G and ch("gather", 64, 128, 1, 1, 1, 8 * 4096) == G
    assert ch("something", 64, 128, 1, 1, 1, 5) == Bk       # an unknown name forces nothing
    assert ch(None, 64, 128, 1, 1, 1, 0) == K.MCONV_KERNEL_NONE
    with pytest.raises(ValueError):
        ch(None, 64, 128, 7, 1, 1, 5)
    with pytest.raises(ValueError):
        ch(None, 64, 128, 1, 3, 1, 5)


def test_every_case_reaches_the_kernel_it_is_meant_for(K, monkeypatch):
    ran = {k: [] for k in (E.GATHER, E.BLOCK, E.DMA)}
    for name, s in E.SPECS.items():
        c = E.build_case(name)
        args = (c["cin"], c["cout"], c["k"], c["gi"], c["go"], len(c["pos"]), c["B"], c["H"], c["W"])
        for kernel in ran:
            if _choose(K, monkeypatch, E.KERNEL_ENV[kernel], *args) == kernel:
                ran[kernel].append(name)
            else:
                assert kernel not in c["kernels"], (name, kernel)
        assert name.split("-")[0] in ("all", E.KERNEL_ENV[c["kernels"][0]])
        # what the names promise
        gs_in, gs_out = c["cin"] // c["gi"], c["cout"] // c["go"]
        if "units" in s:
            assert c["k"] ** 2 * c["gi"] * -(-gs_in // 64) == s["units"]
        if "slabs" in s:
            assert c["k"] ** 2 * c["gi"] == s["slabs"]
        if "chunks" in s:
            assert -(-len(c["pos"]) // 128) == s["chunks"]
        if "open_units" in s:   # units of one tile whose input group is open for some position
            open_ = ((c["topo_in"] < c["topo_out"][0][None]).reshape(c["gi"], -1)).any(1)
            assert int(open_.sum()) == s["open_units"] and len(c["pos"]) <= 32 * 6
        if name.startswith("gather-rowtiles"):
            assert gs_out % 32 == 0 and gs_out // 32 == int(name[len("gather-rowtiles"):])
    top = E.build_case("dma-top-slab-alone")
    open_ = (top["topo_in"] < top["topo_out"][0][None]).reshape(top["gi"], -1)
    assert open_[:-1, :128].sum() == 0 and open_[-1, :128].all() and open_[:, 128:].any(0).all() and (top["pos"][:128] == np.arange(128)).all()
    last = E.build_case("dma-last-image")
    assert (last["pos"] // (last["H"] * last["W"]) == last["B"] - 1).all() and last["B"] == 3
    print({E.KERNEL_ENV[k]: len(v) for k, v in ran.items()})
    assert len(ran[E.GATHER]) == len(E.SPECS) and len(ran[E.DMA]) >= 20 and len(ran[E.BLOCK]) >= 40


def test_chain_launches_reach_their_kernels(K, monkeypatch):
    """The big chain: every launch is taken by the LDS-DMA kernel when forced; the small chain: by the block kernel."""
    for size, force, kernel in (("big", "dma", E.DMA), ("small", "block", E.BLOCK)):
        for kind in ("checker", "random"):
            c = E.chain_case(size, kind)
            for s in range(E.CHAIN_STEPS):
                n = len(E.chain_positions(c, s))
                for L in c["layers"]:
                    cout, cin, k, _ = L["w"].shape
                    assert _choose(K, monkeypatch, force, cin, cout, k, L["gi"], L["go"], n, c["B"], c["H"], c["W"]) == kernel


def test_fuzz_generator_reaches_every_kernel(K, monkeypatch):
    """test_gpu_conv.py::test_masked_conv_fuzz over its 40 seeds: how many reach the LDS-DMA and the block kernel when forced."""
    reach = {"dma": 0, "block": 0}
    for seed in range(40):
        g = E.fuzz_geometry(seed)
        for force, kernel in (("dma", E.DMA), ("block", E.BLOCK)):
            reach[force] += _choose(K, monkeypatch, force, g["cin"], g["cout"], g["k"], g["gi"], g["go"], g["npos"], g["B"], g["H"], g["W"]) == kernel
    print(reach)
    assert reach["dma"] >= 5 and reach["block"] >= 30
