"""GPU: the K order of the fp32 tap kernel (conv_tap_mfma_kernel), pinned bit for bit ("K order of the fp32 tap kernel").

The layers of h_a and h_s run this kernel, and their outputs are rounded into symbols and table rows: a decoder must recompute
them to the bit, and an image's bytes must not depend on the batch it is coded in.  So for every plain-activation layer class the
output must be ONE function of the layer and the image:

  a. the 32-channel-slice launch list (BASIC_CONV_DEBUG=4) and the whole-cout list (8) give the same bits;
  b. both are tests/conv_order.py's ordered fp32 chain under the canonical schedule (which order is canonical: a change that
     reorders both lists together fails here);
  c. image i of a batch of 5 is image i coded alone, and image i as the first of a batch of 2 (tile stacking, batch position);
  d. the natural switch between the lists at 384 position blocks changes nothing.

Then the transforms of the presets module against module (debug "", "4", "8"; batch 2 against batch 1), and one end-to-end
statement of the codec's contract through compress_items.  Every comparison is torch.equal: there are no tolerances in this file.
The data are order-sensitive (randn * 2^k, k in -6..6 per element): tests/test_cpu_conv_order.py shows that two stagings differ in
at least a quarter of the outputs of every case, so an order that differs anywhere does not pass by luck."""
import functools

import numpy as np
import pytest
import torch

import conv_order as co

pytestmark = pytest.mark.gpu


def _set_debug(monkeypatch, debug):
    monkeypatch.delenv("BASIC_CONV_F32", raising=False)
    if debug:
        monkeypatch.setenv("BASIC_CONV_DEBUG", debug)
    else:
        monkeypatch.delenv("BASIC_CONV_DEBUG", raising=False)


def _plan_of(layer):
    from cbench_basic_amd.nn import kernels as K
    act = {co.ACT_NONE: K.ACT_NONE, co.ACT_RELU: K.ACT_RELU, co.ACT_LEAKY: K.ACT_LEAKY_RELU}[layer.act]
    return K.ConvPlan(torch.from_numpy(layer.w), torch.from_numpy(layer.b), layer.s, layer.p, layer.op, layer.tr, act, None, None)


def _run(plan, x, monkeypatch, debug):
    _set_debug(monkeypatch, debug)
    out = plan(x.cuda().contiguous())
    torch.cuda.synchronize()
    return out.cpu()


def _differ(a, b):
    bad = a != b
    return f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist() if bad.any() else None}"


@functools.lru_cache(maxsize=None)
def _case(name):
    layer, x = co.case_data(name)
    return layer, torch.from_numpy(x)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The ordered chain of the first REF_BATCH images under the canonical schedule: computed once, shared, never changed."""
    layer, x = _case(name)
    ref = co.ordered_reference(layer, x[:co.REF_BATCH].numpy(), co.canonical_schedule(layer))
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", list(co.CASES))
def test_launch_lists_agree_and_equal_the_ordered_reference(name, monkeypatch):
    """Checks a and b."""
    layer, x = _case(name)
    plan = _plan_of(layer)
    x3 = x[:co.REF_BATCH]
    sliced, whole = _run(plan, x3, monkeypatch, "4"), _run(plan, x3, monkeypatch, "8")
    ref = torch.from_numpy(np.array(_reference(name)))
    for what, got in (("slices", sliced), ("whole", whole)):
        print(f"{name} {what} against the ordered reference: {_differ(got, ref)}")
    print(f"{name} slices against whole: {_differ(sliced, whole)}")
    assert torch.equal(sliced, whole), f"{name}: the two launch lists sum in different orders: {_differ(sliced, whole)}"
    assert torch.equal(sliced, ref), f"{name}: not the canonical order: {_differ(sliced, ref)}"
    assert torch.equal(whole, ref)


@pytest.mark.parametrize("name", list(co.CASES))
def test_batch_size_and_position_do_not_matter(name, monkeypatch):
    """Check c, under both launch lists and the natural choice."""
    layer, x = _case(name)
    plan = _plan_of(layer)
    for debug in ("", "4", "8"):
        full = _run(plan, x, monkeypatch, debug)
        if debug == "":
            assert torch.equal(full[:co.REF_BATCH], torch.from_numpy(np.array(_reference(name))))
        for i in range(co.BATCH):
            alone = _run(plan, x[i:i + 1], monkeypatch, debug)
            first_of_two = _run(plan, torch.stack([x[i], x[(i + 1) % co.BATCH]]), monkeypatch, debug)
            assert torch.equal(full[i], alone[0]), f"{name} debug {debug!r} image {i} of 5 / alone: {_differ(full[i], alone[0])}"
            assert torch.equal(full[i], first_of_two[0]), f"{name} debug {debug!r} image {i} of 5 / first of 2"


@pytest.mark.parametrize("size, natural, opposite", [(442, "4", "8"), (444, "8", "4")], ids=["382-blocks-sliced", "386-blocks-whole"])
def test_natural_switch_between_the_launch_lists(size, natural, opposite, monkeypatch):
    """Check d: the ha5 layer at cin 8, cout 128 on either side of the switch (221^2 positions = 382 blocks of 128: slices; 222^2 =
    386: whole), each against its forced opposite.  A plan of 128 channels launches once under either list, so where the switch sits
    is read off a 256-channel plan of the same geometry: one slice family against two chunks."""
    from cbench_basic_amd.nn import kernels as K
    rng = np.random.default_rng(co.seed("switch"))
    w = (rng.standard_normal((128, 8, 5, 5)) / 200 ** 0.5).astype(np.float32)
    b = (rng.standard_normal(128) * 0.1).astype(np.float32)
    plan = _plan_of(co.Layer(w, b, 5, 2, 2, 0, False, co.ACT_RELU))
    probe = K.ConvPlan(torch.zeros(256, 8, 5, 5), None, 2, 2, 0, False, K.ACT_RELU, None, None)
    _set_debug(monkeypatch, "")
    assert (probe.launches(1, 442, 442), probe.launches(1, 444, 444)) == (1, 2)
    assert probe.launches(1, size, size) == (1 if natural == "4" else 2)
    x = torch.from_numpy(co.sensitive((1, 8, size, size), co.seed("switch", size)))
    got = _run(plan, x, monkeypatch, "")
    assert torch.equal(got, _run(plan, x, monkeypatch, natural))
    other = _run(plan, x, monkeypatch, opposite)
    assert torch.equal(got, other), f"{size}: the natural launch list and its opposite differ: {_differ(got, other)}"


# ---------------------------------------------------------------------------------------------------------------------
# the transforms of the presets, module against module


@functools.lru_cache(maxsize=None)
def _codec(kind):
    from cbench_basic_amd.presets import basic_codec, hyperprior_codec, seed_synthetic_weights
    codec = seed_synthetic_weights(hyperprior_codec() if kind == "hyperprior" else basic_codec(), seed=0).eval().cuda()
    codec.update_state()
    if kind == "basic":
        codec.set_complex_level(0)   # the widest level; the modules below are called without a controller: widest too
    return codec


def _module(kind, name):
    ec = _codec(kind).entropy_coder
    return (ec.latent_inference_modules if name in ("x_y", "y_z") else ec.latent_generative_modules)[name]


def _module_input(kind, name):
    mod = _module(kind, name)
    plan = (mod.plans() if kind == "hyperprior" else mod.plans(mod.num_levels() - 1))[0]
    shape = {"x_y": (2, plan.cin, 64, 80), "y_z": (2, plan.cin, 12, 20), "z_y": (2, plan.cin, 12, 20), "y_x": (2, plan.cin, 4, 5)}[name]
    return torch.from_numpy(co.sensitive(shape, co.seed(kind, name)))


def _forward(mod, x, monkeypatch, debug):
    _set_debug(monkeypatch, debug)
    with torch.no_grad():
        out = mod(x.cuda().contiguous())
    torch.cuda.synchronize()
    return out.cpu()


def _check_batch_invariance(mod, x, out, monkeypatch, debug):
    for i in range(2):
        alone = _forward(mod, x[i:i + 1], monkeypatch, debug)
        assert torch.equal(out[i], alone[0]), f"debug {debug!r} image {i}: batch 2 / batch 1: {_differ(out[i], alone[0])}"
    swapped = _forward(mod, x.flip(0), monkeypatch, debug)
    assert torch.equal(out[1], swapped[0]) and torch.equal(out[0], swapped[1]), f"debug {debug!r}: batch position"


@pytest.mark.parametrize("name", ["y_z", "z_y"])
@pytest.mark.parametrize("kind", ["hyperprior", "basic"])
def test_hyper_transforms_one_function_of_the_image(kind, name, monkeypatch):
    """h_a and h_s (N 128, M 192; the mean-scale graph at its widest level, 192 / 288 / 384 channels): bit-identical under the
    natural launch choice, forced slices and forbidden slices, and row i of a batch of 2 is the batch-1 result of image i."""
    mod, x = _module(kind, name), _module_input(kind, name)
    outs = {debug: _forward(mod, x, monkeypatch, debug) for debug in ("", "4", "8")}
    assert bool(torch.isfinite(outs[""]).all())
    for debug in ("4", "8"):
        assert torch.equal(outs[""], outs[debug]), f"{kind} {name}: debug '' / {debug!r}: {_differ(outs[''], outs[debug])}"
    for debug in ("", "4", "8"):
        _check_batch_invariance(mod, x, outs[debug], monkeypatch, debug)


@pytest.mark.parametrize("name", ["x_y", "y_x"])
@pytest.mark.parametrize("kind", ["hyperprior", "basic"])
def test_main_transforms_batch_and_position_invariant(kind, name, monkeypatch):
    """g_a and g_s (GDN / IGDN and split-bf16 layers: one launch list, and an rsq that the CPU does not reproduce): only the batch
    and position invariance."""
    mod, x = _module(kind, name), _module_input(kind, name)
    out = _forward(mod, x, monkeypatch, "")
    assert bool(torch.isfinite(out).all())
    _check_batch_invariance(mod, x, out, monkeypatch, "")


@pytest.mark.parametrize("kind", ["hyperprior", "basic"])
def test_items_coded_together_are_items_coded_alone(kind, monkeypatch):
    """compress_items(items, max_batch = all of them) is one compress() per item, byte for byte; also when the batched call alone
    runs every layer whole-cout (BASIC_CONV_DEBUG=8), which is what a picture of many tiles does to h_a, reached here at 64 x 64."""
    codec = _codec(kind)
    items = [torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(co.seed("item", i))) for i in range(6)]
    _set_debug(monkeypatch, "")
    want = [codec.compress(x) for x in items]
    assert codec.compress_items(items, max_batch=len(items)) == want
    _set_debug(monkeypatch, "8")
    got = codec.compress_items(items, max_batch=len(items))
    _set_debug(monkeypatch, "")
    assert got == want
