"""What the scan-line kernel tests share (test_gpu_scanline.py, test_gpu_scanline_wavefront.py, test_gpu_scanline_band.py,
test_gpu_scanline_dispatch.py, scripts/scanline_dispatch_table.py): seeded coders and inputs, and the checks of an encode schedule
of the batched kernel ("wavefront" or "band") against the per-step path of the same coder.  A schedule changes addressing, not
arithmetic: symbols, table rows, the coded latent (float bits) and the bytes must be EQUAL -- no tolerance anywhere -- and
ScanlinePlan.last_kernel() must say that the schedule ran."""
import os

import pytest
import torch

GUARD = 0x7FC0BEEF   # NaN payload of the guard bands
BAND = 4096

# whether the schedule serves B images of an H x W latent, as the library reports it
SCHEDULE_FITS = {"wavefront": lambda sl, B, H, W: sl.wavefront_max(H, W) >= B,
                 "band": lambda sl, B, H, W: sl.band_max(H, W) >= 1}


def _coder(kind, C):
    from cbench_basic_amd.modules.prior_model.prior_coder.pgm_coder import (GaussianChannelGroupMaskConv2DTopoGroupPGMPriorCoder as Coder,
                                                                            TopoGroupDynamicMaskConv2dContextModel as Ctx)
    if kind.startswith("ctxmodel"):   # "ctxmodel", or "ctxmodel-k3" for a 3x3 context window (the masked-convolution plans stop at 5x5)
        ks = int(kind.split("-k")[1]) if "-k" in kind else 5
        c = Coder(in_channels=C, default_topo_group_method="scanline", topo_group_context_model=Ctx(in_channels=C, out_channels=2 * C, kernel_size=ks))
    elif kind == "merger":   # layers that are not whole 32-row tiles
        c = Coder(in_channels=C, default_topo_group_method="scanline")
    elif kind == "merger-expand":
        c = Coder(in_channels=C, default_topo_group_method="scanline", param_merger_expand_bottleneck=True)
    else:
        c = Coder(in_channels=C, use_joint_ar_model_impl=True)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for p in c.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.02))
    c = c.eval().cuda()
    c.update_state()
    return c


_CODERS = {}


def _shared_coder(kind, C):
    """One coder per configuration for the whole run (its weights are seeded: every test sees the same layers)."""
    if (kind, C) not in _CODERS:
        _CODERS[kind, C] = _coder(kind, C)
    c = _CODERS[kind, C]
    c.use_persistent_scanline = True
    c.scanline_encode_schedule = "auto"
    return c


def _inputs(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B, C, H, W, generator=g) * 3).cuda()
    prior = torch.stack([torch.randn(B, C, H, W, generator=g), torch.rand(B, C, H, W, generator=g) * 3 + 0.1], 2).reshape(B, 2 * C, H, W).cuda()
    return y, prior


def _plan_of(coder, C):
    """The coder's ScanlinePlan (built by a tiny raster call if need be)."""
    y, prior = _inputs(1, C, 2, 2, 5)
    coder.use_persistent_scanline = True
    coder.scanline_encode_schedule = "raster"
    coder._run_encode(y, prior)
    sl = coder._layers["scanline"][0]
    sl.check()
    coder.scanline_encode_schedule = "auto"
    return sl


def check_schedule_equals_per_step(schedule, kind, B, H, W, seed):
    C = 192
    coder = _shared_coder(kind, C)
    y, prior = _inputs(B, C, H, W, seed)
    coder.use_persistent_scanline = False
    s0, i0, y0, plan = coder._run_encode(y, prior)
    data0 = coder.encode(y, prior=prior)
    coder.use_persistent_scanline = True
    coder.scanline_encode_schedule = schedule
    s1, i1, y1, _ = coder._run_encode(y, prior)   # (a call the schedule does not fit raises: no case of the tests may)
    sl = coder._layers["scanline"][0]
    sl.check()
    assert SCHEDULE_FITS[schedule](sl, B, H, W)
    assert sl.last_kernel() == schedule, sl.last_kernel()
    ms, mi = int((s0 != s1).sum()), int((i0 != i1).sum())
    my = int((y0.view(torch.int32) != y1.view(torch.int32)).sum())
    print(f"{kind} B={B} {H}x{W} seed {seed} [{schedule}]: symbol diffs {ms}, index diffs {mi}, ybuf bit diffs {my} of {s0.numel()}")
    assert ms == 0 and mi == 0 and my == 0
    data1 = coder.encode(y, prior=prior)
    assert sl.last_kernel() == schedule, sl.last_kernel()
    sl.check()
    assert data1 == data0
    yhat = coder.decode(data1, prior=prior)
    sl.check()
    assert torch.equal(yhat.view(torch.int32), y1.view(torch.int32))


def check_refused_on_the_host(schedule, kind, C, B, H, W):
    """A call the schedule does not fit: the library's *_max says so and a forced call fails before any launch."""
    coder = _shared_coder(kind, C)
    sl = _plan_of(coder, C)
    before = sl.last_kernel()
    assert before in ("generic", "pipelined", "batched")
    assert not SCHEDULE_FITS[schedule](sl, B, H, W)
    y, prior = _inputs(B, C, H, W, 6)
    sl.set_encode_schedule(schedule)
    try:
        with pytest.raises((RuntimeError, ValueError), match="does not fit"):
            sl.encode(y, prior, coder._scale_table_dev)
    finally:
        sl.set_encode_schedule("auto")
    assert sl.last_kernel() == before   # no launch was made


def check_guard_bands(schedule, B, H, W):
    """sym, idx and ybuf as views into sentinel-filled buffers: the schedule's launches write all of each view and nothing else."""
    from cbench_basic_amd import _lib
    from cbench_basic_amd.nn import kernels as K
    C = 192
    coder = _shared_coder("ctxmodel", C)
    sl = _plan_of(coder, C)
    y, prior = _inputs(B, C, H, W, 77 + B)
    coder.use_persistent_scanline = False
    s0, i0, y0, _ = coder._run_encode(y, prior)
    coder.use_persistent_scanline = True
    table = coder._scale_table_dev.to(device="cuda", dtype=torch.float32).contiguous()
    n = B * H * W * C
    off = 64
    bufs = [torch.full((off + n + BAND,), GUARD, dtype=torch.int32, device="cuda") for _ in range(3)]
    for b in bufs:
        b[off: off + n] = 0x7FC00001   # (a NaN as float, no symbol or table row as integer)
    sym, idx, ybuf = (b[off: off + n] for b in bufs)
    sl.set_encode_schedule(schedule)
    try:
        _lib.check(_lib.lib().basic_scanline_encode_dev(sl._h, y.data_ptr(), prior.data_ptr(), B, H, W, table.data_ptr(), table.numel(),
                                                        sym.data_ptr(), idx.data_ptr(), ybuf.data_ptr(), K._stream()))
        sl.check()
    finally:
        sl.set_encode_schedule("auto")
    assert sl.last_kernel() == schedule
    for name, b in zip(("sym", "idx", "ybuf"), bufs):
        h = b.cpu()
        assert bool((h[:off] == GUARD).all()) and bool((h[off + n:] == GUARD).all()), f"the launch wrote outside {name}"
    assert torch.equal(sym.view(B, -1), s0) and torch.equal(idx.view(B, -1), i0)
    assert torch.equal(ybuf.view(B, C, H, W), y0.view(torch.int32))


def check_codec_level(schedule, level, shape):
    """BaSIC on images of `shape`: the raster schedule and `schedule` write the same bytes, which decompress to the same images."""
    from cbench_basic_amd.presets import basic_codec, seed_synthetic_weights
    codec = seed_synthetic_weights(basic_codec(), seed=0).eval().cuda()
    codec.update_state()
    codec.set_complex_level(level)
    yc = codec.entropy_coder.latent_node_entropy_coders["y"]
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(11)).cuda()
    yc.scanline_encode_schedule = "raster"
    raster = codec.compress(x)
    sl = yc._layers["scanline"][0]
    sl.check()
    assert sl.last_kernel() in ("generic", "pipelined", "batched")
    x_raster = codec.decompress(raster)
    yc.scanline_encode_schedule = schedule
    other = codec.compress(x)
    sl = yc._layers["scanline"][0]
    sl.check()
    assert sl.last_kernel() == schedule, sl.last_kernel()
    assert other == raster
    x_other = codec.decompress(other)
    assert torch.equal(x_raster, x_other)


# ---- the dispatch table (tests/golden/scanline_dispatch.json, written by scripts/scanline_dispatch_table.py): which kernel serves a call
DISPATCH_FIELDS = ("kind", "C", "batch", "H", "W", "direction", "schedule", "env")
STREAM_FIELDS = DISPATCH_FIELDS + ("lanes", "rows")   # its `streams` section: decode calls over lane and row streams, asked of choose alone


def dispatch_plan(coder, sl, shapes):
    """A coder's entry of the table's `plans` section: the layer sizes its ScanlinePlan was made of, the coder's table length and
    gate, and what the library reports of the plan -- basic_scanline_plan_info, and per (H, W) of `shapes` the batched kernel's
    largest batch (encode, decode), the wavefront's, and the band's images per launch.  `batched` and `tile_workgroups` (the
    workgroups of one column tile of the batched family: the context layer's 32-row tiles plus the largest dense layer's) are
    not reported by any entry: the first is what batched_max says of a wide latent, the second is restated here from the layers."""
    layers = sl.layer_sizes
    batched = sl.batched_max(64) > 0
    return dict(layers=layers, table_len=int(coder._scale_table_dev.numel()), lane_max_batch=int(coder.persistent_scanline_max_batch),
                workgroups=sl.workgroups, lds_weight_bytes=sl.lds_weight_bytes, batched=batched,
                tile_workgroups=layers["ctx_out"] // 32 + max(r // 32 for r in layers["dense_out"]) if batched else 0,
                limits=[[H, W, sl.batched_max(W), sl.batched_max(W, decode=True), sl.wavefront_max(H, W), sl.band_max(H, W)] for H, W in shapes])


def dispatch_stream(coder, row, cache):
    """(y, prior, bytes) of a row's shape: the inputs are seeded by the shape, the bytes coded once with the coder's defaults."""
    key = (row["kind"], row["C"], row["batch"], row["H"], row["W"])
    if key not in cache:
        y, prior = _inputs(row["batch"], row["C"], row["H"], row["W"], 1000 * row["batch"] + 10 * row["H"] + row["W"])
        os.environ.pop("BASIC_SCAN_KERNEL", None)
        coder.use_persistent_scanline = True
        coder.scanline_encode_schedule = "auto"
        cache[key] = (y, prior, coder.encode(y, prior=prior))
    return cache[key]


def dispatch_choose(coder, sl, row):
    """What ScanlinePlan.choose says about a row's call: (the outcome in the table's words, the launches); launches nothing."""
    if row["env"]:
        os.environ["BASIC_SCAN_KERNEL"] = row["env"]
    try:
        kernel, launches = sl.choose(row["batch"], row["H"], row["W"], coder._scale_table_dev.numel(), row["schedule"], coder.persistent_scanline_max_batch,
                              coder._tables if row["direction"] == "decode" else None, lanes=row.get("lanes", 1), rows=row.get("rows", False))
    except (RuntimeError, ValueError) as e:
        if "does not fit" not in str(e):
            raise
        return "raises", 0
    finally:
        os.environ.pop("BASIC_SCAN_KERNEL", None)
    return kernel or "per-step", launches


def dispatch_run(coder, row, cache):
    """Runs a row's call through the coder -> "per-step" (nothing is run), "raises" (a refusal: "does not fit") or the kernel's name."""
    y, prior, data = dispatch_stream(coder, row, cache)
    decode = row["direction"] == "decode"
    coder.use_persistent_scanline = True
    coder.scanline_encode_schedule = row["schedule"]
    if row["env"]:
        os.environ["BASIC_SCAN_KERNEL"] = row["env"]
    try:
        plan = coder._plans_for(row["H"], row["W"], None, row["batch"])
        sl = coder._scanline_plan(plan, prior, row["batch"], decode=decode, width=row["W"], height=row["H"])
        if sl is None:
            return "per-step"
        if decode:
            coder.decode(data, prior=prior)
        else:
            coder._run_encode(y, prior)
        sl.check()
        return sl.last_kernel()
    except (RuntimeError, ValueError) as e:
        if "does not fit" not in str(e):
            raise
        return "raises"
    finally:
        os.environ.pop("BASIC_SCAN_KERNEL", None)
        coder.scanline_encode_schedule = "auto"
