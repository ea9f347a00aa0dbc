"""Coalesced items on the GPU: N batch-1 items handed to the codec in one call come back as EXACTLY the N byte strings N calls
write, and N such strings decode in one call to exactly the N reconstructions -- for every codec the presets build, through the
harness too (testing_coalesce_items).  The kernels the batched calls take are covered elsewhere; here only the equality matters."""
import pytest
import torch

import codec_cases as cc

pytestmark = pytest.mark.gpu

KINDS = ["hyperprior-fused", "hyperprior-modules", "checkerboard", "basic-l0", "basic-l7", "basic-lanes2", "basic-rows", "basic-combined-l7"]


def _build(kind):
    from cbench_basic_amd.presets import basic_codec, hyperprior_codec, seed_synthetic_weights, topogroup_ar_codec
    if kind.startswith("hyperprior"):
        codec = hyperprior_codec()
    elif kind.startswith("checkerboard"):
        codec = topogroup_ar_codec("checkerboard")
    elif kind == "basic-lanes2":
        codec = basic_codec(stream_lanes=2)
    elif kind == "basic-rows":
        codec = basic_codec(stream_rows=True)
    elif kind.startswith("basic-combined"):
        codec = basic_codec(combined_entropy_coder=True)
    else:
        codec = basic_codec()
    codec = seed_synthetic_weights(codec, seed=0).eval().cuda()
    codec.update_state()
    if kind == "hyperprior-modules":
        codec.entropy_coder.use_fused_session = False
    if kind == "checkerboard-reference":     # one serial stream over the whole batch: nothing to split
        codec.entropy_coder.latent_node_entropy_coders["y"].batch_stream_mode = "reference"
    if kind.startswith("basic"):
        codec.set_complex_level(int(kind[-1]) if kind[-1].isdigit() else 0)
    return codec


def _items():
    """Seven items: five 1 x 3 x 64 x 64 and two 1 x 3 x 64 x 128, interleaved; on the host, as a dataset delivers them."""
    out = []
    for i, wide in enumerate([0, 1, 0, 0, 1, 0, 0]):
        g = torch.Generator().manual_seed(100 + i)
        out.append(torch.rand(1, 3, 64, 128 if wide else 64, generator=g))
    return out


def _check_items_equal_single_calls(codec, kind, calls_all, calls_by_two):
    items = _items()
    want = [codec.compress(x) for x in items]
    want_xhat = [codec.decompress(s) for s in want]
    got = codec.compress_items(items)
    assert codec.last_items_calls == calls_all, (kind, codec.last_items_calls)
    assert [len(s) for s in got] == [len(s) for s in want], kind
    assert got == want, kind                                      # exact bytes, in dataset order
    xhat = codec.decompress_items(want)
    assert codec.last_items_calls == calls_all, (kind, codec.last_items_calls)
    assert len(xhat) == len(items)
    for i, (a, b) in enumerate(zip(xhat, want_xhat)):
        assert a.shape == b.shape and a.shape[0] == 1 and torch.equal(a, b), (kind, i)
    # chunks of at most two; device items
    assert codec.compress_items([x.cuda() for x in items], max_batch=2) == want, kind
    assert codec.last_items_calls == calls_by_two, (kind, codec.last_items_calls)
    xhat = codec.decompress_items(want, max_batch=2)
    assert codec.last_items_calls == calls_by_two, (kind, codec.last_items_calls)
    for i, (a, b) in enumerate(zip(xhat, want_xhat)):
        assert torch.equal(a, b), (kind, i)
    return items, want


@pytest.mark.parametrize("kind", KINDS)
def test_items_keep_their_batch1_bytes_and_reconstructions(kind):
    codec = _build(kind)
    if kind == "hyperprior-fused":
        assert codec.entropy_coder._fused_session({}, None) is not None
    items, want = _check_items_equal_single_calls(codec, kind, calls_all=2, calls_by_two=4)
    if kind == "hyperprior-fused":
        assert codec.entropy_coder.profiler.count["encode_fused"] >= 2 and codec.entropy_coder.profiler.count["decode_fused"] >= 2
    # errors: an item is [1, C, H, W]
    with pytest.raises(ValueError):
        codec.compress_items(items[:2] + [torch.rand(2, 3, 64, 64)])
    with pytest.raises(ValueError):
        codec.compress_items([torch.rand(3, 64, 64)])
    # extra arguments: one call per item, still the same bytes
    if kind == "basic-l7":
        ec = codec.entropy_coder
        node = ec._get_default_node_dict(force_add_default_dynamic_nodes=True)
        extra = {k: v for k, v in node.items() if k.startswith("pgm")}
        assert extra
        assert codec.compress_items(items[:3], **extra) == want[:3]
        assert codec.last_items_calls == 3


def test_reference_stream_mode_falls_back_to_one_call_per_item():
    codec = _build("checkerboard-reference")
    assert not codec.entropy_coder.latent_node_entropy_coders["y"].can_split_items
    _check_items_equal_single_calls(codec, "checkerboard-reference", calls_all=7, calls_by_two=7)


def test_reference_bytes_split_and_decoded_as_items():
    """tests/golden/codec_graph.npz case h1: the REFERENCE's batch-3 string, split into three batch-1 strings, decodes through
    decompress_items to the reference's reconstruction (the bound of tests/test_gpu_codec_graph.py for this case)."""
    from cbench_basic_amd.utils import item_framing as F
    z = cc.load()
    codec, _ = cc.build_codec(z, "h1")
    codec = codec.cuda()
    codec.update_state()
    ref_bytes = z["h1.bytes"].tobytes()
    strings = F.split_codec_string(ref_bytes, 3, [lambda b, n: F.split_compressai_body(b)] * 2)
    assert len(strings) == 3
    xref = torch.from_numpy(z["h1.xhat"])
    for fused in (True, False):
        codec.entropy_coder.use_fused_session = fused
        xhat = codec.decompress_items(strings)
        assert codec.last_items_calls == 1
        xhat = torch.cat(xhat).cpu()
        assert xhat.shape == xref.shape
        assert float((xhat - xref).abs().max()) <= 1e-4 * max(1.0, float(xref.abs().max())), fused
        for i, s in enumerate(strings):
            assert float((codec.decompress(s).cpu() - xref[i:i + 1]).abs().max()) <= 1e-4 * max(1.0, float(xref.abs().max())), (fused, i)
    x = cc.case_input(z, "h1")
    assert codec.compress_items([x[i:i + 1] for i in range(3)]) == strings     # and the items' strings ARE the split reference bytes


# ---------------------------------------------------------------- the harness
def _harness_case(tmp_path, build, items, levels, coalesce, workers=0, metrics="psnr"):
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark, PytorchBatchedDistortion
    codec = build().eval().cuda()    # ONE codec for both passes
    res = {}
    for tag, n, w in (("seq", 0, 0), ("co", coalesce, workers)):
        bench = BasicLosslessCompressionBenchmark(codec, items, distortion_metric=PytorchBatchedDistortion(metrics=metrics),
                                                  testing_complexity_levels=levels, output_dir=str(tmp_path / tag),
                                                  testing_coalesce_items=n, num_testing_workers=w, codec_builder=build if w else None)
        res[tag] = bench.run_benchmark(ignore_exist_metrics=True)
        bench.close()
    seq, co = res["seq"], res["co"]
    assert list(seq) == list(co)
    ends = ("compressed_length", "compression_ratio", "original_length", "psnr", "ms-ssim")
    keys = [k for k in seq if k.endswith(ends)]
    assert len(keys) == (3 + (1 if isinstance(metrics, str) else len(metrics))) * max(1, len(levels))
    for k in keys:     # sizes and distortion are properties of the items, not of the calls that coded them
        print(k, seq[k], co[k])
        assert abs(seq[k] - co[k]) <= 1e-9 * max(1.0, abs(seq[k])), (k, seq[k], co[k])
    assert any(k.endswith("speed_wall_dataset") for k in co)
    return codec


@pytest.mark.parametrize("kind", ["hyperprior", "basic"])
def test_harness_coalesced_pass_equals_sequential(kind, tmp_path):
    from cbench_basic_amd import presets
    build = (lambda: presets.seed_synthetic_weights(presets.hyperprior_codec(), seed=0)) if kind == "hyperprior" else \
            (lambda: presets.seed_synthetic_weights(presets.basic_codec(), seed=0))
    codec = _harness_case(tmp_path, build, _items(), [] if kind == "hyperprior" else [0, 5], coalesce=4)
    assert codec.last_items_calls == 1       # the last chunk of the pass: the two wide items in one call
    from cbench_basic_amd.benchmark import BasicLosslessCompressionBenchmark
    with pytest.raises(ValueError):          # coalescing and dataloader batching do not combine
        BasicLosslessCompressionBenchmark(codec, _items() + [torch.rand(2, 3, 64, 64)], testing_coalesce_items=4).run_benchmark()


def test_harness_coalesced_pass_with_ms_ssim(tmp_path):
    from cbench_basic_amd import presets
    items = []
    for i in range(3):
        g = torch.Generator().manual_seed(200 + i)
        items.append(torch.rand(1, 3, 192, 192, generator=g))
    _harness_case(tmp_path, lambda: presets.seed_synthetic_weights(presets.hyperprior_codec(), seed=0), items, [], coalesce=4,
                  metrics=["psnr", "ms-ssim"])


def test_harness_coalesced_pass_with_workers(tmp_path):
    from cbench_basic_amd import presets
    _harness_case(tmp_path, lambda: presets.seed_synthetic_weights(presets.hyperprior_codec(), seed=0), _items(), [], coalesce=2, workers=2)
