"""GPU parity of the full hyperprior codec (BASELINE configs[0]/[1] graph) against the CPU oracle:
  * transforms within 1e-4 (relative to tensor scale) of the fp32 CPU reference ops,
  * integer symbols / indexes: mismatch count reported; where they agree the bytes are identical,
  * decode(encode(x)) on the GPU reproduces the oracle's reconstruction, PSNR within 0.01 dB.
"""
import math
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    from oracle.codec_oracle import HyperpriorOracle
    codec = seed_synthetic_weights(hyperprior_codec(), seed=0).eval()
    oracle = HyperpriorOracle(codec.entropy_coder.state_dict())
    codec = codec.to("cuda:0")
    codec.update_state()
    return codec, oracle


def _rel(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def test_tables_match_oracle(setup):
    codec, oracle = setup
    ec = codec.entropy_coder
    zc, yc = ec.latent_node_entropy_coders["z"], ec.latent_node_entropy_coders["y"]
    for got, ref in ((zc._cdf_host, oracle.eb[:3]), (yc._cdf_host, oracle.gc)):
        for g, r in zip(got, ref):
            assert np.array_equal(g, r)
    assert np.array_equal(zc._tables.get_cdfs(), oracle.eb[0][:, : oracle.eb[1].max()])
    # GaussianConditional table shape facts (CompressAI): 64 rows, centre = ceil(sigma * 6.1094)
    assert oracle.gc[0].shape[0] == 64 and oracle.gc[2][0] == -1 and oracle.gc[1][0] == 5


@pytest.mark.parametrize("shape", [(1, 3, 64, 64), (2, 3, 128, 96), (1, 3, 256, 256),
                                   (1, 3, 256, 64), (2, 3, 192, 64)])   # the last two: tall pictures (g_a layer 3 at 64 x 16 and 48 x 16)
def test_transforms_and_symbols(setup, shape):
    codec, oracle = setup
    ec = codec.entropy_coder
    torch.manual_seed(shape[2])
    x = torch.rand(*shape)
    a = oracle.analyse(x)
    xg = x.cuda()
    y = ec.latent_inference_modules["x_y"](xg)
    z = ec.latent_inference_modules["y_z"](y)
    assert _rel(y.cpu(), a["y"]) < 1e-4
    assert _rel(z.cpu(), a["z"]) < 1e-4
    zhat = ec.latent_node_entropy_coders["z"](z)
    scales = ec.latent_generative_modules["z_y"](zhat)
    z_mis = int((zhat.cpu() != a["z_hat"]).sum())
    if z_mis == 0:
        assert _rel(scales.cpu()[..., : y.shape[-2], : y.shape[-1]], a["scales"]) < 1e-4
    from cbench_basic_amd.nn import kernels as K
    yc = ec.latent_node_entropy_coders["y"]
    yc._ready()
    sym, idx, _ = K.gc_quantize_index(y, scales[..., : y.shape[-2], : y.shape[-1]].contiguous(), yc._scale_table_dev)
    y_mis = int((sym.cpu() != a["y_sym"]).sum())
    i_mis = int((idx.cpu() != a["y_idx"]).sum())
    n = a["y_sym"].numel()
    print(f"symbol mismatches vs fp32 CPU reference: z {z_mis}/{a['z_sym'].numel()}, y {y_mis}/{n}, idx {i_mis}/{n}")
    # Differences may only be fp32 rounding TIES between the MFMA and the torch-CPU summation orders: every differing element
    # is located and must sit within 2e-4 of a decision boundary of the ORACLE's own values (a half-integer latent for a
    # symbol, a scale-table entry for an index), and there may be at most 2 of each.
    assert y_mis <= 2 and i_mis <= 2 and z_mis <= 2
    if z_mis == 0:
        yo, so = a["y"].reshape(-1), a["scales"].reshape(-1)
        for e in torch.nonzero(sym.cpu().reshape(-1) != a["y_sym"].reshape(-1)).reshape(-1).tolist():
            frac = abs(float(yo[e]) - math.floor(float(yo[e])) - 0.5)
            assert frac < 2e-4, (e, float(yo[e]))
        table = yc.scale_table.cpu()
        for e in torch.nonzero(idx.cpu().reshape(-1) != a["y_idx"].reshape(-1)).reshape(-1).tolist():
            sv = max(float(so[e]), 0.11)
            assert float((table - sv).abs().min()) < 2e-4 * max(1.0, sv), (e, sv)
    # the oracle's reconstruction from ITS symbols vs ours from OURS
    xhat_ref = oracle.g_s(a["y_sym"].float())
    xhat = ec.latent_generative_modules["y_x"](sym.float())
    if y_mis == 0:
        assert _rel(xhat.cpu(), xhat_ref) < 1e-4


@pytest.mark.parametrize("shape", [(1, 3, 64, 64), (3, 3, 64, 96), (2, 3, 192, 128), (5, 3, 64, 64), (1, 3, 128, 256), (4, 3, 128, 64),
                                   (1, 3, 70, 93), (2, 3, 129, 67),    # these two: sizes no layer divides evenly
                                   (1, 3, 256, 64), (2, 3, 192, 64)])  # tall pictures: column-shaped conv tiles
def test_compress_decompress_vs_oracle(setup, shape):
    from oracle.codec_oracle import psnr
    codec, oracle = setup
    torch.manual_seed(7)
    x = torch.rand(*shape)
    data = codec.compress(x)
    assert isinstance(data, bytes)
    ref = oracle.compress(x)
    xhat = codec.decompress(data)
    xref = oracle.decompress(ref)
    # sizes a stride-2 layer does not divide come back LARGER (4 x "2n" of ceil(n / 16)), as from the reference, which does not crop
    # either (the distortion metric does, pytorch_distortion.py:12-15)
    assert xhat.shape == xref.shape and xhat.is_cuda and (xhat.shape == x.shape or (shape[2] % 16 or shape[3] % 16))
    # cross decoding: the oracle decodes OUR stream to (nearly) our reconstruction
    xcross = oracle.decompress(data)
    assert _rel(xhat.cpu(), xcross) < 1e-3
    crop = lambda t: t[..., : shape[2], : shape[3]]
    assert float((psnr(crop(xhat.cpu()), x) - psnr(crop(xref), x)).abs().max()) < 0.01
    a = oracle.analyse(x)
    # byte-identical to the CPU oracle, or every difference is a located fp32 rounding tie (printed with -s)
    flips = _assert_identical_or_located_ties(codec, oracle, x, data, ref, a, f"shape {shape}")
    if flips == 0:
        assert _rel(xhat.cpu(), xref) < 1e-4
    (nz,) = struct.unpack("I", data[:4])
    assert struct.unpack(">3I", data[4:16]) == (a["z"].shape[-2], a["z"].shape[-1], shape[0])


def test_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


def _entropy_stage_inputs(codec, x):
    """The integer (symbols, indexes) the GPU codec hands to rANS for y, recomputed stage by stage."""
    from cbench_basic_amd.nn import kernels as K
    ec = codec.entropy_coder
    y = ec.latent_inference_modules["x_y"](x.cuda())
    z = ec.latent_inference_modules["y_z"](y)
    zhat = ec.latent_node_entropy_coders["z"](z)
    scales = ec.latent_generative_modules["z_y"](zhat)[..., : y.shape[-2], : y.shape[-1]].contiguous()
    yc = ec.latent_node_entropy_coders["y"]
    yc._ready()
    sym, idx, _ = K.gc_quantize_index(y, scales, yc._scale_table_dev)
    return y.cpu(), scales.cpu(), sym.cpu(), idx.cpu()


def _assert_identical_or_located_ties(codec, oracle, x, data, ref, a, tag, max_flips=2):
    """data == ref byte for byte, EXCEPT for fp32 rounding ties between the MFMA and the torch-CPU summation orders:
    every differing symbol / index is located and shown to be a tie (y within 2e-4 of a rounding boundary, or the scale
    within 2e-4 relative of a table threshold), at most max_flips of them, and the rANS layer is then shown exact on the
    oracle's own integers.  Returns the number of flips (0 = identical)."""
    from cbench_basic_amd import ans
    if data == ref:
        return 0
    y, scales, sym, idx = _entropy_stage_inputs(codec, x)
    flips_s = (sym != a["y_sym"]).nonzero()
    flips_i = (idx != a["y_idx"]).nonzero()
    z_same = bool((codec.entropy_coder.latent_node_entropy_coders["z"](
        codec.entropy_coder.latent_inference_modules["y_z"](codec.entropy_coder.latent_inference_modules["x_y"](x.cuda()))).cpu()
        == a["z_hat"]).all())
    print(f"{tag}: streams differ; symbol flips {len(flips_s)}, index flips {len(flips_i)} of {sym.numel()}, z identical {z_same}")
    assert z_same, "a z symbol flipped: the scales of the whole image differ, not a single tie"
    assert 0 < len(flips_s) + len(flips_i) <= max_flips, "streams differ without a located symbol / index flip"
    for f in flips_s:
        v = float(a["y"][tuple(f)])
        print(f"  symbol flip at {tuple(int(i) for i in f)}: y = {v!r} (oracle) vs {float(y[tuple(f)])!r} (GPU)")
        assert abs(abs(v - math.floor(v)) - 0.5) < 2e-4
    for f in flips_i:
        v = float(a["scales"][tuple(f)])
        print(f"  index flip at {tuple(int(i) for i in f)}: scale = {v!r} (oracle) vs {float(scales[tuple(f)])!r} (GPU)")
        assert float(((oracle.table - v).abs() / oracle.table).min()) < 2e-4
    # the rANS layer itself: the oracle's integers through the HIP coder give the oracle's y streams
    enc = ans.Rans64Encoder(16, True, 4)
    enc.init_cdf_params(*oracle.gc)
    (nz,) = struct.unpack("I", ref[:4])
    y_body, cur = ref[4 + nz:], 12
    for b in range(x.shape[0]):
        (n,) = struct.unpack(">I", y_body[cur:cur + 4])
        assert enc.encode_with_indexes(a["y_sym"][b].numpy(), a["y_idx"][b].numpy()) == y_body[cur + 4:cur + 4 + n], b
        cur += 4 + n
    return len(flips_s) + len(flips_i)


def test_kodak_shaped_image_roundtrip(setup):
    """BASELINE configs[1] shape: 3x512x768 (Kodak), batch 1 -- y is 192x32x48 = 294,912 symbols in one stream.
    The stream must equal the CPU oracle's byte for byte, EXCEPT for fp32 rounding ties between the MFMA and the
    torch-CPU summation orders; every such flip is located and shown to be a tie (|frac(y)| within 2e-4 of .5, or the
    scale within 2e-4 relative of a table threshold), at most 2 of them, and the rANS layer is then shown exact on the
    oracle's own integers."""
    from oracle.codec_oracle import psnr
    codec, oracle = setup
    torch.manual_seed(24)
    x = torch.rand(1, 3, 512, 768)
    data = codec.compress(x)
    xhat = codec.decompress(data).cpu()
    ref = oracle.compress(x)
    xref = oracle.decompress(ref)
    assert xhat.shape == x.shape
    a = oracle.analyse(x)
    flips = _assert_identical_or_located_ties(codec, oracle, x, data, ref, a, "kodak-shaped")
    print(f"kodak-shaped: identical={flips == 0}")
    assert float((psnr(xhat, x) - psnr(xref, x)).abs().max()) < 0.01
    # cross-decoding: the oracle reads the GPU stream
    assert _rel(oracle.decompress(data), xhat) < 1e-3


def test_rate_estimates_prior_entropy(setup):
    """forward()'s rate estimate metric (get_raw_cache("metric_dict")["prior_entropy"], nats per image)."""
    from oracle.codec_oracle import eb_entropy, gc_entropy
    codec, oracle = setup
    ec = codec.entropy_coder
    torch.manual_seed(3)
    x = torch.rand(2, 3, 128, 128)
    a = oracle.analyse(x)
    zc, yc = ec.latent_node_entropy_coders["z"], ec.latent_node_entropy_coders["y"]
    zc(a["z"].cuda())
    yc(a["y"].cuda(), prior=a["scales"].cuda())
    got_z = float(zc.get_raw_cache("metric_dict")["prior_entropy"])
    got_y = float(yc.get_raw_cache("metric_dict")["prior_entropy"])
    ref_z = float(eb_entropy(oracle.sd, "latent_node_entropy_coders.z.entropy_bottleneck.", a["z"]))
    ref_y = float(gc_entropy(a["y"], a["scales"]))
    assert abs(got_z - ref_z) <= 1e-3 * abs(ref_z), (got_z, ref_z)
    assert abs(got_y - ref_y) <= 1e-3 * abs(ref_y), (got_y, ref_y)
    # the estimate tracks the actual coded size (bits within a few percent)
    data = codec.compress(x)
    est_bits = (got_z + got_y) * 2 / 0.6931471805599453
    assert abs(est_bits - len(data) * 8) < 0.1 * len(data) * 8
    # codec level (general_codec.py:190-209, latent_graph.py:1168-1178): forward_estimate_bitlen returns BYTES for
    # the batch; the entropy coder caches prior_entropy (nats / image) and estimated_bpd (bits / input dimension)
    xhat, est_bytes = codec.forward_estimate_bitlen(x.cuda())
    assert xhat.shape == x.shape
    assert abs(float(est_bytes) - len(data)) < 0.1 * len(data)
    md = ec.get_raw_cache("metric_dict")
    pe = float(md["prior_entropy"])
    assert abs(pe * 2 / 0.6931471805599453 / 8 - float(est_bytes)) < 1e-3 * float(est_bytes)
    assert abs(float(md["estimated_bpd"]) - pe / 0.6931471805599453 / (3 * 128 * 128)) < 1e-6


def test_full_batch_properties(setup):
    """BASELINE configs[4] shape on one GPU (256 synthetic 3x256x256 images per step, what bench.py times), checked
    through size-independent properties instead of the (slow) CPU oracle:
      * determinism: compressing the same batch twice gives identical bytes,
      * shard invariance: the stream of image i does not depend on the batch it is coded in (the multi-GPU
        sharding of SURVEY 8e relies on this), checked for a handful of images against batch-1 runs,
      * decode(encode(x)) reproduces exactly the quantised latents the encoder coded (round trip through rANS),
        and equals the batch-1 reconstruction of the same image.
    """
    from cbench_basic_amd.modules.prior_model.prior_coder.compressai_coder import read_body
    from cbench_basic_amd.utils.bytes_ops import split_merged_bytes
    codec, oracle = setup
    g = torch.Generator().manual_seed(77)
    x = torch.rand(256, 3, 256, 256, generator=g).cuda()
    data = codec.compress(x)
    assert codec.compress(x) == data
    z_body, y_body = split_merged_bytes(data, num_segments=2)
    z_str, z_shape = read_body(z_body)
    y_str, y_shape = read_body(y_body)
    assert len(z_str) == 256 and len(y_str) == 256 and z_shape == (4, 4) and y_shape == (16, 16)
    xhat = codec.decompress(data)
    assert xhat.shape == x.shape and bool(torch.isfinite(xhat).all())
    for i in (0, 1, 127, 255):
        di = codec.compress(x[i:i + 1])
        zi, yi = split_merged_bytes(di, num_segments=2)
        assert read_body(zi)[0][0][0] == z_str[i][0]
        assert read_body(yi)[0][0][0] == y_str[i][0]
        assert torch.equal(codec.decompress(di)[0], xhat[i])
    # the decoder's latents are the encoder's: re-derive y_hat from the decoded stream and compare with forward()
    ec = codec.entropy_coder
    y = ec.latent_inference_modules["x_y"](x)
    z = ec.latent_inference_modules["y_z"](y)
    zc, yc = ec.latent_node_entropy_coders["z"], ec.latent_node_entropy_coders["y"]
    zhat = zc(z)
    assert torch.equal(zc.decode(z_body), zhat)
    prior = ec.latent_generative_modules["z_y"](zhat)
    assert torch.equal(yc.decode(y_body, prior=prior), yc(y, prior=prior))
