"""The testing half of ``BasicLosslessCompressionBenchmark`` (cbench/benchmark/basic_benchmark.py:105-326,640-1060) and
``BaseBenchmark.save_metrics`` (cbench/benchmark/base.py:54-112): run codec.compress / decompress over a dataset for
every (complexity level, rate level), collect the reference's metric names, write ``metrics.csv`` and ``metrics_2d.csv``.

Step metrics (basic_benchmark.py:121-260): ``original_length`` (bytes of the input tensor), ``compression_ratio``,
``compressed_length``, ``time_compress`` / ``time_decompress`` / ``time_total`` (ms), ``speed_*`` (MiB/s of original
data), the distortion metric (``psnr``), and with ``nn_codec_use_forward_pass`` the ``*_nn_forward`` pair from
``codec.forward_estimate_bitlen``.  Level loop and key prefixes (``sclevel{c}_vrlevel{r}_<metric>``) follow
:913-1026, including BD-rate over the rate levels when there are more than three of them.

``num_testing_workers`` (:829-858): the reference hands contiguous index ranges of the dataloader to a multiprocessing pool --
and switches the pool off when testing on a device (``force_testing_device is None`` is required, :836).  Here the workers are
concurrent stream workers on the ONE GPU (stream_workers.py: host threads, each with its own HIP stream and its own replica of
the codec built by ``codec_builder``), so dataset items are coded concurrently: one item's serial rANS chains and launch-bound
AR steps run beside another item's transforms.  Per-item times are the latencies of the calls as they ran (concurrently);
``time_wall_dataset`` / ``speed_wall_dataset`` give the wall time and MiB/s of the whole dataset pass.

``testing_coalesce_items`` (not in the reference; INTEGRATION.md, "Coalesced items"): a dataset of batch-1 items is coded in calls of
up to that many items of one shape (``codec.compress_items`` / ``decompress_items``); every item keeps the bytes and the
reconstruction of its own batch-1 call, the metrics are logged per item with the keys of the sequential pass, and a call's time is
shared equally among its items.

``metrics_on_uint8`` (not in the reference; INTEGRATION.md, "8-bit images"): the distortion is taken from the 8-bit picture the codec
hands out -- ``codec.decompress(compressed, output_dtype=torch.uint8)``, converted inside the timed region -- against the 8-bit item
(a float item: quantised once), as exact integers; ``on_reconstruction`` receives that very picture after the pass.

``testing_tile=(th, tw)`` (not in the reference; INTEGRATION.md, "Tiled pictures"): every item, a batch-1 picture, is coded as
independent tiles (``codec.compress_tiled`` / ``decompress_tiled``); ``compressed_length`` is the length of the container and the
distortion that of the whole pasted picture.  It does not combine with ``testing_coalesce_items``.  ``testing_tile_overlap`` (an int
or ``(oy, ox)``, at most half a tile; needs ``testing_tile``): the tiles overlap and ``decompress_tiled`` cross-fades the seams.

``testing_tile_pool=N`` (needs ``testing_tile``; INTEGRATION.md, "Tiled pictures"): up to N consecutive batch-1 pictures, of any sizes,
are coded per call (``codec.compress_tiled_items`` / ``decompress_tiled_items``), the tiles of all of them pooled into shared coding
calls.  Every item is logged as the unpooled tiled pass logs it -- its own container's length, its own pasted picture's distortion --
and a call's time is shared equally among its pictures.  It runs on the calling thread: no ``testing_coalesce_items``, no workers.

``testing_tile_pad`` (an int or ``(py, px)`` that divides the tile; needs ``testing_tile``; INTEGRATION.md, "Tiled pictures"): the edge
tiles are coded at their size rounded up to multiples of py x px (``compress_tiled(..., pad_to=)``), so ``compressed_length`` is the
BTL3 container's length.  It composes with ``testing_tile_overlap`` and ``testing_tile_pool``.

``testing_tile_qsteps`` / ``testing_tile_target_bpps`` (need ``testing_tile``; INTEGRATION.md, "Tiled pictures: step and byte budget"):
one pass per step through ``compress_tiled_q``, or per target through ``compress_tiled_to_rate`` (with ``testing_tile_pool`` their
``_items`` forms), under the level prefixes ``tq<step>`` / ``tbpp<target>``; ``compressed_length`` is the BTQ1 container's length and
``decompress_tiled`` reads the steps from it.  They compose with the overlap, the padding, the pool and ``metrics_on_uint8``, and are
refused with each other, with ``testing_qsteps`` / ``testing_target_bpps`` (which stay refused with ``testing_tile``) and with what
refuses those.

``testing_skip_rows=[r, ...]`` ("Skip coding"): one pass per value through ``compress_skip`` / ``decompress_skip``
under the level prefix ``skip<r>``; ``compressed_length`` is the BSK1 container's length.  Refused with what refuses
``testing_qsteps``, and with the steps, the targets and the tiled knobs themselves.
"""
import copy
import csv
import os
import pickle
import time
from collections import OrderedDict

import numpy as np
import torch

from .metrics import MetricLogger


class BasicLosslessCompressionBenchmark:
    def __init__(self, codec, dataloader, *args, distortion_metric=None, skip_decompress=False,
                 nn_codec_use_forward_pass=False, nn_codec_forward_pass_skip_compression=False,
                 testing_variable_rate_levels=None, testing_variable_rate_bj_delta_metric=None,
                 testing_complexity_levels=None, force_testing_device="cuda", output_dir=None, num_repeats=1,
                 num_testing_workers=0, codec_builder=None, worker_transform_token=None, testing_coalesce_items=0,
                 metrics_on_uint8=False, on_reconstruction=None, testing_tile=None, testing_tile_overlap=0, testing_tile_pool=0,
                 testing_tile_pad=None, testing_qsteps=None, testing_target_bpps=None, testing_tile_qsteps=None,
                 testing_tile_target_bpps=None, testing_skip_rows=None, **kwargs):
        self.codec = codec
        self.dataloader = dataloader
        self.distortion_metric = distortion_metric
        self.skip_decompress = skip_decompress
        self.nn_codec_use_forward_pass = nn_codec_use_forward_pass
        self.nn_codec_forward_pass_skip_compression = nn_codec_forward_pass_skip_compression
        self.testing_variable_rate_levels = list(testing_variable_rate_levels or [])
        self.testing_variable_rate_bj_delta_metric = testing_variable_rate_bj_delta_metric
        self.testing_complexity_levels = list(testing_complexity_levels or [])
        self.force_testing_device = force_testing_device
        self.output_dir = output_dir
        self.num_repeats = num_repeats
        self.metric_logger = MetricLogger()
        self.num_testing_workers = int(num_testing_workers or 0)
        self.codec_builder = codec_builder
        # concurrent sessions with ordered MFMA phases + packed rANS workgroups: pays for batches (measured: 48
        # images in batches of 8, 3 workers: 248 -> 297 MiB/s), costs at batch 1 where everything is latency (Kodak-shaped,
        # 4 workers: 21.7 -> 13.8 Mpix/s).  None = on for batches of 8 or more
        self.worker_transform_token = worker_transform_token
        if self.num_testing_workers > 1 and codec_builder is None:
            raise ValueError("num_testing_workers > 1 needs codec_builder: a callable returning a fresh codec of the same "
                             "architecture (every worker codes with its own replica; weights and levels are copied from `codec`)")
        # coalesced items ("Coalesced items"): a dataset of batch-1 items is coded in calls of up to this many items
        # of one shape (codec.compress_items / decompress_items), every item keeping its own bytes; 0 / 1 = one call per item
        self.testing_coalesce_items = int(testing_coalesce_items or 0)
        if self.testing_coalesce_items < 0:
            raise ValueError("testing_coalesce_items must be >= 0")
        # the 8-bit picture is what is measured: items and reconstructions meet the metric as uint8 ("8-bit images")
        self.metrics_on_uint8 = bool(metrics_on_uint8)
        # on_reconstruction(level_prefix, item_index, picture_u8): the uint8 [B, C, H, W] tensor the metric saw for dataset item
        # `item_index` (a batch-1 item: once per image), called for every item once the pass over the dataset is over and its wall
        # time taken, in dataset order, from the calling thread -- whatever the route and the workers' order
        self.on_reconstruction = on_reconstruction
        if on_reconstruction is not None and not self.metrics_on_uint8:
            raise ValueError("on_reconstruction hands out the 8-bit picture the metric saw: it needs metrics_on_uint8=True")
        # tiled pictures ("Tiled pictures"): every batch-1 item goes through compress_tiled / decompress_tiled
        if testing_tile is not None:
            testing_tile = (testing_tile, testing_tile) if isinstance(testing_tile, int) else tuple(int(v) for v in testing_tile)
            if len(testing_tile) != 2 or min(testing_tile) < 1:
                raise ValueError(f"testing_tile is (th, tw), positive, not {testing_tile!r}")
            if self.testing_coalesce_items > 1:
                raise ValueError("testing_tile codes one picture per call: it does not combine with testing_coalesce_items")
        self.testing_tile = testing_tile
        # overlapped tiles, seams cross-faded by decompress_tiled: an int or (oy, ox), at most half a tile
        testing_tile_overlap = (testing_tile_overlap,) * 2 if isinstance(testing_tile_overlap, int) else tuple(int(v) for v in testing_tile_overlap)
        if len(testing_tile_overlap) != 2 or min(testing_tile_overlap) < 0:
            raise ValueError(f"testing_tile_overlap is (oy, ox), not negative, not {testing_tile_overlap!r}")
        if any(testing_tile_overlap):
            if testing_tile is None:
                raise ValueError("testing_tile_overlap needs testing_tile")
            if 2 * testing_tile_overlap[0] > testing_tile[0] or 2 * testing_tile_overlap[1] > testing_tile[1]:
                raise ValueError(f"testing_tile_overlap {testing_tile_overlap} is more than half a {testing_tile} tile")
        self.testing_tile_overlap = testing_tile_overlap
        # pooled tiles: up to this many consecutive pictures per compress_tiled_items / decompress_tiled_items call; 0 / 1 = one each
        self.testing_tile_pool = int(testing_tile_pool or 0)
        if self.testing_tile_pool < 0:
            raise ValueError("testing_tile_pool must be >= 0")
        if self.testing_tile_pool:
            if testing_tile is None:
                raise ValueError("testing_tile_pool needs testing_tile")   # which refuses testing_coalesce_items above 1
            if self.num_testing_workers > 1:
                raise ValueError("testing_tile_pool runs on the calling thread: it does not combine with num_testing_workers")
        # edge-padded tiles: an int or (py, px) that divides the tile; None: no padding, and no pad_to reaches the codec
        if testing_tile_pad is not None:
            testing_tile_pad = (testing_tile_pad,) * 2 if isinstance(testing_tile_pad, int) else tuple(int(v) for v in testing_tile_pad)
            if len(testing_tile_pad) != 2 or min(testing_tile_pad) < 1:
                raise ValueError(f"testing_tile_pad is (py, px), positive, not {testing_tile_pad!r}")
            if testing_tile is None:
                raise ValueError("testing_tile_pad needs testing_tile")
            if testing_tile[0] % testing_tile_pad[0] or testing_tile[1] % testing_tile_pad[1]:
                raise ValueError(f"testing_tile_pad {testing_tile_pad} does not divide a {testing_tile} tile")
        self.testing_tile_pad = testing_tile_pad
        self._tile_pad = {} if testing_tile_pad is None else dict(pad_to=testing_tile_pad)
        # quantiser steps ("Quantiser step"): one pass over the dataset per step through compress_q / decompress_q,
        # level prefix q<step>; the steps are the rate axis, as the variable-rate levels are for a codec that has them
        from ..utils.qstep import check_qsteps
        self.testing_qsteps = [float(q) for q in (testing_qsteps or [])]
        for q in self.testing_qsteps:
            check_qsteps(q)
        if self.testing_qsteps:
            for name, on in (("testing_variable_rate_levels", bool(self.testing_variable_rate_levels)),
                             ("testing_complexity_levels", bool(self.testing_complexity_levels)),
                             ("testing_coalesce_items", self.testing_coalesce_items > 1), ("testing_tile", testing_tile is not None),
                             ("nn_codec_use_forward_pass", bool(nn_codec_use_forward_pass))):
                if on:
                    raise ValueError(f"testing_qsteps does not combine with {name}: the step is a knob of compress_q / decompress_q alone")
        # rate targets ("Rate control"): one pass per target through compress_to_rate / decompress_q, level prefix
        # bpp<target>; refused with what refuses the steps, and with the steps themselves
        from ..utils.rate import budgets_from
        self.testing_target_bpps = [float(r) for r in (testing_target_bpps or [])]
        for r in self.testing_target_bpps:
            if not r > 0 or r == float("inf"):
                raise ValueError(f"testing_target_bpps must be positive and finite, got {r}")
            budgets_from(None, r, 1, 1 << 12, 1 << 12)
        if self.testing_target_bpps:
            for name, on in (("testing_qsteps", bool(self.testing_qsteps)),
                             ("testing_variable_rate_levels", bool(self.testing_variable_rate_levels)),
                             ("testing_complexity_levels", bool(self.testing_complexity_levels)),
                             ("testing_coalesce_items", self.testing_coalesce_items > 1), ("testing_tile", testing_tile is not None),
                             ("nn_codec_use_forward_pass", bool(nn_codec_use_forward_pass))):
                if on:
                    raise ValueError(f"testing_target_bpps does not combine with {name}: the target is a knob of compress_to_rate alone")
        # tiled pictures under a step or a byte budget ("Tiled pictures: step and byte budget"): one pass per value
        # through compress_tiled_q / compress_tiled_to_rate (with testing_tile_pool their _items forms), level prefixes tq<step> and
        # tbpp<target>; decompress_tiled reads the step from the container.  They need testing_tile, and are refused with each other,
        # with the untiled knobs above and with what refuses those
        self.testing_tile_qsteps = [float(q) for q in (testing_tile_qsteps or [])]
        for q in self.testing_tile_qsteps:
            check_qsteps(q)
        self.testing_tile_target_bpps = [float(r) for r in (testing_tile_target_bpps or [])]
        for r in self.testing_tile_target_bpps:
            if not r > 0 or r == float("inf"):
                raise ValueError(f"testing_tile_target_bpps must be positive and finite, got {r}")
            budgets_from(None, r, 1, 1 << 12, 1 << 12)
        for mine, other in (("testing_tile_qsteps", "testing_tile_target_bpps"), ("testing_tile_target_bpps", "testing_tile_qsteps")):
            if not getattr(self, mine):
                continue
            if testing_tile is None:
                raise ValueError(f"{mine} needs testing_tile: the untiled knobs are testing_qsteps / testing_target_bpps")
            for name, on in ((other, bool(getattr(self, other))), ("testing_qsteps", bool(self.testing_qsteps)),
                             ("testing_target_bpps", bool(self.testing_target_bpps)),
                             ("testing_variable_rate_levels", bool(self.testing_variable_rate_levels)),
                             ("testing_complexity_levels", bool(self.testing_complexity_levels)),
                             ("testing_coalesce_items", self.testing_coalesce_items > 1),
                             ("nn_codec_use_forward_pass", bool(nn_codec_use_forward_pass))):
                if on:
                    raise ValueError(f"{mine} does not combine with {name}: it is a knob of the tiled calls alone")
        # skip coding ("Skip coding"): one pass per row count through compress_skip / decompress_skip, level prefix
        # skip<r>; refused with what refuses the steps, and with every other rate knob
        from ..utils.skip import check_skip_rows
        self.testing_skip_rows = [check_skip_rows(r) for r in (testing_skip_rows or [])]
        if self.testing_skip_rows:
            for name, on in (("testing_qsteps", bool(self.testing_qsteps)), ("testing_target_bpps", bool(self.testing_target_bpps)),
                             ("testing_tile_qsteps", bool(self.testing_tile_qsteps)),
                             ("testing_tile_target_bpps", bool(self.testing_tile_target_bpps)),
                             ("testing_variable_rate_levels", bool(self.testing_variable_rate_levels)),
                             ("testing_complexity_levels", bool(self.testing_complexity_levels)),
                             ("testing_coalesce_items", self.testing_coalesce_items > 1), ("testing_tile", testing_tile is not None),
                             ("nn_codec_use_forward_pass", bool(nn_codec_use_forward_pass))):
                if on:
                    raise ValueError(f"testing_skip_rows does not combine with {name}: the rows are a knob of compress_skip / decompress_skip alone")
        self._skip_rows = None
        self._qstep = None
        self._target_bpp = None
        self._tile_qstep = None
        self._tile_bpp = None
        self._level_prefix = ""
        self._pictures = {}
        self._pool = None

    # ---- files (base.py:41-52)
    @property
    def metric_file(self):
        return os.path.join(self.output_dir, "metrics.csv")

    @property
    def metric_raw_file(self):
        return os.path.join(self.output_dir, "metrics.pkl")

    # ---- one step (basic_benchmark.py:105-260)
    @staticmethod
    def _estimate_byte_length(data):
        if isinstance(data, bytes):
            return len(data)
        if isinstance(data, str):
            return len(data.encode("utf-8"))
        if isinstance(data, torch.Tensor):
            return int(np.prod(data.shape)) * data.element_size()
        if isinstance(data, np.ndarray):
            return int(data.size * data.itemsize)
        raise ValueError("Bitstream of data {} in type {} cannot be estimated!".format(data, type(data)))

    def _sync(self):
        # the queue of THIS caller is empty before and after every timed region: the current stream -- the default stream in a
        # sequential run (where it is the only one in use), the worker's own stream in a parallel one (a device-wide
        # synchronisation there would make every worker wait for all the others at every item)
        if torch.cuda.is_available():
            torch.cuda.current_stream().synchronize()

    @staticmethod
    def _to_f32(x):
        """An 8-bit batch as the float graph takes it: u8 / 255 (the library's kernel on the GPU)."""
        if x.is_cuda:
            from ..nn import kernels as K
            return K.image_u8_to_f32(x)
        return x.float().div(255)

    @staticmethod
    def _to_u8(x):
        """A float batch as the 8-bit picture of it (the library's kernel on the GPU, its definition in torch ops on the CPU)."""
        if x.is_cuda:
            from ..nn import kernels as K
            return K.image_f32_to_u8(x.float())
        return torch.nan_to_num(x.float(), nan=0.0).clamp(0, 1).mul(255).round().to(torch.uint8)

    def _target(self, data):
        """What a reconstruction of ``data`` is compared with: the item on the testing device; an 8-bit item converted ONCE there
        (u8 / 255 by the library's kernel), so that its distortion is the one of the same item given as float32.  With
        ``metrics_on_uint8`` it is the 8-bit item itself, and a float item quantised ONCE."""
        target = data.to(self.force_testing_device) if self.force_testing_device else data
        if not isinstance(target, torch.Tensor):
            return target
        if self.metrics_on_uint8:
            return target if target.dtype == torch.uint8 else self._to_u8(target)
        if target.dtype == torch.uint8:
            target = self._to_f32(target)
        return target

    def _forward_input(self, data_input, data_target):
        """The forward pass is the float graph: an 8-bit item enters it converted."""
        if getattr(data_input, "dtype", None) != torch.uint8:
            return data_input
        return self._to_f32(data_target) if self.metrics_on_uint8 else data_target

    def _compress(self, codec, data):
        if self._skip_rows is not None:
            return codec.compress_skip(data, self._skip_rows)
        if self._target_bpp is not None:
            return codec.compress_to_rate(data, target_bpp=self._target_bpp)
        if self._qstep is not None:
            return codec.compress_q(data, self._qstep)
        if self.testing_tile is None:
            return codec.compress(data)
        if not isinstance(data, torch.Tensor) or data.dim() != 4 or data.shape[0] != 1:
            raise ValueError("testing_tile codes a dataset of batch-1 pictures ([1, C, H, W]); got "
                             f"{tuple(data.shape) if isinstance(data, torch.Tensor) else type(data).__name__}")
        if self._tile_bpp is not None:
            return codec.compress_tiled_to_rate(data, target_bpp=self._tile_bpp, tile=self.testing_tile, overlap=self.testing_tile_overlap,
                                                **self._tile_pad)
        if self._tile_qstep is not None:
            return codec.compress_tiled_q(data, self._tile_qstep, tile=self.testing_tile, overlap=self.testing_tile_overlap, **self._tile_pad)
        return codec.compress_tiled(data, tile=self.testing_tile, overlap=self.testing_tile_overlap, **self._tile_pad)

    def _decompress(self, codec, compressed):
        if self._skip_rows is not None:
            return codec.decompress_skip(compressed, output_dtype=torch.uint8 if self.metrics_on_uint8 else None)
        if self._qstep is not None or self._target_bpp is not None:
            return codec.decompress_q(compressed, output_dtype=torch.uint8 if self.metrics_on_uint8 else None)
        if self.testing_tile is not None:
            return codec.decompress_tiled(compressed, output_dtype=torch.uint8 if self.metrics_on_uint8 else None)
        return codec.decompress(compressed, output_dtype=torch.uint8) if self.metrics_on_uint8 else codec.decompress(compressed)

    def _deliver_pictures(self):
        """After a pass, outside its timed regions: every item's picture to ``on_reconstruction``, in dataset order."""
        pictures, self._pictures = self._pictures, {}
        if self.on_reconstruction is not None:
            for i in sorted(pictures):
                self.on_reconstruction(self._level_prefix, i, pictures[i])

    def _run_step(self, step, data, metric_logger, codec=None, distortion_metric=None):
        codec = self.codec if codec is None else codec
        # the batch stays where the loader left it (the host): codec.compress() uploads it INSIDE the timed region, as the
        # reference's does (general_codec.py:46-47 under basic_benchmark.py:199-202); only the metric's target is moved
        data_input = data
        data_target = self._target(data)
        original_length = self._estimate_byte_length(data_input)   # an 8-bit item: one byte per sample, a quarter of the float item's
        metric_logger.update(original_length=original_length)
        dm = self.distortion_metric if distortion_metric is None else distortion_metric
        if self.nn_codec_use_forward_pass and hasattr(codec, "forward_estimate_bitlen"):
            decompressed, compressed_length = codec.forward_estimate_bitlen(self._forward_input(data_input, data_target))
            compressed_length = float(compressed_length)
            metric_logger.update(compression_ratio_nn_forward=compressed_length / original_length,
                                 compressed_length_nn_forward=compressed_length)
            if dm is not None:
                dm(self._to_u8(decompressed) if self.metrics_on_uint8 else decompressed, data_target)
            if self.nn_codec_forward_pass_skip_compression:
                return
        self._sync()
        t0 = time.time()
        compressed = self._compress(codec, data_input)
        self._sync()
        time_compress = time.time() - t0
        compressed_length = self._estimate_byte_length(compressed)
        metric_logger.update(compression_ratio=compressed_length / original_length, compressed_length=compressed_length,
                             time_compress=time_compress * 1000,
                             speed_compress=original_length / time_compress / 1024 / 1024)
        if not self.skip_decompress:
            t0 = time.time()
            decompressed = self._decompress(codec, compressed)   # metrics_on_uint8: the picture is the product, converted in here
            self._sync()
            time_decompress = time.time() - t0
            metric_logger.update(time_decompress=time_decompress * 1000,
                                 speed_decompress=original_length / time_decompress / 1024 / 1024,
                                 time_total=(time_compress + time_decompress) * 1000,
                                 speed_total=original_length / (time_compress + time_decompress) / 1024 / 1024)
            if dm is not None:
                dm(decompressed, data_target)
            if self.on_reconstruction is not None:
                self._pictures[step] = decompressed

    def _worker_pool(self, first_item=None, batch=None):
        """The stream workers and their codec replicas, brought to the main codec's weights, levels and tables.  ``batch``: the
        images per call when that is not the first item's batch (coalesced items)."""
        from .stream_workers import StreamWorkerPool
        if self._pool is None:
            if batch is None and first_item is not None and hasattr(first_item, "shape") and len(first_item.shape) == 4:
                batch = first_item.shape[0]
            self._token_on = self.worker_transform_token if self.worker_transform_token is not None else bool(batch is not None and batch >= 8)
            def make():
                c = self.codec_builder()
                if hasattr(c, "eval"):
                    c.eval()
                if self._token_on:
                    for m in (c.modules() if hasattr(c, "modules") else []):   # concurrent sessions: ordered MFMA phases, packed rANS workgroups
                        if hasattr(m, "fused_transform_token"):
                            m.fused_transform_token, m.fused_rans_waves = True, 8
                return c.to(self.force_testing_device or "cuda") if hasattr(c, "to") else c
            self._pool = StreamWorkerPool(make, self.num_testing_workers, torch.device(self.force_testing_device or "cuda"))
        level_attrs = ("_current_complex_level", "_current_rate_level", "_current_task_idx", "active_codec_idx")
        # replicas already at the main codec's weights and levels (a warm-up pass, the next pass at the same level) are left
        # alone: reloading and update_state() would rebuild tables and layer plans, and the first item of every worker would
        # pay for it inside the timed pass.  Fingerprint: every state tensor's storage and in-place version counter + the levels.
        def fingerprint():
            mods = list(self.codec.named_modules()) if hasattr(self.codec, "named_modules") else [("", self.codec)]
            levels = tuple((n, a, repr(getattr(m, a))) for n, m in mods for a in level_attrs if hasattr(m, a))
            searched = tuple((n, id(getattr(m, "_complexity_param_all_levels", None)), getattr(m, "_num_complex_levels", None)) for n, m in mods)
            sd = self.codec.state_dict() if hasattr(self.codec, "state_dict") else {}
            state = tuple((k, t.data_ptr(), t._version) for k, t in sd.items())
            # ... and a content checksum (sum and sum of squares of every state tensor, one synchronisation per pass): edits that do
            # not bump the version counter (`.data`, a checkpoint loader writing through views) are seen too
            fl = [t.detach().double().reshape(-1) for t in sd.values() if torch.is_tensor(t) and t.numel() > 0]
            content = tuple(torch.stack([torch.stack([f.sum(), (f * f).sum()]) for f in fl]).sum(0).tolist()) if fl else ()
            return levels, searched, state, content
        fp = fingerprint()
        if getattr(self._pool, "_synced_to", None) == fp:
            return self._pool
        for r in self._pool.codecs:
            if hasattr(r, "named_modules"):
                theirs = dict(r.named_modules())
                for name, src in self.codec.named_modules():   # the codec itself, grouped members, their entropy coders
                    dst = theirs.get(name)
                    if dst is None:
                        continue
                    if hasattr(src, "_complexity_param_all_levels"):   # searched levels: modules made after construction
                        dst._complexity_param_all_levels = copy.deepcopy(src._complexity_param_all_levels)
                        dst._num_complex_levels = src._num_complex_levels
                    for a in level_attrs:
                        if hasattr(src, a):
                            setattr(dst, a, getattr(src, a))
                    if hasattr(dst, "_valid_host"):
                        dst._valid_host = None
                r.load_state_dict(self.codec.state_dict(), strict=False)
            else:
                for a in level_attrs:
                    if hasattr(self.codec, a):
                        setattr(r, a, getattr(self.codec, a))
            r.update_state()
        self._pool._synced_to = fp
        return self._pool

    def invalidate_replicas(self):
        """Force the stream workers' codec replicas to be re-synchronised before the next pass.  The automatic check covers the
        state_dict (storage, version counters, content checksum), the level attributes and the searched levels; call this after
        changing anything ELSE on the main codec that the replicas must share (a tuning attribute set by hand, a module swapped in)."""
        if self._pool is not None:
            self._pool._synced_to = None

    # ---- coalesced items: chunks of batch-1 items of one shape, one timed compress_items / decompress_items per chunk
    def _run_chunk(self, chunk, items, records, codec=None):
        """Codes items[i] for i in chunk in one call each way and fills records[i] = (metric updates, distortion results) with
        exactly the keys _run_step logs; a chunk's call time is shared equally among its items."""
        codec = self.codec if codec is None else codec
        dm = self.distortion_metric   # asked with cache_metrics=False only: nothing is logged before the pass is over
        data = [items[i] for i in chunk]
        targets = [self._target(d) for d in data]
        lengths = [self._estimate_byte_length(d) for d in data]
        n = len(chunk)
        for i, L in zip(chunk, lengths):
            records[i] = (OrderedDict(original_length=L), [])
        if self.nn_codec_use_forward_pass and hasattr(codec, "forward_estimate_bitlen"):
            for i, d, t, L in zip(chunk, data, targets, lengths):   # the forward estimate stays one call per item
                decompressed, compressed_length = codec.forward_estimate_bitlen(self._forward_input(d, t))
                compressed_length = float(compressed_length)
                records[i][0].update(compression_ratio_nn_forward=compressed_length / L, compressed_length_nn_forward=compressed_length)
                if dm is not None:
                    records[i][1].append(dm(self._to_u8(decompressed) if self.metrics_on_uint8 else decompressed, t, cache_metrics=False))
            if self.nn_codec_forward_pass_skip_compression:
                return
        self._sync()
        t0 = time.time()
        compressed = self._compress_many(codec, data)
        self._sync()
        time_compress = (time.time() - t0) / n
        if len(compressed) != n:
            raise ValueError(f"{len(compressed)} strings were returned for {n} items")
        for i, c, L in zip(chunk, compressed, lengths):
            compressed_length = self._estimate_byte_length(c)
            records[i][0].update(compression_ratio=compressed_length / L, compressed_length=compressed_length,
                                 time_compress=time_compress * 1000, speed_compress=L / time_compress / 1024 / 1024)
        if not self.skip_decompress:
            t0 = time.time()
            decompressed = self._decompress_many(codec, compressed)
            self._sync()
            time_decompress = (time.time() - t0) / n
            for i, L in zip(chunk, lengths):
                records[i][0].update(time_decompress=time_decompress * 1000, speed_decompress=L / time_decompress / 1024 / 1024,
                                     time_total=(time_compress + time_decompress) * 1000,
                                     speed_total=L / (time_compress + time_decompress) / 1024 / 1024)
            if dm is not None and self.testing_tile_pool:   # pictures of any sizes: each measured as the tiled pass measures it
                for i, d, t in zip(chunk, decompressed, targets):
                    records[i][1].append(dm(d, t, cache_metrics=False))
            elif dm is not None:
                for i, r in zip(chunk, dm.per_item(list(decompressed), targets, cache_metrics=False)):
                    records[i][1].append(r)
            if self.on_reconstruction is not None:
                for i, picture in zip(chunk, decompressed):
                    self._pictures[i] = picture

    def _compress_many(self, codec, data):
        """The items of a chunk in one call: coalesced items of one shape, or pooled tiles of pictures of any sizes."""
        if self.testing_tile_pool and self._tile_bpp is not None:
            return codec.compress_tiled_items_to_rate(data, target_bpp=self._tile_bpp, tile=self.testing_tile,
                                                      overlap=self.testing_tile_overlap, **self._tile_pad)
        if self.testing_tile_pool and self._tile_qstep is not None:
            return codec.compress_tiled_items_q(data, self._tile_qstep, tile=self.testing_tile, overlap=self.testing_tile_overlap,
                                                **self._tile_pad)
        if self.testing_tile_pool:
            return codec.compress_tiled_items(data, tile=self.testing_tile, overlap=self.testing_tile_overlap, **self._tile_pad)
        return codec.compress_items(data, max_batch=len(data))

    def _decompress_many(self, codec, compressed):
        if self.testing_tile_pool:
            return codec.decompress_tiled_items(compressed, output_dtype=torch.uint8 if self.metrics_on_uint8 else None)
        if self.metrics_on_uint8:
            return codec.decompress_items(compressed, max_batch=len(compressed), output_dtype=torch.uint8)
        return codec.decompress_items(compressed, max_batch=len(compressed))

    def _run_dataset_tile_pool(self):
        """The tiled pass with up to ``testing_tile_pool`` consecutive pictures per call, logged per item in dataset order."""
        logger = MetricLogger()
        self._sync()
        t0 = time.time()
        items = list(self.dataloader)
        for d in items:
            if not isinstance(d, torch.Tensor) or d.dim() != 4 or d.shape[0] != 1:
                raise ValueError("testing_tile_pool codes a dataset of batch-1 pictures ([1, C, H, W]); got "
                                 f"{tuple(d.shape) if isinstance(d, torch.Tensor) else type(d).__name__}")
        if not (hasattr(self.codec, "compress_tiled_items") and hasattr(self.codec, "decompress_tiled_items")):
            raise ValueError("testing_tile_pool needs a codec with compress_tiled_items / decompress_tiled_items")
        records = [None] * len(items)
        for first in range(0, len(items), self.testing_tile_pool):
            self._run_chunk(list(range(first, min(first + self.testing_tile_pool, len(items)))), items, records)
        self._sync()
        wall = time.time() - t0
        n_bytes = 0
        for d, (updates, distortions) in zip(items, records):
            logger.update(**updates)
            for r in distortions:
                self.distortion_metric.metric_logger.update(**r)
            n_bytes += self._estimate_byte_length(d)
        out = logger.get_global_average()
        if items:
            out["time_wall_dataset"] = wall * 1000
            out["speed_wall_dataset"] = n_bytes / wall / 1024 / 1024
        self._deliver_pictures()
        return out

    def _run_dataset_coalesced(self):
        from ..utils.item_framing import coalesce_chunks
        logger = MetricLogger()
        self._sync()
        t0 = time.time()   # the sequential pass loads inside its wall time; so does this one (the worker pass restarts the clock, as today)
        items = list(self.dataloader)
        for d in items:
            if not hasattr(d, "shape") or len(d.shape) != 4 or d.shape[0] != 1:
                raise ValueError("testing_coalesce_items codes a dataset of batch-1 items ([1, C, H, W]); got "
                                 f"{tuple(d.shape) if hasattr(d, 'shape') else type(d)}: coalescing and dataloader batching do not combine")
        if not (hasattr(self.codec, "compress_items") and hasattr(self.codec, "decompress_items")):
            raise ValueError("testing_coalesce_items needs a codec with compress_items / decompress_items")
        if self.distortion_metric is not None and not hasattr(self.distortion_metric, "per_item"):
            raise ValueError("testing_coalesce_items needs a distortion metric with per_item")
        chunks = coalesce_chunks([(tuple(d.shape), getattr(d, "dtype", None)) for d in items], self.testing_coalesce_items)
        records = [None] * len(items)
        if self.num_testing_workers > 1 and (self.force_testing_device or "cuda").startswith("cuda"):
            pool = self._worker_pool(items[0] if items else None, batch=max((len(c) for c in chunks), default=None))
            W = min(self.num_testing_workers, max(1, len(chunks)))
            base, extra = divmod(len(chunks), W)
            bounds = [0]   # whole chunks, contiguous ranges of the chunk list
            for w in range(W):
                bounds.append(bounds[-1] + base + (1 if w < extra else 0))
            self._sync()
            t0 = time.time()

            def work(codec, w):
                for c in range(bounds[w], bounds[w + 1]):
                    self._run_chunk(chunks[c], items, records, codec=codec)
                return None
            pool.map(work, list(range(W)))
        else:
            for chunk in chunks:
                self._run_chunk(chunk, items, records)
        self._sync()
        wall = time.time() - t0
        n_bytes = 0
        for d, (updates, distortions) in zip(items, records):   # logged per item, in DATASET order
            logger.update(**updates)
            for r in distortions:
                self.distortion_metric.metric_logger.update(**r)
            n_bytes += self._estimate_byte_length(d)
        out = logger.get_global_average()
        if items:
            out["time_wall_dataset"] = wall * 1000
            out["speed_wall_dataset"] = n_bytes / wall / 1024 / 1024
        self._deliver_pictures()
        return out

    def _run_dataset(self):
        if self.testing_coalesce_items > 1:
            return self._run_dataset_coalesced()
        if self.testing_tile_pool > 1:
            return self._run_dataset_tile_pool()
        logger = MetricLogger()
        n_items, n_bytes = 0, 0
        self._sync()
        t0 = time.time()
        if self.num_testing_workers > 1 and (self.force_testing_device or "cuda").startswith("cuda"):
            items = list(self.dataloader)
            pool = self._worker_pool(items[0] if items else None)
            W = min(self.num_testing_workers, max(1, len(items)))
            base, extra = divmod(len(items), W)
            # contiguous index ranges as in the reference (:851-852), remainder spread (the reference drops len % W items)
            bounds = [0]
            for w in range(W):
                bounds.append(bounds[-1] + base + (1 if w < extra else 0))
            loggers = [MetricLogger() for _ in range(W)]
            dms = [copy.deepcopy(self.distortion_metric) if self.distortion_metric is not None else None for _ in range(W)]
            codec_of = {id(c): i for i, c in enumerate(pool.codecs)}
            self._sync()
            t0 = time.time()

            def work(codec, w):
                for step in range(bounds[w], bounds[w + 1]):
                    self._run_step(step, items[step], loggers[w], codec=codec, distortion_metric=dms[w])
                return None
            pool.map(work, list(range(W)))
            for w in range(W):
                logger.merge(loggers[w])
                if dms[w] is not None:
                    self.distortion_metric.metric_logger.merge(dms[w].metric_logger)
            for d in items:
                n_items, n_bytes = n_items + 1, n_bytes + self._estimate_byte_length(d)
        else:
            for step, data in enumerate(self.dataloader):
                self._run_step(step, data, logger)
                n_items, n_bytes = n_items + 1, n_bytes + self._estimate_byte_length(data)
        self._sync()
        wall = time.time() - t0
        out = logger.get_global_average()
        if n_items:
            out["time_wall_dataset"] = wall * 1000
            out["speed_wall_dataset"] = n_bytes / wall / 1024 / 1024
        self._deliver_pictures()
        return out

    def close(self):
        if self._pool is not None:
            self._pool.close()
            self._pool = None

    # ---- level loop (basic_benchmark.py:640-1030): rate levels innermost, then complexity levels
    def run_testing(self, *args, **kwargs):
        metrics, metrics_2d = OrderedDict(), OrderedDict()
        vr, vc = self.testing_variable_rate_levels, self.testing_complexity_levels
        # the rate axis: (rate level, quantiser step) pairs -- the codec's own levels, or the steps (never both: __init__)
        axis = [(r, None, None) for r in vr] or [(None, q, None) for q in self.testing_qsteps] or [(None, None, r) for r in self.testing_target_bpps]
        skip_axis = list(self.testing_skip_rows)   # the skip rows take the axis alone (__init__): one (None, None, None) entry each
        axis = axis or [(None, None, None)] * len(skip_axis)
        # the tiled knobs take the same place: (None, step, target) with the tiled calls behind them
        tiled_axis = [(None, q, None) for q in self.testing_tile_qsteps] or [(None, None, r) for r in self.testing_tile_target_bpps]
        axis = axis or tiled_axis
        if hasattr(self.codec, "eval"):
            self.codec.eval()
        if self.force_testing_device and hasattr(self.codec, "to"):
            self.codec.to(self.force_testing_device)
        for _ in range(self.num_repeats):
            for ci, clevel in enumerate(vc if vc else [None]):
                rate_pts, distortion_pts = [], []
                for ri, (rlevel, qstep, bpp) in enumerate(axis if axis else [(None, None, None)]):
                    if skip_axis:
                        self._skip_rows = skip_axis[ri]
                    elif tiled_axis:
                        self._tile_qstep, self._tile_bpp = qstep, bpp
                    else:
                        self._qstep, self._target_bpp = qstep, bpp
                    if clevel is not None:
                        self.codec.set_complex_level(clevel)
                    if rlevel is not None:
                        self.codec.set_rate_level(rlevel)
                    if hasattr(self.codec, "post_training_process"):
                        self.codec.post_training_process()
                    self.codec.update_state()
                    if self.distortion_metric is not None:
                        self.distortion_metric.reset()
                    rate_prefix = [f"vrlevel{rlevel}"] if rlevel is not None else [f"q{qstep:g}"] if qstep is not None else \
                        [f"bpp{bpp:g}"] if bpp is not None else []
                    if tiled_axis:
                        rate_prefix = ["t" + rate_prefix[0]]
                    if skip_axis:
                        rate_prefix = [f"skip{skip_axis[ri]}"]
                    self._level_prefix = "_".join(([f"sclevel{clevel}"] if clevel is not None else []) + rate_prefix)
                    current = self._run_dataset()
                    if self.distortion_metric is not None:
                        current.update(**self.distortion_metric.collect_metrics())
                    prefixes = []
                    if clevel is not None:
                        prefixes.append(f"sclevel{clevel}")
                    if rate_prefix:
                        prefixes.extend(rate_prefix)
                        bj = self.testing_variable_rate_bj_delta_metric
                        if bj is not None:
                            rn, dn = bj.collect_metric_names
                            if rn in current and dn in current:
                                rate_pts.append(current[rn])
                                distortion_pts.append(current[dn])
                    prefix = "_".join(prefixes)
                    if prefixes:
                        metrics_2d.setdefault(prefix, OrderedDict())
                    for key, value in current.items():
                        metrics[f"{prefix}_{key}"] = value  # (sic: the reference keeps the underscore without a prefix)
                        if prefixes:
                            metrics_2d[prefix][key] = value
                    if len(vc) > 1 and hasattr(self.codec, "get_current_complex_metrics"):
                        for key, value in self.codec.get_current_complex_metrics().items():
                            metrics[f"{prefix}_{key}"] = value
                            if prefixes:
                                metrics_2d[prefix][key] = value
                # BD metric over this complexity level's rate points (needs at least 4 points, :979-992)
                bj = self.testing_variable_rate_bj_delta_metric
                if bj is not None and len(axis) > 3 and len(rate_pts) == len(axis):
                    bj_prefix = f"sclevel{ci}_" if vc else ""
                    value = bj((rate_pts, distortion_pts))[bj.name]
                    metrics[bj_prefix + bj.name] = value
                    metrics_2d[prefix][bj.name] = value
        self._qstep = self._target_bpp = self._tile_qstep = self._tile_bpp = self._skip_rows = None
        if metrics_2d and self.output_dir:
            self.save_metrics(metric_file=os.path.join(self.output_dir, "metrics_2d.csv"),
                              metric_data=list(metrics_2d.values()), names=list(metrics_2d.keys()), raw=False)
        return metrics

    def run_benchmark(self, *args, run_testing=True, ignore_exist_metrics=False, **kwargs):
        if self.codec is None:
            raise ValueError("No codec to benchmark!")
        if self.output_dir:
            os.makedirs(self.output_dir, exist_ok=True)
            if not ignore_exist_metrics and os.path.exists(self.metric_raw_file):
                with open(self.metric_raw_file, "rb") as f:  # the benchmark has been run: its metrics are the result
                    return pickle.load(f)
        if run_testing:
            metric_dict = self.run_testing(*args, **kwargs)
            if self.output_dir:
                self.save_metrics(metric_dict)
            return metric_dict

    # ---- base.py:54-112 (CSV: name column first, then metric columns in first-seen order, then hparams)
    def save_metrics(self, metric_data=None, hparams=None, names=None, metric_file=None, raw=True):
        metric_file = metric_file or self.metric_file
        if metric_data is None:
            return
        if raw:
            with open(self.metric_raw_file, "wb") as f:
                pickle.dump(metric_data, f)
        fieldnames, f_metrics, f_hparams, rows = OrderedDict(), OrderedDict(), OrderedDict(), []

        def _append(metric, hparam=None, name=None):
            row = OrderedDict()
            if isinstance(metric, dict):
                if name is not None:
                    fieldnames["name"] = None
                    row["name"] = name
                for k in metric:
                    f_metrics[k] = None
                row.update(**metric)
                if isinstance(hparam, dict):
                    for k in hparam:
                        f_hparams[k] = None
                    row.update(**hparam)
            rows.append(row)

        if isinstance(metric_data, (list, tuple)):
            hparams = hparams or [None] * len(metric_data)
            names = names or [None] * len(metric_data)
            for m, h, n in zip(metric_data, hparams, names):
                _append(m, h, n)
        else:
            _append(metric_data, hparams, names)
        with open(metric_file, "w", newline="") as f:
            writer = csv.DictWriter(f, fieldnames=list(fieldnames) + list(f_metrics) + list(f_hparams))
            writer.writeheader()
            writer.writerows(rows)
