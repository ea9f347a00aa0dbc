"""GeneralCodec -- cbench/codecs/general_codec.py:18-130,320-346 restricted to the
``entropy_coder``-only configuration every north-star experiment uses
(configs/lossy_graph_scalable_exp_hp.py, configs/lossy_latent_graph_topogroup.py: the latent
graph IS the entropy coder; preprocessor / prior_model / context_model slots are None)."""
from ..base import HotPathModule
from .base import (CodecInterface, VariableComplexityCodecInterface, VariableRateCodecInterface,
                   VariableTaskCodecInterface)


class GeneralCodec(HotPathModule, CodecInterface, VariableRateCodecInterface, VariableComplexityCodecInterface,
                   VariableTaskCodecInterface):
    def __init__(self, *args, preprocessor=None, prior_model=None, context_model=None, entropy_coder=None,
                 prior_first=False, **kwargs):
        super().__init__()
        if preprocessor is not None or prior_model is not None or context_model is not None:
            raise NotImplementedError("only the entropy_coder slot is on the MI355X hot path (SURVEY 8a a1)")
        self.entropy_coder = entropy_coder
        self.prior_first = prior_first

    def compress(self, data, *args, **kwargs):
        # general_codec.py:46-47: the upload is part of compress().  The latent-graph coder does it itself (on its
        # stream, asynchronously from page-locked memory), so a host batch is handed over as it is.
        if data.device != self.device and not (data.device.type == "cpu" and hasattr(self.entropy_coder, "_fused_session")):
            data = data.to(device=self.device)
        with self.profiler.start_time_profile("time_compress_entropy_coder"):
            return self.entropy_coder.encode(data, *args, prior=None, **kwargs)

    def decompress(self, data, *args, **kwargs):
        with self.profiler.start_time_profile("time_decompress_entropy_coder"):
            return self.entropy_coder.decode(data, *args, prior=None, **kwargs)

    def compress_q(self, data, qstep, *args, **kwargs):
        """``compress`` under a quantiser step of the y latent (INTEGRATION.md "Quantiser step"; the hyperprior codec's rate knob,
        not part of the reference's codec interface): ``qstep`` is one step for the batch or one per image, finite and in
        [2^-4, 2^6].  -> the container of utils/qstep.py: b"BQS1", uint32 LE n, n float32 LE steps, then exactly what
        ``entropy_coder.encode(data, qstep=qstep)`` returned -- at step 1 that is ``compress(data)`` byte for byte."""
        from ..utils.qstep import check_qsteps, pack_qsteps
        steps = check_qsteps(qstep, data.shape[0])
        return pack_qsteps(steps, self.compress(data, *args, qstep=steps, **kwargs))

    def decompress_q(self, data, *args, output_dtype=None, **kwargs):
        """A container of compress_q -> the reconstruction, as ``decompress`` gives it (``output_dtype`` as there).  The steps are
        read from the container; a wrong magic, a short buffer or a step count that is neither 1 nor the batch of the inner
        stream is a ValueError raised before anything is launched."""
        from ..utils.qstep import unpack_qsteps
        steps, inner = unpack_qsteps(data)
        return self.decompress(inner, *args, output_dtype=output_dtype, qstep=steps, **kwargs)

    def compress_skip(self, data, skip_rows, qstep=None, *args, **kwargs):
        """``compress`` with skip coding of the y latent (INTEGRATION.md "Skip coding"; the hyperprior codecs, not part of the
        reference's codec interface): an element whose table row is below ``skip_rows`` -- an integer in [0, rows of the scale table];
        utils.skip.skip_rows_for_sigma states it as a scale -- is not coded, and decodes as 0 (the mean, for the mean-scale codec).
        ``qstep``: None, or the quantiser step(s) of compress_q; the rows are then those of sigma / step.  -> the container of
        utils/skip.py: b"BSK1", uint32 LE skip_rows, uint32 LE n (0 without a step), n float32 LE steps, then exactly what
        ``entropy_coder.encode(data, skip_rows=, qstep=)`` returned -- at skip_rows 0 that is ``compress(data)``, or the inner stream
        of ``compress_q(data, qstep)``, byte for byte.  No rate target, tiles or autoregressive codec with it (ValueError / TypeError)."""
        from ..utils.qstep import check_qsteps
        from ..utils.skip import check_skip_rows, pack_skip
        r = check_skip_rows(skip_rows)
        steps = None if qstep is None else check_qsteps(qstep, data.shape[0])
        extra = {} if steps is None else dict(qstep=steps)
        return pack_skip(r, steps, self.compress(data, *args, skip_rows=r, **extra, **kwargs))

    def decompress_skip(self, data, *args, output_dtype=None, **kwargs):
        """A container of compress_skip -> the reconstruction, as ``decompress`` gives it (``output_dtype`` as there).  The skip rows
        and the steps are read from the container; a wrong magic, a short buffer, rows past the table or invalid steps are a ValueError
        raised before anything is launched."""
        from ..utils.skip import unpack_skip
        r, steps, inner = unpack_skip(data)
        extra = {} if steps is None else dict(qstep=steps)
        return self.decompress(inner, *args, output_dtype=output_dtype, skip_rows=r, **extra, **kwargs)

    def compress_to_rate(self, data, target_bytes=None, target_bpp=None, candidates=16, passes=2, step_range=(2 ** -4, 2 ** 6),
                         return_report=False, **kwargs):
        """``compress_q`` with the step of every image chosen on the GPU so that the image's payload -- its z stream plus its y
        stream(s); not the fixed framing -- fits a byte budget (INTEGRATION.md "Rate control").  Give exactly one target, a number or one
        per image: ``target_bytes``, or ``target_bpp`` (budget = floor(bpp * H * W / 8)).  ``candidates`` steps, log-spaced over
        ``step_range``, are rated in one pass over the latent and the smallest that fits is refined ``passes - 1`` times between
        itself and its lower neighbour.  -> the BQS1 container of compress_q with one step per image (``decompress_q`` reads it),
        byte for byte ``compress_q(data, those steps)``; with ``return_report`` also a dict of per-image ``steps``,
        ``predicted_bytes``, ``payload_bytes``, ``budget`` and ``met`` (payload <= budget).  An image no candidate fits takes the
        largest step and reports ``met`` False.  ValueError for an invalid request, before anything is launched."""
        import numpy as np
        from ..utils.qstep import pack_qsteps
        from ..utils.rate import RateTarget, budgets_from, first_grid
        if data.dim() != 4:
            raise ValueError(f"compress_to_rate takes a [B, C, H, W] batch, got shape {tuple(data.shape)}")
        B, _, H, W = data.shape
        budgets = budgets_from(target_bytes, target_bpp, B, H, W)
        rt = RateTarget(budgets, first_grid(candidates, step_range), passes, batch=B)
        inner = self.compress(data, rate_target=rt, **kwargs)
        out = pack_qsteps(rt.steps, inner)
        if not return_report:
            return out
        payload = np.asarray(self.entropy_coder.payload_bytes(inner, B), dtype=np.int64)
        want = rt.budgets_for(B)
        return out, dict(steps=rt.steps, predicted_bytes=rt.predicted_bytes, payload_bytes=payload, budget=want, met=payload <= want,
                         fits=rt.fits)

    def compress_items(self, items, *args, max_batch=None, **kwargs):
        """N batch-1 items -> exactly ``[self.compress(x) for x in items]``, items of one shape coded in shared batches
        (entropy coder's ``encode_items``; not part of the reference's codec interface)."""
        with self.profiler.start_time_profile("time_compress_entropy_coder"):
            return self.entropy_coder.encode_items(items, *args, max_batch=max_batch, **kwargs)

    def decompress_items(self, strings, *args, max_batch=None, **kwargs):
        """N batch-1 strings -> their reconstructions, ``[1, C, H, W]`` each, equal to ``self.decompress(s)`` of every string."""
        with self.profiler.start_time_profile("time_decompress_entropy_coder"):
            return self.entropy_coder.decode_items(strings, *args, max_batch=max_batch, **kwargs)

    def compress_tiled(self, image, *args, tile=(512, 512), max_batch=None, overlap=0, pad_to=1, **kwargs):
        """One picture ``[1, C, H, W]`` -> the container of its independently coded tiles (utils/tiling.py), tile k's string exactly
        ``self.compress(image[:, :, y:y + h, x:x + w])`` (entropy coder's ``encode_tiled``).  ``overlap`` (int or ``(oy, ox)``, at most
        half a tile): neighbouring tiles share that many rows / columns, and decompress_tiled cross-fades the seams.  ``pad_to`` (int or
        ``(py, px)``, dividing the tile): an edge tile is coded at its size rounded up to multiples of py x px, the picture's last row
        and column replicated, and decompress_tiled crops it; 1, the default, pads nothing."""
        with self.profiler.start_time_profile("time_compress_entropy_coder"):
            return self.entropy_coder.encode_tiled(image, *args, tile=tile, max_batch=max_batch, overlap=overlap, pad_to=pad_to, **kwargs)

    def decompress_tiled(self, data, *args, **kwargs):
        """A container of compress_tiled -> the picture at its own size, or the ``region`` of it (entropy coder's ``decode_tiled``);
        the overlap and the padding of the tiles, if any, are read from the container."""
        with self.profiler.start_time_profile("time_decompress_entropy_coder"):
            return self.entropy_coder.decode_tiled(data, *args, **kwargs)

    def compress_tiled_items(self, pictures, *args, tile=(512, 512), overlap=0, max_batch=None, pad_to=1, **kwargs):
        """N pictures ``[1, C, H, W]`` of any sizes -> their N containers, exactly ``[self.compress_tiled(p, tile=, overlap=, pad_to=)
        for p in pictures]``, the tiles of all pictures pooled into shared coding calls (entropy coder's ``encode_tiled_items``); with
        ``pad_to=tile`` every tile of every picture has one size."""
        with self.profiler.start_time_profile("time_compress_entropy_coder"):
            return self.entropy_coder.encode_tiled_items(pictures, *args, tile=tile, overlap=overlap, max_batch=max_batch, pad_to=pad_to,
                                                         **kwargs)

    def decompress_tiled_items(self, containers, *args, **kwargs):
        """N containers -> their N pictures, each equal to ``self.decompress_tiled(container)`` (entropy coder's
        ``decode_tiled_items``)."""
        with self.profiler.start_time_profile("time_decompress_entropy_coder"):
            return self.entropy_coder.decode_tiled_items(containers, *args, **kwargs)

    # ---- tiled pictures under a quantiser step, stated or chosen for a byte budget (INTEGRATION.md "Tiled pictures: step and byte
    # budget"; the hyperprior codec).  decompress_tiled / decompress_tiled_items read the BTQ1 containers these return.
    def compress_tiled_q(self, image, qstep, tile=(512, 512), overlap=0, pad_to=1, max_batch=None):
        """``compress_tiled`` under a quantiser step: ``qstep`` is one step, or one per tile in grid order.  -> a BTQ1 container
        (utils/tiling.py), tile k's string exactly ``compress_q(P_k, step_k)[12:]`` of the tile compress_tiled cuts."""
        with self.profiler.start_time_profile("time_compress_entropy_coder"):
            return self.entropy_coder.encode_tiled_q(image, qstep, tile=tile, max_batch=max_batch, overlap=overlap, pad_to=pad_to)

    def compress_tiled_items_q(self, pictures, qsteps, tile=(512, 512), overlap=0, pad_to=1, max_batch=None):
        """``compress_tiled_items`` under quantiser steps, one for all or one per picture: N BTQ1 containers, each byte for byte
        ``compress_tiled_q`` of its picture, from the same pooled calls as the step-less method."""
        with self.profiler.start_time_profile("time_compress_entropy_coder"):
            return self.entropy_coder.encode_tiled_items_q(pictures, qsteps, tile=tile, overlap=overlap, max_batch=max_batch, pad_to=pad_to)

    def compress_tiled_to_rate(self, image, target_bytes=None, target_bpp=None, tile=(512, 512), overlap=0, pad_to=1, max_batch=None,
                               candidates=16, passes=2, step_range=(2 ** -4, 2 ** 6), return_report=False, workspace_limit=2 << 30):
        """``compress_tiled_q`` with the picture's ONE step chosen on the GPU so that the whole container, framing included, fits a byte
        budget: ``target_bytes``, or ``target_bpp`` (budget = floor(bpp * H * W / 8)).  -> the container, byte for byte
        ``compress_tiled_q(image, that step)``; with ``return_report`` also a dict of ``step``, ``predicted_bytes``,
        ``container_bytes``, ``budget``, ``met``, ``fits``, ``n_tiles`` and per-tile ``predicted_payload`` / ``payload``.  When nothing
        fits the picture takes the largest step and ``met`` is False.  ValueError, before anything is launched, for an invalid request,
        a budget not above the framing, or latents past ``workspace_limit`` bytes."""
        with self.profiler.start_time_profile("time_compress_entropy_coder"):
            return self.entropy_coder.encode_tiled_to_rate(image, target_bytes=target_bytes, target_bpp=target_bpp, tile=tile, overlap=overlap,
                                                           pad_to=pad_to, max_batch=max_batch, candidates=candidates, passes=passes,
                                                           step_range=step_range, return_report=return_report,
                                                           workspace_limit=workspace_limit)

    def compress_tiled_items_to_rate(self, pictures, target_bytes=None, target_bpp=None, tile=(512, 512), overlap=0, pad_to=1,
                                     max_batch=None, candidates=16, passes=2, step_range=(2 ** -4, 2 ** 6), return_report=False,
                                     workspace_limit=2 << 30):
        """``compress_tiled_to_rate`` of N pictures, one target for all or one each, the tiles pooled as in ``compress_tiled_items``:
        N containers, each byte for byte ``compress_tiled_to_rate`` of its picture alone; the reports come as a list."""
        with self.profiler.start_time_profile("time_compress_entropy_coder"):
            return self.entropy_coder.encode_tiled_items_to_rate(pictures, target_bytes=target_bytes, target_bpp=target_bpp, tile=tile,
                                                                 overlap=overlap, pad_to=pad_to, max_batch=max_batch, candidates=candidates,
                                                                 passes=passes, step_range=step_range, return_report=return_report,
                                                                 workspace_limit=workspace_limit)

    @property
    def last_items_calls(self):
        return self.entropy_coder.last_items_calls

    @property
    def last_tiles_decoded(self):
        return self.entropy_coder.last_tiles_decoded

    def forward(self, data, *args, **kwargs):
        return self.entropy_coder(data, *args, **kwargs)

    def forward_estimate_bitlen(self, data, *args, **kwargs):
        """general_codec.py:190-209: (reconstruction, estimated compressed size in BYTES) from the entropy
        coder's cached rate estimate (prior_entropy is in nats per image)."""
        import math
        import torch
        with torch.no_grad():
            result = self.forward(data, *args, **kwargs)
            estimated_bitlen = 0
            pe = self.entropy_coder.get_raw_cache("metric_dict").get("prior_entropy") \
                if hasattr(self.entropy_coder, "get_raw_cache") else None
            if pe is not None:
                estimated_bitlen = estimated_bitlen + pe * data.size(0) / math.log(2)
            return result, estimated_bitlen / 8

    def update_state(self, *args, **kwargs) -> None:  # general_codec.py:320-326
        for m in self.children():
            if hasattr(m, "update_state"):
                m.update_state(*args, **kwargs)

    def post_training_process(self, *args, **kwargs):
        for m in self.children():
            if hasattr(m, "post_training_process"):
                m.post_training_process(*args, **kwargs)

    # variable rate / complexity / task plumbing (general_codec.py:328-360)
    def set_rate_level(self, level, *args, **kwargs):
        return self.entropy_coder.set_rate_level(level, *args, **kwargs)

    @property
    def num_rate_levels(self):
        return self.entropy_coder.num_rate_levels

    def set_complex_level(self, level, *args, **kwargs):
        return self.entropy_coder.set_complex_level(level, *args, **kwargs)

    def get_current_complex_metrics(self, *args, **kwargs):
        return self.entropy_coder.get_current_complex_metrics(*args, **kwargs)

    @property
    def num_complex_levels(self):
        return self.entropy_coder.num_complex_levels

    def set_task(self, task, *args, **kwargs):
        return self.entropy_coder.set_task(task, *args, **kwargs)

    @property
    def num_tasks(self):
        return self.entropy_coder.num_tasks
