"""Metric accumulation, distortion and Bjontegaard-delta metrics.

Reference: ``cbench/utils/logger.py`` (MetricLogger: running means), ``cbench/benchmark/metrics/pytorch_distortion.py:12-60``
(PSNR over the whole batch), ``cbench/benchmark/metrics/bj_delta.py:6-94``.
"""
import math
from collections import OrderedDict

import numpy as np
import torch


class MetricLogger:
    """Running sums; ``get_global_average()`` -> {name: mean over all updates}."""

    def __init__(self):
        self._sum, self._cnt = OrderedDict(), OrderedDict()

    def update(self, **kwargs):
        for k, v in kwargs.items():
            if isinstance(v, torch.Tensor):
                v = v.item()
            self._sum[k] = self._sum.get(k, 0.0) + float(v)
            self._cnt[k] = self._cnt.get(k, 0) + 1

    def get_global_average(self):
        return OrderedDict((k, self._sum[k] / self._cnt[k]) for k in self._sum)

    def clear(self):
        self._sum.clear()
        self._cnt.clear()

    def merge(self, other):
        """Adds another logger's sums and counts (the per-worker loggers of a parallel run)."""
        for k in other._sum:
            self._sum[k] = self._sum.get(k, 0.0) + other._sum[k]
            self._cnt[k] = self._cnt.get(k, 0) + other._cnt[k]


def psnr_from_sse(sse, samples, peak=255.0):
    """PSNR in dB of ``samples`` samples whose squared errors sum to ``sse``: ``10 log10(peak^2 samples / sse)`` in float64, ``inf``
    for ``sse == 0``.  Scalars give a float, arrays an array.  The sum of an 8-bit picture is an exact integer
    (``nn/kernels.py::image_sse_u8``), so this is the only rounding between the picture and its PSNR."""
    sse, samples = np.asarray(sse, dtype=np.float64), np.asarray(samples, dtype=np.float64)
    with np.errstate(divide="ignore"):
        out = 10.0 * np.log10(np.float64(peak) ** 2 * samples / sse)
    return float(out) if out.ndim == 0 else out


class PytorchBatchedDistortion:
    """pytorch_distortion.py:21-68: ``"psnr"`` (of the mean squared error over the whole batch) and ``"ms-ssim"`` (mean over the
    batch; benchmark/ms_ssim.py restates the absent pytorch_msssim package: parity-unpinned).

    A pair of which BOTH sides are uint8 is measured as the 8-bit picture it is (not in the reference): the PSNR comes from the
    exact integer sum of squared differences against a peak of 255 (``max_val`` must be 1.0, read as "full range", or 255), ms-ssim
    from the pair converted to u8 / 255.  A pair with one float side takes the float path, as before."""

    def __init__(self, *args, metrics="psnr", max_val=1.0, **kwargs):
        self._metrics = metrics if isinstance(metrics, list) else [metrics]
        for m in self._metrics:
            if m not in ("psnr", "ms-ssim"):
                raise NotImplementedError(f"{m} is not implemented!")
        self.max_val = max_val
        self.metric_logger = MetricLogger()

    @property
    def name(self):
        return "&".join(self._metrics)

    @property
    def metrics(self):
        return self._metrics

    # ---- both sides uint8: the 8-bit picture itself
    @staticmethod
    def _is_u8_pair(output, target):
        return all(isinstance(t, torch.Tensor) and t.dtype == torch.uint8 for t in (output, target))

    def _sse_u8(self, output, target):
        """int64 [B, C] on the host: the exact sums of squared differences (the HIP kernel on the GPU, int64 torch ops on the CPU)."""
        if self.max_val not in (1.0, 255):
            raise ValueError(f"an 8-bit pair has a peak of 255: max_val is 1.0 (full range) or 255, not {self.max_val!r}")
        if output.is_cuda:
            from ..nn import kernels as K
            return K.image_sse_u8(output, target).cpu()
        return ((output.to(torch.int64) - target.to(torch.int64)) ** 2).sum((2, 3))

    @staticmethod
    def _ms_ssim_u8(output, target):
        """[B] MS-SSIM of a uint8 pair: the pair as u8 / 255 against a data range of 1."""
        if output.is_cuda:
            from ..nn import kernels as K
            return K.ms_ssim_per_image_u8(output, target)
        from .ms_ssim import ms_ssim   # image by image: a batched convolution may block its sums differently
        return torch.stack([ms_ssim(output[i:i + 1].float().div(255), target[i:i + 1].float().div(255), data_range=1.0, size_average=False)[0]
                            for i in range(target.shape[0])])

    def _per_item_u8(self, output, target):
        output = output[..., :target.shape[-2], :target.shape[-1]]  # make spatial size equal
        cols = {}
        if "psnr" in self._metrics:
            sse = self._sse_u8(output, target).sum(1).tolist()
            cols["psnr"] = [psnr_from_sse(s, target[0].numel()) for s in sse]
        if "ms-ssim" in self._metrics:
            cols["ms-ssim"] = self._ms_ssim_u8(output, target).tolist()
        return cols

    def __call__(self, output, target, cache_metrics=True):
        if self._is_u8_pair(output, target):
            output = output[..., :target.shape[-2], :target.shape[-1]]  # make spatial size equal
            result = {}
            if "psnr" in self._metrics:   # of the whole batch: total sum over total samples
                result["psnr"] = psnr_from_sse(int(self._sse_u8(output, target).sum()), target.numel())
            if "ms-ssim" in self._metrics:
                result["ms-ssim"] = float(self._ms_ssim_u8(output, target).mean())
            result = {m: result[m] for m in self._metrics}
            if cache_metrics:
                self.metric_logger.update(**result)
            return result
        output = output.type_as(target)[..., :target.shape[-2], :target.shape[-1]]  # make spatial size equal
        result = {}
        if "psnr" in self._metrics:
            if output.is_cuda:
                from ..nn import kernels as K
                mse = float(K.mse_per_image(output.contiguous(), target.contiguous()).double().mean())
            else:
                mse = torch.mean((output - target) ** 2).item()
            result["psnr"] = 20 * np.log10(self.max_val) - 10 * np.log10(mse)
        if "ms-ssim" in self._metrics:
            from .ms_ssim import ms_ssim
            result["ms-ssim"] = float(ms_ssim(output, target, data_range=self.max_val))
        result = {m: result[m] for m in self._metrics}   # the reference's order
        if cache_metrics:
            self.metric_logger.update(**result)
        return result

    def per_item(self, output, target, cache_metrics=True):
        """One result dict PER IMAGE of a batch (or of a list of ``[1, C, H, W]`` tensors of one shape), each what ``__call__`` gives
        for that image alone: psnr from the image's own mean squared error, ms-ssim from its own per-image value.  Every dict is
        logged as one update, so the running means equal those of N batch-1 calls."""
        if isinstance(output, (list, tuple)):
            output = output[0] if len(output) == 1 else torch.cat(list(output))
        if isinstance(target, (list, tuple)):
            target = target[0] if len(target) == 1 else torch.cat(list(target))
        N = target.shape[0]
        if self._is_u8_pair(output, target):
            cols = self._per_item_u8(output, target)
            results = [{m: cols[m][i] for m in self._metrics} for i in range(N)]
            if cache_metrics:
                for r in results:
                    self.metric_logger.update(**r)
            return results
        output = output.type_as(target)[..., :target.shape[-2], :target.shape[-1]]  # make spatial size equal
        cols = {}
        if "psnr" in self._metrics:
            if output.is_cuda:
                from ..nn import kernels as K
                mse = K.mse_per_image(output.contiguous(), target.contiguous()).double().tolist()
            else:
                mse = [torch.mean((output[i:i + 1] - target[i:i + 1]) ** 2).item() for i in range(N)]
            cols["psnr"] = [20 * np.log10(self.max_val) - 10 * np.log10(m) for m in mse]
        if "ms-ssim" in self._metrics:
            from .ms_ssim import ms_ssim
            if output.is_cuda:   # the fused kernel reduces image by image
                cols["ms-ssim"] = ms_ssim(output, target, data_range=self.max_val, size_average=False).tolist()
            else:                # image by image: a batched convolution may block its sums differently
                cols["ms-ssim"] = [float(ms_ssim(output[i:i + 1], target[i:i + 1], data_range=self.max_val, size_average=False)[0])
                                   for i in range(N)]
        results = [{m: cols[m][i] for m in self._metrics} for i in range(N)]   # the reference's order
        if cache_metrics:
            for r in results:
                self.metric_logger.update(**r)
        return results

    def collect_metrics(self):
        return self.metric_logger.get_global_average()

    def reset(self):
        self.metric_logger.clear()


def bj_delta(R1, PSNR1, R2, PSNR2, mode=0):
    """Bjontegaard delta (bj_delta.py:48-94): mode 0 = average PSNR difference, mode 1 = average rate difference in %,
    from cubic fits over log-rate integrated on the common interval."""
    lR1, lR2 = np.log(R1), np.log(R2)
    if mode == 0:
        p1, p2 = np.polyfit(lR1, PSNR1, 3), np.polyfit(lR2, PSNR2, 3)
        lo, hi = max(min(lR1), min(lR2)), min(max(lR1), max(lR2))
        i1, i2 = np.polyint(p1), np.polyint(p2)
        int1 = np.polyval(i1, hi) - np.polyval(i1, lo)
        int2 = np.polyval(i2, hi) - np.polyval(i2, lo)
        return (int2 - int1) / (hi - lo)
    p1, p2 = np.polyfit(PSNR1, lR1, 3), np.polyfit(PSNR2, lR2, 3)
    lo, hi = max(min(PSNR1), min(PSNR2)), min(max(PSNR1), max(PSNR2))
    i1, i2 = np.polyint(p1), np.polyint(p2)
    int1 = np.polyval(i1, hi) - np.polyval(i1, lo)
    int2 = np.polyval(i2, hi) - np.polyval(i2, lo)
    return (math.exp((int2 - int1) / (hi - lo)) - 1) * 100


class BJDeltaMetric:
    """bj_delta.py:6-45: called with (rate_pts, distortion_pts) of the tested codec against ``reference_pts``."""

    def __init__(self, reference_pts=None, collect_metric_names=("compressed_length", "psnr"), mode=0, **kwargs):
        assert mode in (0, 1)
        self.reference_pts, self.collect_metric_names, self.mode = reference_pts, collect_metric_names, mode
        self.metric_logger = MetricLogger()

    @property
    def name(self):
        return "BD-" + (self.collect_metric_names[1] if self.mode == 0 else "rate")

    def __call__(self, output, target=None):
        target = self.reference_pts if target is None else target
        (R1, P1), (R2, P2) = output, target
        try:
            result = {self.name: bj_delta(R1, P1, R2, P2, mode=self.mode)}
        except Exception:  # the reference swallows fit failures the same way
            result = {self.name: -100}
        self.metric_logger.update(**result)
        return result
