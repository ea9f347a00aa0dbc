"""Image ingest for the benchmark harness.

* ``ImageFolderDataset``: PNG/JPEG files -> float32 CHW in [0, 1] (``ToTensor``: uint8 / 255), the Kodak path of
  ``cbench/data/datasets/torchvision_datasets.py:80-88``.
* ``RandomImageDataset``: the synthetic generator of ``configs/datasets/images/random_image_generator.py:12-15``
  (image i = ``torch.manual_seed(i); torch.rand(3, H, W)``).

With ``dtype=torch.uint8`` both yield 8-bit images for the codec's uint8 path ("8-bit images"): the folder
dataset hands out the decoder's own [H][W][C] array as a permuted [C, H, W] view -- no copy, no float pass, no division on the
host; the codec uploads the bytes and converts them on the GPU.
"""
import os

import numpy as np
import torch


def _image_dtype(dtype):
    if dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"an image dataset yields torch.float32 or torch.uint8, not {dtype}")
    return dtype


class ImageFolderDataset:
    EXT = (".png", ".jpg", ".jpeg", ".bmp", ".ppm")

    def __init__(self, root, max_num=None, dtype=torch.float32):
        self.dtype = _image_dtype(dtype)
        self.files = sorted(os.path.join(root, f) for f in os.listdir(root) if f.lower().endswith(self.EXT))
        if max_num is not None:
            self.files = self.files[:max_num]

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        from PIL import Image
        with Image.open(self.files[i]) as im:
            a = np.array(im.convert("RGB"), dtype=np.uint8)  # own, writable copy
        if self.dtype == torch.uint8:
            return torch.from_numpy(a).permute(2, 0, 1)   # the decoder's array itself, seen as [C, H, W]
        return torch.from_numpy(a).permute(2, 0, 1).contiguous().float().div_(255.0)


class RandomImageDataset:
    def __init__(self, num=8, size=(3, 256, 256), dtype=torch.float32):
        self.num, self.size, self.dtype = num, tuple(size), _image_dtype(dtype)

    def __len__(self):
        return self.num

    def __getitem__(self, i):
        if not 0 <= i < self.num:
            raise IndexError(i)
        torch.manual_seed(i)
        if self.dtype == torch.uint8:
            return torch.randint(0, 256, self.size, dtype=torch.uint8)
        return torch.rand(*self.size)


def batched(dataset, batch_size=1):
    """Minimal DataLoader: stacks ``batch_size`` equally sized images (the reference tests with batch_size=1)."""
    buf = []
    for i in range(len(dataset)):
        buf.append(dataset[i])
        if len(buf) == batch_size:
            yield _stack(buf)
            buf = []
    if buf:
        yield _stack(buf)


def _stack(buf):
    # uint8 [C, H, W] views of decoders' [H][W][C] arrays stay in that order: the batch is [B, C, H, W] over [B][H][W][C] memory
    # (one item: the array itself), which the codec reads as it lies
    if all(t.dtype == torch.uint8 and t.dim() == 3 and t.shape[0] > 1 and t.permute(1, 2, 0).is_contiguous() for t in buf):
        if len(buf) == 1:
            return buf[0][None]
        return torch.stack([t.permute(1, 2, 0) for t in buf]).permute(0, 3, 1, 2)
    return torch.stack(buf)
