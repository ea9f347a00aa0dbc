"""The mean-scale hyperprior graph on the CPU: oracle.codec_oracle's HyperpriorOracle with the mean-scale hyper transforms
(MS_H_A / MS_H_S), the prior chunked into (scales, means) along the channels as upstream's ``gaussian_params.chunk(2, 1)`` does, y
coded as ``round(y - mu)`` and rebuilt as ``symbol + mu``.  Torch CPU ops and the C rANS oracle only: no kernel of the library."""
import struct

import torch

from oracle.codec_oracle import MS_H_A, MS_H_S, HyperpriorOracle, gc_indexes, read_body, run_sequential


class MeanScaleOracle(HyperpriorOracle):
    def h_a(self, y): return run_sequential(self.sd, "latent_inference_modules.y_z.model", MS_H_A, y)
    def h_s(self, z): return run_sequential(self.sd, "latent_generative_modules.z_y.model", MS_H_S, z)

    def analyse(self, x):
        y = self.g_a(x)
        z = self.h_a(y)
        med = self.eb[3].reshape(1, -1, 1, 1)
        z_sym = torch.round(z - med)
        z_hat = z_sym + med
        prior = self.h_s(z_hat)[..., : y.shape[-2], : y.shape[-1]]
        scales, means = prior.chunk(2, 1)
        y_q = torch.round(y - means)
        return dict(y=y, z=z, z_sym=z_sym.int(), z_hat=z_hat, prior=prior, scales=scales, means=means, y_idx=gc_indexes(scales, self.table),
                    y_sym=y_q.int(), y_hat=y_q + means)

    def compress(self, x):
        return super().compress(x)   # the parent's framing of analyse()'s z and y symbols and indexes

    def decompress(self, data):
        (nz,) = struct.unpack("I", data[:4])
        bz, by = data[4:4 + nz], data[4 + nz:]
        z_strings, zshape = read_body(bz)
        C = self.eb[3].numel()
        z_idx = torch.arange(C, dtype=torch.int32).reshape(C, 1, 1).expand(C, *zshape).contiguous().numpy()
        z_sym = torch.stack([torch.from_numpy(self.z_dec.decode_with_indexes(s, z_idx)) for s in z_strings])
        z_hat = z_sym.float() + self.eb[3].reshape(1, -1, 1, 1)
        y_strings, yshape = read_body(by)
        scales, means = self.h_s(z_hat)[..., : yshape[0], : yshape[1]].chunk(2, 1)
        y_idx = gc_indexes(scales, self.table)
        y_sym = torch.stack([torch.from_numpy(self.y_dec.decode_with_indexes(s, y_idx[b].numpy())) for b, s in enumerate(y_strings)])
        return self.g_s(y_sym.float() + means)
