"""What the quantiser step of the hyperprior y coder costs (INTEGRATION.md "Quantiser step"; output: profiles/qstep.txt).

256 synthetic 3 x 256 x 256 images (image i = torch.manual_seed(i); torch.rand), resident in HBM, one stream, one session:
compress + decompress (the step-less route, whose launches the change leaves alone) against compress_q + decompress_q at step 1 and at
steps 0.5, 2 and 4 -- alternating in ONE process, every route warmed, three rounds, medians and spreads; plus the bytes and the PSNR
of every step.  A host clock around work that ends in a device synchronise.

    python scripts/qstep_probe.py [--images 256] [--size 256] [--rounds 3] [--reps 3] > profiles/qstep.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="compress + decompress passes timed together in a round")
    args = ap.parse_args()
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    codec = seed_synthetic_weights(hyperprior_codec(), seed=0).eval().cuda()
    codec.update_state()
    imgs = []
    for i in range(args.images):
        torch.manual_seed(i)
        imgs.append(torch.rand(3, args.size, args.size))
    x = torch.stack(imgs).cuda()
    routes = [("compress + decompress", None), ("compress_q, step 1", 1.0), ("compress_q, step 0.5", 0.5), ("compress_q, step 2", 2.0),
              ("compress_q, step 4", 4.0)]

    def once(step):
        if step is None:
            data = codec.compress(x)
            return data, codec.decompress(data)
        data = codec.compress_q(x, step)
        return data, codec.decompress_q(data)

    info = {}
    for name, step in routes:       # warm-up, and the figures that do not depend on the clock
        data, xhat = once(step)
        mse = ((xhat.clamp(0, 1) - x) ** 2).mean(dim=(1, 2, 3)).double()
        info[name] = (len(data), float((-10 * torch.log10(mse)).mean()))
    assert once(1.0)[0][12:] == once(None)[0], "step 1 must write the step-less bytes"
    times = {name: [] for name, _ in routes}
    for _ in range(args.rounds):
        for name, step in routes:   # alternating: every round visits every route
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                once(step)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.reps * 1e3)
    base = statistics.median(times[routes[0][0]])
    print("Quantiser step of the hyperprior y coder (scripts/qstep_probe.py on one MI355X; see INTEGRATION.md, \"Quantiser step\").  A host clock")
    print("around work that ends in a device synchronise, every route warmed once, three alternating rounds in one process; the step-less")
    print("route, whose launches the change leaves untouched, is the baseline of the same run.  The weights are seeded noise: the bytes and")
    print("the PSNR column say that the step moves the rate and the distortion in the expected directions, and mean nothing as R-D figures.")
    print("The expectation was that the step kernels (one division per latent more than the step-less ones) stay inside the run-to-run")
    print("spread of a step that takes tens of milliseconds; the last column is the figure, against the baseline row of this run.  Nothing")
    print("is gated on it.")
    print()
    print(f"hyperprior codec, seeded weights; {torch.cuda.get_device_name(0)}; {args.images} float32 images of 3 x {args.size} x {args.size} resident in HBM, "
          f"one stream; ms per compress + decompress of the batch, median (min .. max) over {args.rounds} alternating rounds of {args.reps} passes")
    print()
    for name, _ in routes:
        t = times[name]
        med = statistics.median(t)
        nbytes, psnr = info[name]
        print(f"   {name:24s} {nbytes:10d} bytes  {nbytes * 8 / (args.images * args.size ** 2):7.4f} bpp  PSNR {psnr:6.2f} dB   "
              f"{med:8.2f} ({min(t):.2f} .. {max(t):.2f}; spread {(max(t) - min(t)) / med:.3f} of the median)   {med / base:.3f} of the step-less route")


if __name__ == "__main__":
    main()
