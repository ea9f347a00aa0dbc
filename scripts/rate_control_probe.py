"""What rate control of the hyperprior y coder costs and how close it lands (INTEGRATION.md "Rate control"; output:
profiles/rate_control.txt).

256 synthetic 3 x 256 x 256 images (image i = torch.manual_seed(i); torch.rand), resident in HBM, one stream, one session, every
route warmed, alternating rounds in ONE process, medians and spreads:

  1. the rate-curve kernel at 16 candidates against 16 rounds of gc_quantize_index_q + i32_to_f32 + gauss_nll_per_image(steps=) on
     the same y and sigma -- the only way to rate a step without it (device events around the launches);
  2. compress_to_rate (16 candidates, 2 passes) against compress_q at the steps it chose: the price of choosing;
  3. the same call against a host bisection of 8 compress_q calls, every image searching its own step;
  4. payload / budget per image at three budgets.

    python scripts/rate_control_probe.py [--images 256] [--size 256] [--rounds 3] [--reps 3] > profiles/rate_control.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _line(name, t, extra=""):
    med = statistics.median(t)
    return f"   {name:58s} {med:9.3f} ms ({min(t):.3f} .. {max(t):.3f}; spread {(max(t) - min(t)) / med:.3f} of the median){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from cbench_basic_amd.nn import kernels as K
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    from cbench_basic_amd.utils.rate import first_grid
    codec = seed_synthetic_weights(hyperprior_codec(), seed=0).eval().cuda()
    codec.update_state()
    ec = codec.entropy_coder
    imgs = []
    for i in range(args.images):
        torch.manual_seed(i)
        imgs.append(torch.rand(3, args.size, args.size))
    x = torch.stack(imgs).cuda()
    B, pixels = args.images, args.size ** 2

    # ---- 1. the kernel against the launches it replaces, on the graph's own y and sigma
    with torch.no_grad():
        y = ec.latent_inference_modules["x_y"](x)
        z = ec.latent_inference_modules["y_z"](y)
        zc, yc = ec.latent_node_entropy_coders["z"], ec.latent_node_entropy_coders["y"]
        yc._ready()
        scales = yc._crop(ec.latent_generative_modules["z_y"](zc(z)), *y.shape[-2:])
    cand = first_grid(16)
    cand_dev = torch.from_numpy(cand).cuda()

    def curve():
        return K.rate_curve(y, scales, cand_dev, yc._scale_table_dev, yc._tables, yc.scale_bound, 1)

    def estimate():
        out = []
        for c in cand:
            sym, _, _ = K.gc_quantize_index_q(y, scales, float(c), yc._scale_table_dev, yc.scale_bound, want_yhat=False)
            out.append(K.gauss_nll_per_image(K.i32_to_f32(sym), scales, False, yc.scale_bound, 1e-9, steps=float(c)))
        return out

    def device_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.reps

    bits = curve().cpu().numpy()
    nll = torch.stack(estimate()).cpu().numpy()                      # [16][B] nats
    kernel_t, est_t = [], []
    for _ in range(args.rounds):
        kernel_t.append(device_ms(curve))
        est_t.append(device_ms(estimate))
    read_bytes = 2 * 4 * y.numel()

    # ---- 2, 3. the call against compress_q at its steps, and against a host bisection
    budget = int(0.5 * pixels / 8)
    data, rep = codec.compress_to_rate(x, target_bpp=0.5, return_report=True)
    steps = rep["steps"]
    assert data == codec.compress_q(x, steps), "compress_to_rate must write compress_q's bytes at the steps it chose"

    def bisect():
        lo, hi = np.full(B, np.log2(0.0625)), np.full(B, np.log2(64.0))
        for _ in range(8):
            mid = (lo + hi) / 2
            inner = memoryview(codec.compress_q(x, (2.0 ** mid).astype(np.float32)))[8 + 4 * B:]
            fits = np.asarray(ec.payload_bytes(inner, B)) <= budget
            hi, lo = np.where(fits, mid, hi), np.where(fits, lo, mid)
        return (2.0 ** hi).astype(np.float32)

    bis_steps = bisect()
    bis_payload = np.asarray(ec.payload_bytes(memoryview(codec.compress_q(x, bis_steps))[8 + 4 * B:], B))
    routes = [("compress_q at the chosen steps", lambda: codec.compress_q(x, steps)),
              ("compress_to_rate, 16 candidates, 2 passes", lambda: codec.compress_to_rate(x, target_bpp=0.5)),
              ("compress_to_rate, 16 candidates, 1 pass", lambda: codec.compress_to_rate(x, target_bpp=0.5, passes=1)),
              ("compress_to_rate, 16 candidates, 3 passes", lambda: codec.compress_to_rate(x, target_bpp=0.5, passes=3)),
              ("host bisection, 8 compress_q calls", bisect)]
    for _, fn in routes:
        fn()
    times = {name: [] for name, _ in routes}
    for _ in range(args.rounds):
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.reps * 1e3)

    print("Rate control of the hyperprior y coder (scripts/rate_control_probe.py on one MI355X; see INTEGRATION.md, \"Rate control\").  Every")
    print("route warmed once, alternating rounds in one process.  The weights are seeded noise: bytes and bpp say where a budget lands, and")
    print("mean nothing as R-D figures.  Nothing is gated on these figures.")
    print()
    print(f"hyperprior codec, seeded weights; {torch.cuda.get_device_name(0)}; {B} float32 images of 3 x {args.size} x {args.size} resident in HBM, one stream;")
    print(f"y: {tuple(y.shape)}, {y.numel()} latents; median (min .. max) over {args.rounds} alternating rounds of {args.reps} passes")
    print()
    print("1. Rating 16 candidate steps (device events around the launches).  The cost table (64 rows x 3133 entries, 802 KB) is read where")
    print("   it lies, through L2: no window of it is staged in LDS.")
    km = statistics.median(kernel_t)
    print(_line("rate-curve kernel, 16 candidates, one launch", kernel_t,
                f"   {read_bytes / km / 1e6:.1f} GB/s of the single y + sigma read ({read_bytes / 1e6:.1f} MB)"))
    print(_line("16 x (gc_quantize_index_q + i32_to_f32 + gauss_nll(steps=))", est_t, f"   {statistics.median(est_t) / km:.2f} x the kernel"))
    tot_bits = bits.sum(0) / 65536.0
    est_bits = nll.sum(1) / np.log(2.0)
    print("   step, table cost of the batch (exact, bits), likelihood estimate (bits), ratio:")
    for k in range(0, 16, 3):
        ratio = f"{tot_bits[k] / est_bits[k]:.4f}" if est_bits[k] >= 1 else "-"
        print(f"      {cand[k]:8.4f}  {tot_bits[k]:14.0f}  {est_bits[k]:14.0f}  {ratio}")
    print()
    print(f"2, 3. One call at 0.5 bpp ({budget} bytes of payload per image), host clock around work that ends in a device synchronise.")
    base = statistics.median(times[routes[0][0]])
    for name, _ in routes:
        print(_line(name, times[name], f"   {statistics.median(times[name]) / base:.3f} of compress_q"))
    print(f"   payload / budget after the bisection: median {np.median(bis_payload / budget):.4f}, min {np.min(bis_payload / budget):.4f}, "
          f"max {np.max(bis_payload / budget):.4f}; {int((bis_payload <= budget).sum())} of {B} met")
    print()
    print("4. Where the payload lands (16 candidates; per image payload / budget, and predicted / budget):")
    for bpp in (0.25, 0.5, 1.0):
        for passes in (1, 2, 3):
            _, r = codec.compress_to_rate(x, target_bpp=bpp, passes=passes, return_report=True)
            q = r["payload_bytes"] / r["budget"]
            p = r["predicted_bytes"] / r["budget"]
            print(f"   {bpp:5.2f} bpp ({int(r['budget'][0]):6d} B), {passes} pass(es): payload / budget median {np.median(q):.4f} min {q.min():.4f} max {q.max():.4f}; "
                  f"predicted / budget median {np.median(p):.4f}; predicted - payload max {int((r['predicted_bytes'] - r['payload_bytes']).max())} B; "
                  f"{int(r['met'].sum())} of {B} met; steps {r['steps'].min():.4f} .. {r['steps'].max():.4f}")


if __name__ == "__main__":
    main()
