"""What a byte budget per tiled picture costs (INTEGRATION.md "Tiled pictures: step and byte budget"; output:
profiles/tiled_rate.txt).

Two workloads, uint8 pictures resident in HBM, one stream, every route warmed, alternating rounds in ONE process, medians and spreads:

  A. one 4096 x 6144 picture at tile 512 (96 tiles, max_batch 16);
  B. 24 Kodak-shaped pictures (768 x 512 and 512 x 768) at tile 256, pooled (max_batch 32).

For each: compress_tiled_to_rate (16 candidates, 1 / 2 / 3 passes) against compress_tiled_q at the step it chose -- the price of
choosing -- and against a host bisection of 8 compress_tiled_q calls, the only way to meet a budget without it.  The target is the
middle of the containers' lengths at steps 1 and 64, so that the script fixes no byte figure.

    python scripts/tiled_rate_probe.py [--rounds 3] [--reps 2] > profiles/tiled_rate.txt
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


def _pictures(shapes):
    out = []
    for i, (h, w) in enumerate(shapes):
        g = torch.Generator().manual_seed(i)
        x = torch.rand(1, 3, h, w, generator=g)
        x[..., : h // 2, :] = x[..., : h // 2, :] * 0.1 + 0.45      # a flat half: the tiles do not deserve equal bytes
        out.append((x * 255).round().to(torch.uint8).cuda())
    return out


def _timed(routes, rounds, reps):
    for _, fn in routes:
        fn()
    times = {name: [] for name, _ in routes}
    for _ in range(rounds):
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e3)
    return times


def _workload(codec, title, pics, kw, rounds, reps):
    q = lambda steps: codec.compress_tiled_items_q(pics, steps, **kw)
    L1, L64 = [len(c) for c in q(1.0)], [len(c) for c in q(64.0)]
    targets = [(a + b) // 2 for a, b in zip(L1, L64)]
    out, reps_ = codec.compress_tiled_items_to_rate(pics, target_bytes=targets, return_report=True, **kw)
    steps = [r["step"] for r in reps_]
    assert out == q(steps), "compress_tiled_items_to_rate must write compress_tiled_items_q's bytes at the steps it chose"
    calls = codec.last_items_calls

    def bisect():
        lo, hi = np.full(len(pics), np.log2(0.0625)), np.full(len(pics), np.log2(64.0))
        for _ in range(8):
            mid = (lo + hi) / 2
            fits = np.array([len(c) for c in q((2.0 ** mid).astype(np.float32))]) <= np.array(targets)
            hi, lo = np.where(fits, mid, hi), np.where(fits, lo, mid)
        return (2.0 ** hi).astype(np.float32)

    bis = np.array([len(c) for c in q(bisect())]) / np.array(targets)
    routes = [("compress_tiled_items_q at the chosen steps", lambda: q(steps))]
    routes += [(f"compress_tiled_items_to_rate, 16 candidates, {p} pass{'es' if p > 1 else ''}",
                lambda p=p: codec.compress_tiled_items_to_rate(pics, target_bytes=targets, passes=p, **kw)) for p in (1, 2, 3)]
    routes.append(("host bisection, 8 compress_tiled_items_q calls", bisect))
    times = _timed(routes, rounds, reps)
    tiles = sum(r["n_tiles"] for r in reps_)
    print(f"{title}: {len(pics)} picture(s), {tiles} tiles in {calls} pooled calls, {sum(p.shape[2] * p.shape[3] for p in pics) / 1e6:.1f} Mpix; "
          f"targets {min(targets)} .. {max(targets)} bytes")
    base = statistics.median(times[routes[0][0]])
    for name, _ in routes:
        print(_line(name, times[name], f"   {statistics.median(times[name]) / base:.3f} of the stated step"))
    for p in (1, 2, 3):
        _, r = codec.compress_tiled_items_to_rate(pics, target_bytes=targets, passes=p, return_report=True, **kw)
        fill = np.array([x["container_bytes"] / x["budget"] for x in r])
        over = max(x["predicted_bytes"] - x["container_bytes"] for x in r)
        print(f"   {p} pass(es): container / budget median {np.median(fill):.4f} min {fill.min():.4f} max {fill.max():.4f}; predicted - container "
              f"max {over} B; {sum(bool(x['met']) for x in r)} of {len(r)} met; steps {min(x['step'] for x in r):.4f} .. {max(x['step'] for x in r):.4f}")
    print(f"   after the bisection: container / budget median {np.median(bis):.4f} min {bis.min():.4f} max {bis.max():.4f}; "
          f"{int((bis <= 1).sum())} of {len(bis)} met")
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a quarter-size run of both workloads (a check of the script, not a figure)")
    args = ap.parse_args()
    from cbench_basic_amd.presets import hyperprior_codec, seed_synthetic_weights
    codec = seed_synthetic_weights(hyperprior_codec(), seed=0).eval().cuda()
    codec.update_state()
    print("A byte budget per tiled picture (scripts/tiled_rate_probe.py on one MI355X; see INTEGRATION.md, \"Tiled pictures: step and byte")
    print("budget\").  Every route warmed once, alternating rounds in one process, host clock around work that ends in a device synchronise.")
    print("The weights are seeded noise: bytes say where a budget lands, and mean nothing as R-D figures.  Nothing is gated on these figures.")
    print()
    print(f"hyperprior codec, seeded weights; {torch.cuda.get_device_name(0)}; uint8 pictures resident in HBM, one stream; median (min .. max) over "
          f"{args.rounds} alternating rounds of {args.reps} calls")
    print()
    big = (1024, 1536) if args.small else (4096, 6144)
    kodak = [(768, 512) if i % 3 == 0 else (512, 768) for i in range(6 if args.small else 24)]
    _workload(codec, "A. one large picture, tile 512, max_batch 16", _pictures([big]), dict(tile=512, max_batch=16), args.rounds, args.reps)
    _workload(codec, "B. Kodak-shaped pictures, tile 256, pooled, max_batch 32", _pictures(kodak), dict(tile=256, max_batch=32), args.rounds, args.reps)


if __name__ == "__main__":
    main()
