#!/usr/bin/env python3
"""Records which kernel serves a scan-line call: walks a fixed list of (coder, batch, H, W, direction, scanline_encode_schedule,
BASIC_SCAN_KERNEL) and writes one outcome per call to tests/golden/scanline_dispatch.json, with the device's compute-unit count
(the rules count workgroups against it):

    "per-step"   the coder's _scanline_plan returns None (nothing is run: the per-step path would code the call)
    "raises"     the call is refused ("does not fit")
    otherwise    ScanlinePlan.last_kernel() after _run_encode, or after decoding what the coder's defaults encoded

Two more sections let the planner (csrc/scan_plan.h) be checked without a GPU (tests/test_cpu_scan_plan.py):

    "plans"      per coder: the layer sizes its ScanlinePlan was made of, its table length and gate, and what the library reports
                 of the plan (scanline_cases.dispatch_plan)
    "streams"    decode calls over lane and row streams (lanes 1, 3, 12; rows off, on; BASIC_SCAN_KERNEL unset or a kernel with a
                 decode form) over the C = 192 shapes: the outcome and the launches ScanlinePlan.choose gives -- nothing is launched

tests/test_gpu_scanline_dispatch.py replays the table: a change of the host code must not change a row.  Run it on the GPU the
table is for, at the commit whose decisions are the reference:

    python scripts/scanline_dispatch_table.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import scanline_cases as sc  # noqa: E402

KERNELS = ("generic", "pipelined", "batched", "wavefront", "band")
SCHEDULES = ("auto", "raster", "wavefront", "band")
# 5x5 window, C = 192: Kodak-shaped latents, bench.py's 16x16 up to and past the raster kernels' 64 images, more images than the
# wavefront's 64 columns, a full wavefront, a latent narrower than ksize / 2 + 2, one taller than 64 rows, one too wide for a band
SHAPES = [("ctxmodel", 192, B, 32, 48) for B in (1, 2, 3, 8, 16)] + [("ctxmodel", 192, B, 16, 16) for B in (1, 4, 5, 33, 64, 96)] + \
         [("ctxmodel", 192, 65, 1, 4), ("ctxmodel", 192, 13, 4, 4), ("ctxmodel", 192, 2, 3, 2), ("ctxmodel", 192, 1, 70, 24),
          ("ctxmodel", 192, 1, 3, 130), ("ctxmodel-k3", 192, 1, 4, 3), ("ctxmodel-k3", 192, 3, 16, 16), ("merger", 32, 1, 5, 5)]


def calls():
    for shape in SHAPES:
        for direction in ("encode", "decode"):   # (a decode call ignores the schedule: crossed with it all the same)
            for schedule, env in [(s, None) for s in SCHEDULES] + [("auto", k) for k in KERNELS]:
                yield dict(zip(sc.DISPATCH_FIELDS, shape + (direction, schedule, env)))


def stream_calls():
    for shape in SHAPES:
        if shape[1] == 192:
            for lanes in (1, 3, 12):
                for rows in (False, True):
                    for env in (None, "wavefront", "batched", "pipelined", "generic"):
                        yield dict(zip(sc.STREAM_FIELDS, shape + ("decode", "auto", env, lanes, rows)))


def main():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows, cache = [], {}
    for row in calls():
        row["outcome"] = sc.dispatch_run(sc._shared_coder(row["kind"], row["C"]), row, cache)
        print(row, flush=True)
        rows.append(row)
    plans, streams, coders = [], [], {}
    for kind, C in sorted({s[:2] for s in SHAPES}):
        coder = sc._shared_coder(kind, C)
        coders[kind, C] = (coder, sc._plan_of(coder, C))
        shapes = sorted({s[3:] for s in SHAPES if s[:2] == (kind, C)})
        plans.append(dict(kind=kind, C=C, **sc.dispatch_plan(*coders[kind, C], shapes)))
    for row in stream_calls():
        row["outcome"], row["launches"] = sc.dispatch_choose(*coders[row["kind"], row["C"]], row)
        streams.append(row)
    path = os.path.join(ROOT, "tests", "golden", "scanline_dispatch.json")
    with open(path, "w") as f:
        f.write('{"compute_units": %d, "fields": %s, "rows": [\n' % (cus, json.dumps(list(sc.DISPATCH_FIELDS) + ["outcome"])))
        f.write(",\n".join(json.dumps([r[k] for k in sc.DISPATCH_FIELDS + ("outcome",)]) for r in rows))
        f.write('\n],\n"plans": [\n')
        f.write(",\n".join(json.dumps(p) for p in plans))
        f.write('\n],\n"stream_fields": %s, "streams": [\n' % json.dumps(list(sc.STREAM_FIELDS) + ["outcome", "launches"]))
        f.write(",\n".join(json.dumps([r[k] for k in sc.STREAM_FIELDS + ("outcome", "launches")]) for r in streams))
        f.write("\n]}\n")
    print(f"{len(rows)} rows, {len(plans)} plans, {len(streams)} stream rows -> {path}")


if __name__ == "__main__":
    main()
