"""The band decode launch of the scan-line coder (row streams), the parts that need no GPU: the planner
(cbench_basic_amd/csrc/scan_plan.h) replayed through csrc/scan_plan_check.cpp as test_cpu_scan_plan.py does.  The capacity of a
launch is restated here from its description -- an image owns A = W // s + 1 slots of one 32-column tile, a tile costs one set of
compute workgroups, a decoder wavefront serves one (image, slot, lane) and four of them share a workgroup, and everything is
resident at once -- and compared with what the planner answers; the decode schedule's outcomes are asked call by call; the decode
sweep must find every planned launch resident."""
import math
import os
import re
import subprocess
import sys

import pytest

from test_cpu_scan_plan import CSRC, CUS, PLANS, ROOT, geometry_line, run

UNITS = (64, 256, 304)


@pytest.fixture(scope="module")
def checker():
    subprocess.run(["make", "-s", "-C", CSRC, "scan_plan_check"], check=True, capture_output=True, text=True)
    return os.path.join(CSRC, "scan_plan_check")


def band_decode_capacity(plan, H, W, lanes, cus, band_max):
    """The largest n <= band_max with tiles(n) * workgroups per tile + ceil(n * min(A, H) * lanes / 4) <= compute units."""
    g = plan["layers"]
    if not plan["batched"] or g["channels"] % lanes or (lanes > 1 and (g["channels"] // lanes) % 16):
        return 0
    s = g["ksize"] // 2 + 2
    A = W // s + 1
    if A > 32:
        return 0
    ipt, per_tile = 32 // A, plan["tile_workgroups"]
    fits = [n for n in range(1, band_max + 1) if math.ceil(n / ipt) * per_tile + math.ceil(n * min(A, H) * lanes / 4) <= cus]
    return max(fits, default=0)


def test_limits_decode_is_the_formula(checker):
    lines, asked = [], []
    for plan in PLANS.values():
        lines.append(geometry_line(plan))
        asked.append(None)
        for H, W, *_, recorded in plan["limits"]:
            for cus in UNITS:
                lines.append(f"limits {H} {W} {cus}")
                asked.append(("band", recorded if cus == CUS else None))
                for lanes in (1, 3, 12):
                    lines.append(f"limits-decode {H} {W} {lanes} {cus}")
                    asked.append(("decode", plan, H, W, lanes, cus))
    out = run(checker, "replay", lines)
    assert len(out) == len(lines)
    band_max, seen = None, 0
    for line, answer, a in zip(lines, out, asked):
        if a is None:
            continue
        if a[0] == "band":   # the band's own limit at this unit count: the bound of the lines that follow (the recorded device: the table's)
            band_max = int(answer.split()[4])
            assert a[1] is None or band_max == a[1]
        else:
            _, plan, H, W, lanes, cus = a
            want = band_decode_capacity(plan, H, W, lanes, cus, band_max)
            assert answer == f"limits-decode {want}", f"{line}: {answer!r}, the formula gives {want} (band_max {band_max})"
            seen += want > 0
    assert seen >= 20   # the formula was exercised, not only zeros
    # the figures the issue's arithmetic gives for BaSIC's layers on 256 units: 12 / 9 / 4 images of 32 x 48 at 1 / 3 / 12 lanes
    basic = geometry_line(PLANS["ctxmodel", 192])
    assert run(checker, "replay", [basic] + [f"limits-decode 32 48 {k} 256" for k in (1, 3, 12)])[1:] == ["limits-decode 12", "limits-decode 9", "limits-decode 4"]


def call(batch, H, W, rows, decode_schedule=None, env="none", gate=4, lanes=1, cus=256, schedule="auto", direction="decode"):
    fields = ["call", batch, H, W, direction, schedule, env, gate, lanes, int(rows), 64, 96 * 1024, cus]
    return " ".join(map(str, fields + ([decode_schedule] if decode_schedule else [])))


def test_decode_schedule_outcomes(checker):
    basic = geometry_line(PLANS["ctxmodel", 192])
    asked = [
        (call(8, 32, 48, 1, "band"), "band 1"),
        (call(8, 32, 48, 1, "band", gate=-1), "band 1"),
        (call(3, 70, 24, 1, "band"), "band 1"),                       # taller than the wavefront's 64 columns
        (call(100, 32, 48, 1, "band", lanes=3), "band 12"),           # no raster kernel serves 100 images: the gate lets the band through
        (call(8, 32, 48, 1, env="band"), "band 1"),                   # the environment forces it the same way
        (call(8, 32, 48, 1, "band", env="batched"), "batched 1"),     # ... and wins over the schedule
        (call(8, 32, 48, 1, "raster"), "batched 1"),
        (call(2, 32, 48, 1, "wavefront"), "wavefront 1"),
        (call(2, 32, 48, 1, "raster", env="wavefront"), "wavefront 1"),
        (call(8, 32, 48, 1, "band", schedule="band"), "band 1"),      # the encode schedule stays ignored by decode calls
        (call(8, 32, 48, 1, "raster", schedule="band"), "batched 1"),
    ]
    out = run(checker, "replay", [basic] + [a for a, _ in asked])[1:]
    for (line, want), got in zip(asked, out):
        assert got == want, f"{line}: {got!r}, expected {want!r}"
    # a width whose slots exceed one tile: refused, before any launch, for a library call and through the coder's gate alike
    for gate in (-1, 4):
        for line in (call(1, 3, 130, 1, "band", gate=gate), call(1, 3, 130, 1, env="band", gate=gate), call(8, 32, 48, 1, "wavefront", gate=gate)):
            got = run(checker, "replay", [basic, line])[1]
            assert got.startswith("raises 0 ") and "does not fit" in got, f"{line}: {got!r}"


def test_rows_off_and_auto_are_unaffected(checker):
    basic = geometry_line(PLANS["ctxmodel", 192])
    lines, pairs = [basic], []
    for batch, H, W in [(1, 32, 48), (2, 32, 48), (8, 32, 48), (3, 70, 24), (1, 3, 130), (64, 16, 16), (100, 16, 16)]:
        for gate in (-1, 4):
            for env in ("none", "band", "wavefront", "batched"):
                for rows in (0, 1):
                    plain = call(batch, H, W, rows, env=env, gate=gate)
                    for ds in ("auto", "raster", "wavefront", "band") if not rows else ("auto",):
                        pairs.append((len(lines), len(lines) + 1))
                        lines += [plain, call(batch, H, W, rows, ds, env=env, gate=gate)]
    out = run(checker, "replay", lines)
    assert len(out) == len(lines)
    for i, j in pairs:
        assert out[i] == out[j], f"{lines[j]}: {out[j]!r}, without the field {out[i]!r}"
    # rows = 0 goes on ignoring BASIC_SCAN_KERNEL=band, as the recorded table says
    assert run(checker, "replay", [basic, call(8, 32, 48, 0, env="band"), call(8, 32, 48, 0)])[1:] == ["batched 1"] * 2


def test_sweep_decode_finds_every_planned_launch_resident(checker):
    done = subprocess.run([checker, "sweep-decode"], input="\n".join(geometry_line(p) for p in PLANS.values()) + "\n", capture_output=True, text=True)
    print(done.stdout)
    assert done.returncode == 0, done.stdout + done.stderr
    words = done.stdout.split()
    counts = dict(zip(words[::2], map(int, words[1::2])))
    assert counts["geometries"] == len(PLANS) == 3 and counts["violations"] == 0
    assert counts["requests"] > 0 and counts["planned"] > 0 and counts["refused"] > 0
    assert counts["planned"] + counts["refused"] + counts["per-step"] == counts["requests"]


def test_new_entries_are_declared_with_prototypes():
    from cbench_basic_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "basic_hip.h")).read()
    for name in ("basic_scanline_set_decode_schedule", "basic_scanline_band_decode_max"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._SIGNATURES, name
    sig = _lib._SIGNATURES
    assert sig["basic_scanline_set_decode_schedule"] == sig["basic_scanline_set_encode_schedule"]
    assert len(sig["basic_scanline_band_decode_max"][1]) == len(sig["basic_scanline_band_max"][1]) + 2   # the table set and the lanes


def test_the_tool_wants_row_streams_for_a_decode_schedule(tmp_path):
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_benchmark.py"), "--codec", "basic", "--scanline-decode-schedule", "band",
                           "--out", str(tmp_path)], capture_output=True, text=True)
    assert done.returncode == 2 and "--stream-rows" in done.stderr, done.stderr
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_benchmark.py"), "--codec", "basic", "--stream-rows",
                           "--scanline-decode-schedule", "diagonal", "--out", str(tmp_path)], capture_output=True, text=True)
    assert done.returncode == 2 and "invalid choice" in done.stderr, done.stderr
