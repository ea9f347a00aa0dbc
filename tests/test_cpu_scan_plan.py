"""The scan-line planner (cbench_basic_amd/csrc/scan_plan.h) needs no HIP and no device, so what it decides is checked here on the
CPU: csrc/scan_plan_check.cpp, a stand-alone program built with the host compiler (make scan_plan_check; a missing compiler
fails), replays every call of tests/golden/scanline_dispatch.json -- recorded on the device the table names, with the geometry of
each coder taken from the table's `plans` section -- and sweeps the invariants the spin-waiting kernels rest on: a planned grid is
resident (1 <= grid <= compute units), holds a compute unit alone (kMinLds <= LDS <= kMaxLds) and its launches cover the batch."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cbench_basic_amd", "csrc")

with open(os.path.join(ROOT, "tests", "golden", "scanline_dispatch.json")) as _f:
    TABLE = json.load(_f)
CUS = TABLE["compute_units"]
ROWS = [dict(zip(TABLE["fields"], r)) for r in TABLE["rows"]]
STREAMS = [dict(zip(TABLE["stream_fields"], r)) for r in TABLE["streams"]]
PLANS = {(p["kind"], p["C"]): p for p in TABLE["plans"]}
# a decode call's outcome depends on the decoder's LDS only through "<= 160 KiB": both ends of what a launch may hold
DECODER_LDS = (96 * 1024, 160 * 1024)


@pytest.fixture(scope="module")
def checker():
    subprocess.run(["make", "-s", "-C", CSRC, "scan_plan_check"], check=True, capture_output=True, text=True)
    return os.path.join(CSRC, "scan_plan_check")


def geometry_line(plan):
    g = plan["layers"]
    return " ".join(map(str, ["geometry", g["channels"], g["ctx_out"], g["ksize"], g["prior_channels"], len(g["dense_out"])] + g["dense_out"] +
                        g["act_after"] + g["dense_in_groups"]))


def call_line(plan, row, decoder_lds):
    return " ".join(map(str, ["call", row["batch"], row["H"], row["W"], row["direction"], row["schedule"], row["env"] or "none", plan["lane_max_batch"],
                              row.get("lanes", 1), int(row.get("rows", False)), plan["table_len"], decoder_lds, CUS]))


def run(checker, mode, lines):
    out = subprocess.run([checker, mode], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    return out


def replay_rows(checker, rows):
    """Every row through `replay` (a decode row at both DECODER_LDS) -> the rows whose outcome, launches or refusal are not the
    recorded ones, in words."""
    lines, asked = [], []
    for key, plan in PLANS.items():
        lines.append(geometry_line(plan))
        asked.append(None)
        for row in rows:
            if (row["kind"], row["C"]) == key:
                for lds in DECODER_LDS if row["direction"] == "decode" else (0,):
                    lines.append(call_line(plan, row, lds))
                    asked.append((plan, row, lds))
    assert sum(a is not None and a[2] in (0, DECODER_LDS[0]) for a in asked) == len(rows)   # no row is left out
    out = run(checker, "replay", lines)
    assert len(out) == len(lines)
    wrong = []
    for answer, a in zip(out, asked):
        if a is None:
            continue
        plan, row, lds = a
        outcome, launches, text = (answer.split(" ", 2) + [""])[:3]
        band_max = {(H, W): n for H, W, _, _, _, n in plan["limits"]}[row["H"], row["W"]]
        expect = -(-row["batch"] // band_max) if row["outcome"] == "band" else int(row["outcome"] not in ("per-step", "raises"))
        if outcome != row["outcome"] or int(launches) != row.get("launches", expect) or int(launches) != expect or \
                (outcome == "raises" and "does not fit" not in text):
            wrong.append(f"{row} decoder_lds {lds}: replay says {answer!r}, {expect} launches expected")
    return wrong


def test_recorded_table_replays_on_the_cpu(checker):
    assert len(ROWS) == 342
    wrong = replay_rows(checker, ROWS)
    assert not wrong, "\n".join(wrong)


def test_stream_rows_replay_on_the_cpu(checker):
    assert STREAMS and {r["lanes"] for r in STREAMS} == {1, 3, 12} and {r["rows"] for r in STREAMS} == {False, True}
    wrong = replay_rows(checker, STREAMS)
    assert not wrong, "\n".join(wrong)


def test_geometry_of_the_recorded_coders(checker):
    lines, expect = [], []
    for plan in PLANS.values():
        lines.append(geometry_line(plan))
        expect.append(f"geometry {plan['workgroups']} {plan['lds_weight_bytes'] // 4} {int(plan['batched'])} {plan['tile_workgroups']}")
        for H, W, *limits in plan["limits"]:
            lines.append(f"limits {H} {W} {CUS}")
            expect.append("limits " + " ".join(map(str, limits)))
    out = run(checker, "replay", lines)
    # (a plan that has not the batched kernel's shape: b_nw is not used and not compared)
    out = [" ".join(o.split()[:4] + ["0"]) if o.startswith("geometry") and o.split()[3] == "0" else o for o in out]
    assert out == expect, "\n".join(f"{q}: {o!r}, recorded {e!r}" for q, o, e in zip(lines, out, expect) if o != e)
    assert all(p["lds_weight_bytes"] % 4 == 0 for p in PLANS.values())


def test_sweep_finds_every_planned_launch_resident(checker):
    done = subprocess.run([checker, "sweep"], input="\n".join(geometry_line(p) for p in PLANS.values()) + "\n", capture_output=True, text=True)
    print(done.stdout)
    assert done.returncode == 0, done.stdout + done.stderr
    words = done.stdout.split()
    counts = dict(zip(words[::2], map(int, words[1::2])))
    assert counts["geometries"] == len(PLANS) == 3 and counts["violations"] == 0
    # the whole list, nothing excluded: three geometries x 3 compute-unit counts x 16 shapes x 14 batches x 2 directions x 4 schedules
    # x 6 forces x 2 gates x lanes and rows (decode), less what the entry points refuse before they plan
    assert counts["requests"] == 531216 and counts["planned"] + counts["refused"] + counts["per-step"] == counts["requests"]
