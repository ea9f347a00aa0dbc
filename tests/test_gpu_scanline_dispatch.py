"""Which kernel serves a scan-line call is decided in one place, the planner of csrc/scanline.hip.  tests/golden/scanline_dispatch.json
(scripts/scanline_dispatch_table.py) holds what a fixed list of calls -- coder, batch, H, W, direction, scanline_encode_schedule,
BASIC_SCAN_KERNEL -- ran when it was recorded: a kernel's name, "per-step" (the coder leaves the call to its per-step path) or
"raises" (a refusal).  Every row must come out of ScanlinePlan.choose without a launch, with the launches the kernel needs, and
out of the coder's own path again: _scanline_plan, then the call where it leaves one, which must run that kernel.  The rules
count workgroups against the device's compute units, so the table holds for the device it names.
tests/test_cpu_scan_plan.py replays the same table through the planner alone (csrc/scan_plan.h) on the CPU, with each coder's layer
sizes taken from the table's `plans` section: the live coders must still have those, and the `streams` section (decode calls over
lane and row streams) must come out of ScanlinePlan.choose as recorded."""
import json
import os

import pytest
import torch

import scanline_cases as sc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scanline_dispatch.json")) as _f:
    TABLE = json.load(_f)
ROWS = [dict(zip(TABLE["fields"], r)) for r in TABLE["rows"]]
SHAPES = sorted({(r["kind"], r["C"], r["batch"], r["H"], r["W"]) for r in ROWS}, key=str)
STREAMS = [dict(zip(TABLE["stream_fields"], r)) for r in TABLE["streams"]]
_STREAMS = {}


@pytest.mark.parametrize("kind,C,B,H,W", SHAPES)
def test_dispatch_table_replays(kind, C, B, H, W):
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    if cus != TABLE["compute_units"]:
        pytest.skip(f"the table was recorded on a device of {TABLE['compute_units']} compute units, this one has {cus}")
    rows = [r for r in ROWS if (r["kind"], r["C"], r["batch"], r["H"], r["W"]) == (kind, C, B, H, W)]
    assert rows
    coder = sc._shared_coder(kind, C)
    sl = sc._plan_of(coder, C)
    wrong = []
    for row in rows:
        call = " ".join(f"{k}={row[k]}" for k in ("direction", "schedule", "env"))
        before = sl.last_kernel()
        chosen, launches = sc.dispatch_choose(coder, sl, row)
        assert sl.last_kernel() == before   # choose launches nothing
        if chosen != row["outcome"]:
            wrong.append(f"{call}: choose says {chosen}, recorded {row['outcome']}")
        # a band takes the launches its images per launch (basic_scanline_band_max) leave it, every other kernel one, no kernel none
        expect = -(-B // sl.band_max(H, W)) if chosen == "band" else int(chosen not in ("per-step", "raises"))
        if launches != expect:
            wrong.append(f"{call}: choose says {launches} launches of {chosen}, {expect} expected")
        ran = sc.dispatch_run(coder, row, _STREAMS)   # the coder's own path: _scanline_plan, then the call where there is one
        if ran != row["outcome"]:
            wrong.append(f"{call}: ran {ran}, recorded {row['outcome']}")
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("kind,C", sorted({s[:2] for s in SHAPES}))
def test_recorded_plans_are_the_live_coders(kind, C):
    """The fixture cannot drift from the coders: layer sizes, table length, gate and basic_scanline_plan_info are the recorded ones
    on any device; what counts compute units, on the table's."""
    recorded = next(p for p in TABLE["plans"] if (p["kind"], p["C"]) == (kind, C))
    coder = sc._shared_coder(kind, C)
    sl = sc._plan_of(coder, C)
    live = sc.dispatch_plan(coder, sl, [tuple(lim[:2]) for lim in recorded["limits"]])
    for k in ("layers", "table_len", "lane_max_batch", "workgroups", "lds_weight_bytes"):
        assert live[k] == recorded[k], k
    if torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count == TABLE["compute_units"]:
        assert live == {k: recorded[k] for k in live}


@pytest.mark.parametrize("kind,C", sorted({(r["kind"], r["C"]) for r in STREAMS}))
def test_stream_rows_replay(kind, C):
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    if cus != TABLE["compute_units"]:
        pytest.skip(f"the table was recorded on a device of {TABLE['compute_units']} compute units, this one has {cus}")
    coder = sc._shared_coder(kind, C)
    sl = sc._plan_of(coder, C)
    before = sl.last_kernel()
    wrong = [f"{row}: choose says {got}" for row in STREAMS if (row["kind"], row["C"]) == (kind, C)
             for got in [sc.dispatch_choose(coder, sl, row)] if got != (row["outcome"], row["launches"])]
    assert sl.last_kernel() == before   # choose launches nothing
    assert not wrong, "\n".join(wrong)
