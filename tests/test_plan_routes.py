"""CPU: which kernels every plan of tools/plan_routes.py's matrix launches (networks x batches x precisions x forward route switches, and the
backward switches each alone; host-only plans: device = -1) is what tests/plan_routes.json records - creation status, op labels, launch
count, workspace bytes, backward summary, backward workspace bytes, bytes of the backward's packed weights.  The file is rewritten (python tools/plan_routes.py) only by a change that means to move a route; a refactor of the dispatch
leaves it as the build before it produced it."""

import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("plan_routes", os.path.join(ROOT, "tools", "plan_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_plan_of_the_matrix_routes_as_recorded():
    tool = _tool()
    with open(tool.TABLE) as f:
        want = json.load(f)
    got = tool.table()
    assert sorted(got) == sorted(want), f"matrix keys changed: {sorted(set(got) ^ set(want))[:8]}"
    assert len(got) >= 500 and sum(1 for v in got.values() if v["status"] == 0) >= 480
    bad = tool.mismatches(got, want)
    assert not bad, "plans that route differently (python tools/plan_routes.py --dump KEY shows one): " + ", ".join(
        f"{k}: {want[k]} -> {got[k]}" for k in bad[:6]) + (f" ... and {len(bad) - 6} more" if len(bad) > 6 else "")


def test_anchor_plans():
    """a few entries by value, so that a regenerated table is recognisable as the right baseline"""
    with open(_tool().TABLE) as f:
        want = json.load(f)
    for key, launches, ws in (("ddpm/b128/bf16", 45, 1_303_683_584), ("ddpm/b1/bf16", 57, 10_290_688), ("ddpm/b128/fp16r32", 53, 1_840_554_496),
                              ("ddpm/b128/fp32", 128, 2_460_885_504)):
        assert (want[key]["launches"], want[key]["workspace_bytes"]) == (launches, ws), key
    assert want["tiny/b8/fp16r32"] == {"status": -2}  # (no silent 16-bit fall-back)
    # the backward workspace: with and without the activated tensors the GroupNorm backward writes for the grouped weight gradient
    assert want["ddpm/b128/bf16"]["bwd_workspace_bytes"] == 2_128_814_848
    assert want["ddpm/b128/bf16/DMME_NO_WG_ACT"]["bwd_workspace_bytes"] == 1_449_337_600
