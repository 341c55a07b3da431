"""The host-side plan of a render call, pinned without a GPU: tests/plan_table.json (tools/gen_plan_table.py) records route,
gradient layout, workspace sizes / offsets, scratch sizes and early statuses for a few hundred (grid, cfg, dispatch, R) cases;
the current build must reproduce every entry exactly."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT
from voxe_hip import abi


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_plan_table", os.path.join(ROOT, "tools", "gen_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table(gen):
    """[(case, plan)] with plan as gen.evaluate() returns it"""
    t = json.load(open(gen.TABLE))
    assert t["keys"] == gen.KEYS
    return [(case, dict(zip(t["keys"], scalars), sched=sched, region=region)) for case, scalars, sched, region in t["rows"]]


def test_table_covers_every_route_layout_and_optional_buffer(table):
    """the conditions that keep the comparison below from being vacuous"""
    plans = [plan for _, plan in table]
    assert len(table) >= 200
    routes = {p["route"] for p in plans}
    assert {abi.ROUTE_NONE, abi.ROUTE_SCATTER, abi.ROUTE_TILE, abi.ROUTE_PACKED_SCATTER, abi.ROUTE_REGION,
            abi.ROUTE_DETERMINISTIC} <= routes
    layouts = {p["bwd_layout"] for p in plans}
    assert {abi.GRAD_LINEAR, abi.GRAD_BRICKED, abi.GRAD_ANY} <= layouts
    sched = [p["sched"] for p in plans if p["sched"][0] == abi.OK]
    assert any(s[1] == 1 for s in sched) and any(s[1] == 0 for s in sched)
    assert any(p["region"][0] == abi.OK and len(p["region"]) == 18 for p in plans)
    assert any(p["region"][0] == abi.ERR_UNSUPPORTED for p in plans)
    # both workspace tiers differ somewhere, and every early status occurs
    assert any(p["workspace_bytes"] > p["workspace_bytes_inference"] > 0 for p in plans)
    for key in ("render_fwd", "render_bwd", "render_bwd_acc", "render_bwd_acc_into", "sample_probe"):
        assert {abi.ERR_NULL_POINTER, abi.ERR_BAD_SHAPE, abi.ERR_UNSUPPORTED, abi.ERR_WORKSPACE} <= {p[key] for p in plans}, key
    # a NULL workspace never gets past the checks
    assert all(p[key] != abi.OK for p in plans for key in ("render_fwd", "render_bwd", "sample_probe"))


def test_generator_cases_are_the_recorded_ones(gen, table):
    assert json.loads(json.dumps(gen.cases())) == [case for case, _ in table]


def test_current_build_reproduces_the_plan_table(gen, table):
    lib = gen.load_library()
    wrong = []
    for i, (case, plan) in enumerate(table):
        got = gen.evaluate(lib, case)
        if got != plan:
            wrong.append((i, case, {k: (plan.get(k), got[k]) for k in got if got[k] != plan.get(k)}))
    assert not wrong, f"{len(wrong)} of {len(table)} cases differ; first: {wrong[0]}"
