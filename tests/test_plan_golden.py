"""CPU: the planner's output over an enumerated sweep (tests/plan_sweep.py) equals
the recorded one.  tests/golden/plan_digests.json holds one digest per (option
setting, head dim, K/V type pair) of every case's return code, workspace size
and fattn_describe text, recorded before the planner was restructured: a
host-side refactor must leave every plan as it was.  A change that means to
move a plan regenerates the fixture (plan_sweep.py --write) and says so."""
import json
import os

import pytest

import fattn
import plan_sweep

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_digests.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_small_and_complete(golden):
    assert os.path.getsize(GOLDEN) < 128 * 1024
    want = {name for name, _ in plan_sweep.settings()}
    assert set(golden["digests"]) == want
    groups = {plan_sweep.group_name(D, kt, vt) for D in plan_sweep.HEAD_DIMS for kt, vt in plan_sweep.TYPE_PAIRS}
    every = set(plan_sweep.groups())  # ... and the one-type pairs and the MLA groups
    assert groups < every
    assert all(set(g) == every for g in golden["digests"].values())


def test_every_option_in_the_sweep():
    """Each option fattn exposes is swept at one value or more."""
    swept = {opt for _, opts in plan_sweep.settings() for opt in opts}
    assert swept == set(fattn.OPTION_DEFAULTS)


def test_plans_match_golden(golden):
    G = plan_sweep.groups()
    assert len(next(iter(G.values()))) == golden["cases_per_group"]
    assert {g: len(c) for g, c in G.items() if len(c) != golden["cases_per_group"]} == golden["cases_of_group"]
    bad = []
    for name, opts in plan_sweep.settings():
        with fattn.options(opts):
            for g, cases in G.items():
                if plan_sweep.digest(cases) != golden["digests"][name][g]:
                    bad.append((name, g))
    hint = ""
    if bad:
        name, g = bad[0]
        hint = (f"; for the text, run `python tests/plan_sweep.py --dump new.txt --setting '{name}' --group {g}` "
                "with this build and with the last good one (FATTN_LIB=<its libfattn.so>), then diff the two files")
    assert not bad, f"{len(bad)} (setting, group) digests differ, first: {bad[:8]}{hint}"


def test_row_workspace_sizes_match_golden(golden):
    assert plan_sweep.row_workspace_sizes() == golden["row_workspace"]
