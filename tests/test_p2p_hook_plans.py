"""The hook adapter's layer-call plans against their recorded table: tests/golden/make_p2p_hook_plans.py walks the shipped controllers and
ControllerBatches of them (1, 2, 3 groups of two prompts, 2 groups of three, plain stores, members whose self-replace windows disagree)
through two steps of SD1.5's layer kinds on every batch layout the executor runs and on the ones that must not be fused;
tests/golden/p2p_hook_plans.json holds, per layer call, whether needs_probs short-cut it, the counters afterwards and the fields of the
probability kernel's epilogue struct that HookAdapter.plan filled in.  Written once from the adapter as it stood BEFORE its two planning
branches (one controller / a batch of them) became one prompt-group path.  No GPU and no built library.

Every row must be equal; there are no coded exceptions.
"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_p2p_hook_plans", os.path.join(GOLDEN, "make_p2p_hook_plans.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def replay():
    with open(rec.GOLDEN) as f:
        golden = json.load(f)
    return golden, rec.record()


def test_the_golden_file_matches_the_walk(replay):
    golden, _ = replay
    assert golden["fields"] == list(rec.FIELDS) and golden["step_fields"] == list(rec.STEP_FIELDS)
    assert golden["walk"] == [list(w) for w in rec.WALK]
    names = [c[0] for c in rec.cases()]
    assert list(golden["cases"]) == names and len(names) == len(set(names)) == 9 * 6
    assert all(len(c["rows"]) == rec.STEPS * len(rec.WALK) and len(c["steps"]) == rec.STEPS for c in golden["cases"].values())
    rows = [r for c in golden["cases"].values() for r in c["rows"]]
    col = {f: [r[i] for r in rows] for i, f in enumerate(rec.FIELDS)}
    # the walk reaches what it claims: short-cut and materialised layers, planned and refused calls, 1 / 2 / 3 groups, one and two edits
    # per group, self rows from the base prompt, both batch halves as the first conditional row
    assert set(col["tick"]) == set(col["planned"]) == set(col["self_from_base"]) == set(col["edit_At"]) == {0, 1}
    assert set(col["groups"]) == {0, 1, 2, 3} and set(col["edit_count"]) == {0, 1, 2} and len(set(col["first_cond_row"])) > 2
    assert all(row[0] == 1 and row[-2:] == [1, 1] for edges in golden["cross_edges"] for row in edges[:4])
    assert all(row[0] == 0 for edges in golden["cross_edges"] for row in edges[4:])


def test_every_layer_call_is_planned_as_recorded(replay):
    golden, got = replay
    wrong = [(name, i, want, have) for name, c in golden["cases"].items()
             for i, (want, have) in enumerate(zip(c["rows"], got["cases"][name]["rows"])) if want != have]
    assert not wrong, f"{len(wrong)} layer calls differ, the first: {wrong[:5]}"
    assert got["cross_edges"] == golden["cross_edges"]


def test_the_counters_stand_where_they_stood(replay):
    golden, got = replay
    wrong = [(name, c["steps"], got["cases"][name]["steps"]) for name, c in golden["cases"].items() if c["steps"] != got["cases"][name]["steps"]]
    assert not wrong, wrong[:5]
