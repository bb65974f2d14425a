"""The planner of icd_gemm against its recorded table: tools/gemm_plan_sweep.py generates some 5600 descriptors (inputs only, dummy host
pointers), tests/golden/gemm_plans.json holds what the planner answered for each of them - the return code and the eight fields of
icd_gemm_plan_info - and icd_gemm_workspace_bytes of every distinct shape, written once from gemm_run as it stood BEFORE it was taken
apart into gemm_validate / gemm_plan / gemm_args / gemm_launch.  No GPU: icd_gemm_plan enqueues nothing and dereferences nothing.

Rows that differ from the recording on purpose (the golden rows are left as generated):
  * "conv C0 = 0 on a big tile" - a conv whose first source has no channels (C0 = 0, all 64 channels in a1) used to pass when the launch
    took a big tile and was refused ("conv channels must be multiples of 8") on the 128-wide route; the conv checks are written once now,
    in front of the tile choice, so it is refused on every route.  (The same hoisted check also refuses a NEGATIVE C1 whose sum with C0 is
    a multiple of 64 on a big tile, which the old code let through; that nonsensical descriptor is not in the sweep.)
  * "ln separate pass, lda != K" - ICD_GEMM_LN_COMPUTE on a route that runs the icd_layernorm_stats launch needs contiguous rows (icd_amd.h);
    icd_gemm refused that, icd_gemm_plan did not look.  The check is part of the plan now, so both entries refuse it.
"""
import ctypes as C
import importlib.util
import json
import os

import pytest

from conftest import ROOT
from invertible_cd_amd import _lib
from test_gemm_edges import REFUSALS

_spec = importlib.util.spec_from_file_location("gemm_plan_sweep", os.path.join(ROOT, "tools", "gemm_plan_sweep.py"))
sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sweep)

# name -> message fragment of the refusal that replaces the recorded plan
NOW_REFUSED = {"conv C0 = 0 on a big tile": "conv channels must be multiples of 8",
               "ln separate pass, lda != K": "needs contiguous rows (lda == K)"}


@pytest.fixture(scope="module")
def replay():
    with open(sweep.GOLDEN) as f:
        golden = json.load(f)
    got, names, msgs = sweep.record(_lib.load())
    return golden, got, names, msgs


def test_the_golden_file_covers_every_plan_field(replay):
    golden, _, names, _ = replay
    assert golden["fields"] == ["rc"] + list(sweep.FIELDS)
    assert len(golden["plans"]) == len(names) == len(set(names)) and len(names) >= 5000
    sweep.check_coverage(golden["plans"])


def test_every_descriptor_gets_the_recorded_plan(replay):
    golden, got, names, msgs = replay
    wrong = []
    for name, want, have, msg in zip(names, golden["plans"], got["plans"], msgs):
        if name in NOW_REFUSED:
            assert want[0] == 0 and have[0] == -1 and NOW_REFUSED[name] in msg, (name, want, have, msg)
        elif want != have:
            wrong.append((name, want, have, msg))
    assert not wrong, f"{len(wrong)} plans differ, the first: {wrong[:5]}"
    assert sum(n in NOW_REFUSED for n in names) == len(NOW_REFUSED)


def test_workspace_bytes_are_the_recorded_ones_and_cover_the_split_taken(replay):
    golden, got, names, _ = replay
    assert got["workspace"] == golden["workspace"]
    # the workspace the executor sizes from icd_gemm_workspace_bytes admits every split the planner would take with unlimited bytes
    by_name = dict(zip(names, got["plans"]))
    pairs = [(n, by_name[n[:-len("ws")] + "ample"]) for n in names if n.endswith(" ws")]
    assert len(pairs) > 500
    for n, ample in pairs:
        assert by_name[n] == ample, (n, by_name[n], ample)


def test_refusal_rows_carry_their_message(replay):
    _, got, names, msgs = replay
    by_name = {n: (p, m) for n, p, m in zip(names, got["plans"], msgs)}
    for name, _, fragment in REFUSALS:
        plan, msg = by_name[f"refusal: {name}"]
        assert plan[0] == -1 and plan[1:] == [0] * 8 and fragment in msg, (name, plan, msg)
        assert by_name[f"refusal + FORCE_BIG: {name}"][0][0] == -1, name
    for (plan, msg), name in ((by_name[n], n) for n in names):
        assert (plan[0] != 0) == bool(msg) and plan[0] in (0, -1), name


def test_the_plan_entry_answers_on_the_stack_without_side_effects():
    """icd_gemm_plan writes all eight fields (nothing is left from the caller's struct) and leaves the descriptor alone."""
    lib = _lib.load()
    d = sweep.dense_desc(8192, 1280, 1280)
    before = bytes(d)
    info = _lib.GemmPlanInfo(*([-7] * 8))
    assert lib.icd_gemm_plan(C.byref(d), C.byref(info)) == 0
    assert bytes(d) == before
    assert all(getattr(info, f) != -7 for f in sweep.FIELDS) and info.cfg in range(7) and info.group_m == 1
