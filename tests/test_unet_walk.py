"""The dry walk of the UNet executor against its recorded table: tools/unet_walk_sweep.py generates some 3200 cases (configurations x
options x shapes, inputs only), tests/golden/unet_walk.json holds what the executor answered for each of them - the arena's byte count
(icd_unet_workspace_bytes_ex), icd_unet_kv_cache_bytes, the number of attention layers - and, per handle, icd_unet_finalize's return code and
message with nothing bound (how many tensor lookups the walk makes, and the first).  Written once from runtime.hip as it stood BEFORE it was
taken apart into descriptor constructors and one function per block.  No GPU: a dry walk enqueues nothing and dereferences nothing.

Every row must be equal; there are no coded exceptions.
"""
import importlib.util
import json
import os

import pytest

from conftest import ROOT
from invertible_cd_amd import _lib

_spec = importlib.util.spec_from_file_location("unet_walk_sweep", os.path.join(ROOT, "tools", "unet_walk_sweep.py"))
sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sweep)


@pytest.fixture(scope="module")
def replay():
    with open(sweep.GOLDEN) as f:
        golden = json.load(f)
    got, names = sweep.record(_lib.load())
    return golden, got, names


def test_the_sweep_reaches_every_branch_it_claims():
    cs = sweep.cases()
    assert len(cs) == len({c[0] for c in cs}) and 2000 <= len(cs) <= 6000
    sweep.check_coverage(cs)


def test_the_golden_file_matches_the_sweep(replay):
    golden, _, names = replay
    assert golden["fields"] == list(sweep.FIELDS)
    assert len(golden["rows"]) == len(names)
    assert set(golden["finalize"]) == {n.rsplit(" | ", 1)[0] for n in names}
    assert all(r[0] > 4096 and r[1] > 0 and r[2] > 0 for r in golden["rows"])
    # an empty handle: ICD_ERR_MISSING_TENSOR, the count of lookups and the first of them
    assert all(rc == -4 and " tensors not bound, first: " in msg for rc, msg in golden["finalize"].values())


def test_every_dry_walk_returns_the_recorded_bytes(replay):
    golden, got, names = replay
    wrong = [(n, want, have) for n, want, have in zip(names, golden["rows"], got["rows"]) if want != have]
    assert not wrong, f"{len(wrong)} of {len(names)} walks differ, the first: {wrong[:5]}"


def test_finalize_asks_for_the_recorded_tensors(replay):
    golden, got, _ = replay
    wrong = [(k, want, got["finalize"].get(k)) for k, want in golden["finalize"].items() if got["finalize"].get(k) != want]
    assert not wrong, f"{len(wrong)} of {len(golden['finalize'])} handles differ, the first: {wrong[:5]}"
