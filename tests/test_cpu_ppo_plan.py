"""mbpo_ppo_workspace_floats, its statuses and its error texts over a sweep of descriptors (tests/ppo_plan_cases.py) against
tests/golden/ppo_workspace_floats.json, which was recorded from the library before the PPO host was rewritten around ppo_plan /
ppo_variant: the sizes, and with them the workspace layout the GPU tests poison and guard, did not move.  The golden file holds one
SHA-256 per (x, u, hidden) block of 80 descriptors, so equality of the digests is equality of every count, status and text.  No GPU:
the library counts 256 compute units without a device, the MI355X's count."""
import json

import pytest

import ppo_plan_cases as cases


@pytest.fixture(scope="module")
def observed():
    from mbpo import _hip
    return json.loads(json.dumps(cases.observe(_hip.load())))


@pytest.fixture(scope="module")
def golden():
    return json.loads(cases.GOLDEN.read_text())


def test_the_sweep_is_the_recorded_one(observed, golden):
    assert observed["axes"] == golden["axes"]
    assert golden["descriptors"] == observed["descriptors"] == 5 * 3 * 5 * 5 * 4 * 2 * 2
    assert len(golden["blocks"]) == 5 * 3 * 5


def test_workspace_floats_and_refusals_match_the_record(observed, golden):
    moved = {k: (observed["blocks"].get(k), v) for k, v in golden["blocks"].items() if observed["blocks"].get(k) != v}
    assert not moved, f"{len(moved)} of {len(golden['blocks'])} blocks moved (now, recorded): {dict(list(moved.items())[:3])}"
    assert observed["refusals"] == golden["refusals"]
    assert all(b["min"] > 0 for b in golden["blocks"].values())          # the whole sweep is accepted: the record is of sizes


def test_bad_descriptors_match_the_record(observed, golden):
    assert observed["bad"] == golden["bad"]
    status, text = golden["bad"]["value_net_two_outputs"]
    assert status < 0 and "value net" in text
    assert golden["bad"]["unequal_hidden_is_layered"][0] > 0          # not an error: the layered path
