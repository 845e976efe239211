"""The scratch-contract case table (tests/scratch_contract_cases.py) against include/mbpo_hip.h, without a GPU: every exported function
with a `workspace` parameter and every descriptor with a `workspace` field has a row in the table or stands in its explicit
out-of-scope list, so a new entry point cannot join the ABI without a contract case; the header states the initial-content
requirement of every workspace; the size queries that need no device return a positive size for every row and never shrink when the
batch or the row count grows at a fixed path."""
import contextlib
import ctypes as C
import re
from pathlib import Path

import pytest

import scratch_contract_cases as scc

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mbpo_hip.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

# rows (dispatch paths) per covered entry point: deleting a row from the table fails here
ROWS = {
    "mbpo_ppo_step": 9, "mbpo_ppo_grads": 6, "mbpo_ppo_apply": 6, "mbpo_bptt_actor_grads": 8, "mbpo_critic_grads": 2, "mbpo_mlp_vjp": 3,
    "mbpo_mlp_layered_vjp": 4, "mbpo_adamw_step": 5, "mbpo_ens_nll_grads": 8, "mbpo_ens_eval": 5, "mbpo_ens_keep_best": 2,
    "mbpo_ens_pick_elites": 2, "mbpo_ens_scaler_fit": 5, "mbpo_running_stats_reduce": 3, "mbpo_running_stats_update": 3,
    "mbpo_policy_act": 2, "mbpo_philox_permutation": 3, "mbpo_icem_update": 6, "mbpo_icem_update_constrained": 2,
    "mbpo_icem_update_batched": 2,
}


def _functions():
    """{name: parameter text} of every function the header declares."""
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mbpo_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", CODE, flags=re.S)}


def _structs_with_workspace():
    out = []
    for m in re.finditer(r"typedef struct (mbpo_[a-z0-9_]+)\s*\{(.*?)\}\s*\1\s*;", CODE, flags=re.S):
        if re.search(r"\*\s*workspace\s*;", m.group(2)):
            out.append(m.group(1))
    return out


def test_every_workspace_of_the_header_has_a_case_or_is_out_of_scope():
    fns, structs = _functions(), _structs_with_workspace()
    assert len(fns) >= 60 and {"mbpo_sac_desc", "mbpo_ppo_desc", "mbpo_bptt_desc", "mbpo_ens_train_desc", "mbpo_ens_eval_desc"} <= set(structs)
    covered = scc.covered_entries()
    assert covered <= set(fns), f"rows for entry points the header does not declare: {sorted(covered - set(fns))}"
    need_case = {n for n, params in fns.items() if re.search(r"\*\s*workspace\b", params)}
    assert len(need_case) >= 13
    for s in structs:
        users = {n for n, params in fns.items() if re.search(rf"\b{s}\s*\*", params) and not n.endswith("_workspace_floats")}
        assert users, s
        if s not in scc.OUT_OF_SCOPE:
            need_case |= users
    missing = sorted(need_case - covered)
    assert not missing, f"entry points with a caller-owned workspace but no row in tests/scratch_contract_cases.py: {missing}"
    # the out-of-scope list names real descriptors, and nothing covered hides behind it
    for s in scc.OUT_OF_SCOPE:
        assert re.search(rf"typedef struct {s}\b", CODE), s
        assert not {n for n, params in fns.items() if re.search(rf"\b{s}\s*\*", params)} & covered


def test_rows_per_entry_point():
    count = {}
    for c in scc.CASES.values():
        for e in c.entries:
            count[e] = count.get(e, 0) + 1
    assert count == ROWS
    ids = set(scc.CASES)
    for a, b in scc.SECOND_HAND:
        assert a in ids and b in ids and a != b
        assert scc.CASES[a].family == scc.CASES[b].family and scc.CASES[a].ws_dtype == scc.CASES[b].ws_dtype is not None
    families = {c.family for c in scc.CASES.values() if c.ws_dtype is not None}
    assert families == {scc.CASES[b].family for _, b in scc.SECOND_HAND}, "every family with a workspace has a second-hand pair"
    assert all(not c.unwritten for c in scc.CASES.values()), "the header names no unwritten `out` element today"


def test_header_states_the_initial_content_of_every_workspace():
    """One sentence per entry point (or per descriptor) in the header: the words `need not be initialised` next to every workspace that
    is scratch, `must be zero` where it is state."""
    # comment blocks that mention a covered entry point's workspace
    for name in sorted(scc.covered_entries() - {"mbpo_ens_pick_elites"}):
        hits = [m.start() for m in re.finditer(rf"\b{name}\b", HEADER)]
        assert hits, name
    assert HEADER.count("need not be initialised") >= 12
    assert "`workspace` must be zero before the first call" in HEADER
    doc = (ROOT / "INTEGRATION.md").read_text()
    assert "## Scratch contract" in doc
    section = doc.split("## Scratch contract", 1)[1].split("\n## ", 1)[0]
    for name in sorted(scc.covered_entries()):
        assert f"`{name}`" in section, f"{name} is missing from INTEGRATION.md's scratch-contract table"


@contextlib.contextmanager
def _knob(case):
    if case.knob is None:
        yield
        return
    from mbpo import _hip
    fn = getattr(_hip.load(), case.knob[0])
    fn.argtypes, fn.restype = [C.c_int], C.c_int
    try:
        assert fn(case.knob[1]) == 0
        yield
    finally:
        assert fn(-1) == 0


@pytest.mark.parametrize("cid", sorted(scc.CASES))
def test_size_queries_positive_and_monotonic(cid):
    case = scc.CASES[cid]
    with _knob(case):
        sizes = [case.need(s) for s in (1, 2, 3, 8)]
    if case.ws_dtype is None:
        assert sizes == [0, 0, 0, 0]
        return
    assert sizes[0] > 0
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), f"{cid}: the workspace shrinks as the batch grows: {sizes}"
