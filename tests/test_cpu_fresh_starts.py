"""CPU: the fresh-start reference on its own (tests/fresh_start_ref.py), the conditions every GPU case must meet in the oracle run
alone, and the C-ABI checks of the start_* fields, which need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import fresh_start_cases as fc
import fresh_start_ref as fref
from oracle import philox
from oracle import rollout as oro


def _run_ref(name, queue, qstate, L=None, launches=fc.LAUNCHES):
    c = fc.build(name)
    S = c["S"]
    st = oro.EnvState(c["obs0"], c["first"], c["steps0"], c["done0"])
    draws, rows = fref.Draws(), []
    for k in range(launches):
        st, r, draws = fref.rollout(c["osystem"], c["ppar"], c["pdims"], st, S, c["L"] if L is None else L, queue=queue, qstate=qstate,
                                    seed=fc.SEED, offset=fc.OFFSETS[k], policy_noise=fc._slice(c["pnoise"], k, S),
                                    model_noise=fc._slice(c["mnoise"], k, S), member_idx=fc._slice(c["midx"], k, S), draws=draws, launch=k)
        rows.append(r)
    return st, torch.cat(rows), draws


def test_stream_id_is_the_next_free_one():
    ids = [v for k, v in vars(philox).items() if k.startswith("STREAM_")]
    assert fref.STREAM_START == max(ids) + 1 == 11


def test_single_row_range_equals_oracle_rollout_from_that_row():
    """A sampled range of one row: every draw is that row, so from the first reset on first_obs is that row — the reference equals
    plain oracle.rollout started with first_obs = [the case's own first_obs until an env's first reset, that row after it].  Checked
    as: the rows of an env up to and including its first reset equal plain oracle.rollout with the case's first_obs, and all rows of
    a run whose initial first_obs already IS that row equal plain oracle.rollout outright."""
    name = "ens_ts1_noise"
    c = fc.build(name)
    q, qs = fc.oracle_buffer(name)
    qs = dict(qs, sample_position=np.int32(int(qs["insert_position"]) - 1))
    the_row = torch.from_numpy(q.gather(qs, np.array([int(qs["sample_position"])]))[0, :c["X"]].copy())
    S, N = c["S"], c["N"]
    st, rows, draws = _run_ref(name, q, qs)
    assert len(draws) > 0 and set(draws.idx) == {int(qs["sample_position"])}
    assert torch.equal(st.first_obs[torch.tensor(sorted(set(draws.env)))], the_row.expand(len(set(draws.env)), -1))
    # plain oracle.rollout over both launches at once, first_obs = that row from the start
    T = fc.LAUNCHES * S
    plain_st, plain_rows = oro.rollout(c["osystem"], c["ppar"], c["pdims"],
                                       oro.EnvState(c["obs0"], the_row.expand(N, -1).clone(), c["steps0"], c["done0"]), T, c["L"],
                                       policy_noise=c["pnoise"], model_noise=c["mnoise"], member_idx=c["midx"])
    D = rows.shape[1]
    got, want = rows.reshape(T, N, D), plain_rows.reshape(T, N, D)
    disc = c["X"] + c["U"] + 1
    for env in range(N):
        resets = np.nonzero(got[:, env, disc].numpy() == 0)[0]
        first_reset = int(resets[0])
        # after the first reset (which went to the case's own first_obs) the env has left plain's trajectory; from its SECOND reset
        # on it is back on it, bit for bit: the reset state is that row in both and the later randomness is the same
        if len(resets) >= 2:
            s2 = int(resets[1])
            assert torch.equal(got[s2 + 1:, env], want[s2 + 1:, env])
            assert torch.equal(got[s2, env, disc + 1:disc + 1 + c["X"]], the_row)
        assert torch.equal(got[first_reset, env, disc + 1:disc + 1 + c["X"]], c["first"][env])
    # and with the initial first_obs already that row: everything equal
    c2 = dict(c, first=the_row.expand(N, -1).clone())
    st = oro.EnvState(c2["obs0"], c2["first"], c2["steps0"], c2["done0"])
    out = []
    for k in range(fc.LAUNCHES):
        st, r, _ = fref.rollout(c["osystem"], c["ppar"], c["pdims"], st, S, c["L"], queue=q, qstate=qs, seed=fc.SEED, offset=fc.OFFSETS[k],
                                policy_noise=fc._slice(c["pnoise"], k, S), model_noise=fc._slice(c["mnoise"], k, S),
                                member_idx=fc._slice(c["midx"], k, S))
        out.append(r)
    assert torch.equal(torch.cat(out), plain_rows)
    assert torch.equal(st.obs, plain_st.obs) and torch.equal(st.steps, plain_st.steps) and torch.equal(st.done, plain_st.done)


def test_no_reset_no_draw():
    """episode_length beyond the unroll, no termination: plain oracle.rollout, nothing drawn, first_obs untouched."""
    name = "ens_ts1_noise"
    c = fc.build(name)
    q, qs = fc.oracle_buffer(name)
    st, rows, draws = _run_ref(name, q, qs, L=1000)
    assert len(draws) == 0 and torch.equal(st.first_obs, c["first"])
    T = fc.LAUNCHES * c["S"]
    plain_st, plain_rows = oro.rollout(c["osystem"], c["ppar"], c["pdims"], oro.EnvState(c["obs0"], c["first"], c["steps0"], c["done0"]),
                                       T, 1000, policy_noise=c["pnoise"], model_noise=c["mnoise"], member_idx=c["midx"])
    assert torch.equal(rows, plain_rows) and torch.equal(st.obs, plain_st.obs) and torch.equal(st.steps, plain_st.steps)


def test_buffer_is_wrapped_with_a_positive_sample_position():
    q, qs = fc.oracle_buffer("pendulum")
    assert int(qs["insert_position"]) == fc.BUF_MAX == 37 and int(qs["sample_position"]) == 5 and sum(fc.BUF_INSERTS) == 50
    # the logical array holds the LAST 37 of the 50 rows in order: the queue rolled
    assert np.array_equal(qs["data"], fc.buffer_rows("pendulum").numpy()[13:])


@pytest.mark.parametrize("name", list(fc.CASES))
def test_gpu_cases_meet_their_conditions(name):
    """On the oracle run alone: every env resets at least twice, some env resets on two steps its tile neighbour does not, the draws
    use more than one row and stay inside [sample_position, insert_position); the termination case stays within termination_ref's
    caps (asserted inside fc.oracle: at most 10 % of the envs near a bound, at least 10 % terminating, a truncation)."""
    ref = fc.oracle(name)
    c = fc.build(name)
    d = ref["draws"]
    N = c["N"]
    per_env = [d.of_env(e) for e in range(N)]
    assert min(len(p) for p in per_env) >= 2
    sp, ip = int(ref["qstate"]["sample_position"]), int(ref["qstate"]["insert_position"])
    assert all(sp <= i < ip for i in d.idx) and len(set(d.idx)) > 8
    differ = 0
    for e in range(0, N - 1):
        if e // 16 != (e + 1) // 16:
            continue
        a, b = set(d.steps_of_env(e, 0)), set(d.steps_of_env(e + 1, 0))
        differ += len(a - b) >= 2
    assert differ >= 1
    if name == "termination":
        keep = ref["keep"]
        assert int((~keep).sum()) <= 0.1 * N
        rows = torch.cat(ref["rows"])
        disc = c["X"] + c["U"] + 1
        assert int(((rows[:, disc] == 0) & (rows[:, -1] == 0)).sum()) >= 0.1 * N      # terminations that are not truncations
    # both launches draw (the written-back first_obs is consumed in the second)
    assert set(d.launch) == {0, 1}


def test_chain_of_starts_is_the_recorded_draws():
    """fresh_start_ref.chain_of_starts (the bookkeeping rule alone, used for the trainers) reproduces the draws the full reference
    recorded for a case that ends episodes by truncation only."""
    name = "pendulum"
    ref, c = fc.oracle(name), fc.build(name)
    steps0 = np.where(c["done0"].numpy() != 0, 0.0, c["steps0"].numpy())      # (AutoReset zeroes the steps of an env that enters done)
    chain = fref.chain_of_starts(c["N"], [c["S"]] * fc.LAUNCHES, c["L"], [(fc.SEED, o) for o in fc.OFFSETS],
                                 int(ref["qstate"]["sample_position"]), int(ref["qstate"]["insert_position"]), steps0=steps0)
    assert chain == [ref["draws"].of_env(e) for e in range(c["N"])]


# ------------------------------------------------------------------------------------------------ C-ABI, no device
def _rollout_desc():
    from mbpo import _hip
    d = _hip.RolloutDesc()
    d.x_dim, d.u_dim, d.n_envs, d.n_steps, d.episode_length, d.action_repeat = 3, 1, 0, 0, 5, 1      # (empty: nothing to launch)
    d.system_kind, d.reward_kind, d.row_len = _hip.SYS_PENDULUM, _hip.REWARD_PENDULUM, 2 * 3 + 1 + 3
    d.reward_params = d.sys_params = d.actions = 64          # (never dereferenced: n_envs = 0)
    return d


def _episode_desc():
    from mbpo import _hip
    d = _hip.EpisodeStepDesc()
    d.x_dim, d.u_dim, d.n_envs, d.episode_length, d.action_repeat, d.step_index, d.n_steps = 3, 1, 0, 5, 1, 0, 1
    d.row_len = 2 * 3 + 1 + 3
    return d


@pytest.mark.parametrize("make,entry", [(_rollout_desc, "mbpo_model_rollout"), (_episode_desc, "mbpo_episode_step")])
def test_start_buffer_argument_checks_need_no_device(make, entry):
    """All four start_* zero is off; a well-formed set is accepted; rows without state, state without rows, start_row_len < x_dim and
    start_max_size outside (0, 2^31 - 1) are MBPO_ERR_ARG — with n_envs = 0, i.e. before any device use."""
    from mbpo import _hip
    lib = _hip.load()
    fn = getattr(lib, entry)
    assert fn(C.byref(make()), None) == 0, lib.mbpo_last_error()

    def call(rows, max_size, row_len, state):
        d = make()
        d.start_rows, d.start_max_size, d.start_row_len, d.start_state = rows, max_size, row_len, state
        return fn(C.byref(d), None)

    assert call(64, 37, 8, 128) == 0, lib.mbpo_last_error()
    assert call(64, 37, 3, 128) == 0                     # row_len == x_dim
    assert call(64, 2 ** 31 - 2, 8, 128) == 0
    for bad in ((64, 37, 8, None), (None, 37, 8, 128), (None, 37, 8, None), (None, 0, 8, None), (64, 37, 2, 128), (64, 0, 8, 128),
                (64, -1, 8, 128), (64, 2 ** 31 - 1, 8, 128), (64, 2 ** 40, 8, 128)):
        assert call(*bad) == -1, f"{entry}{bad} was accepted"
        assert b"start_" in lib.mbpo_last_error()


def test_descriptor_mirrors_match_the_header(tmp_path):
    """The new fields sit where gcc puts them."""
    import subprocess
    from pathlib import Path
    from mbpo import _hip
    root = Path(__file__).resolve().parent.parent
    fields = ["start_rows", "start_max_size", "start_row_len", "start_state"]
    ep = fields + ["seed", "offset", "rng_dev"]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mbpo_hip.h"\nint main(void) {\n' +
                   "".join(f'  printf("%zu\\n", offsetof(mbpo_rollout_desc, {f}));\n' for f in fields) +
                   "".join(f'  printf("%zu\\n", offsetof(mbpo_episode_step_desc, {f}));\n' for f in ep) +
                   '  printf("%zu %zu\\n", sizeof(mbpo_rollout_desc), sizeof(mbpo_episode_step_desc));\n  return 0;\n}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    want = [getattr(_hip.RolloutDesc, f).offset for f in fields] + [getattr(_hip.EpisodeStepDesc, f).offset for f in ep] + \
           [C.sizeof(_hip.RolloutDesc), C.sizeof(_hip.EpisodeStepDesc)]
    assert out == want
