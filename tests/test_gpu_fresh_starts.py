"""GPU: branched model rollouts — a fresh true-buffer start state after every reset (include/mbpo_hip.h, "fresh starts") — against
tests/fresh_start_ref.py on the cases of tests/fresh_start_cases.py (N = 40 envs, S = 5 steps, episode_length 2, a wrapped 37-row true
buffer, two consecutive launches), every kernel mbpo_model_rollout dispatches to, mbpo_episode_step, and the SAC / PPO trainers.

Tolerances: rows and the carried obs at the rollout's stated atol = rtol = 2e-4 (5e-4 at x = 17), as tests/test_gpu_rollout.py;
first_obs, discount, truncation, steps, done and every start state are exact.
"""
import numpy as np
import pytest
import torch

import fresh_start_cases as fc
import fresh_start_ref as fref
from oracle import philox

pytestmark = pytest.mark.gpu


def _launches(name, dev, mode=-1, start=True, L=None):
    """Both launches of case `name` on the device; returns per launch (rows, obs, first_obs, steps, done) on the host."""
    from mbpo import _hip
    lib = _hip.load()
    out, env = [], None
    buf = fc.device_buffer(name, dev) if start else None
    lib.mbpo_debug_set_rollout_lean(mode)
    try:
        from mbpo import ops
        for k in range(fc.LAUNCHES):
            kw = fc.device_kwargs(name, dev, k, env=env, start=buf)
            if L is not None:
                kw["episode_length"] = L
            rows = ops.model_rollout(**kw)
            env = (kw["obs"], kw["first_obs"], kw["steps"], kw["done"])
            out.append(tuple(t.cpu().clone() for t in (rows, *env)))
    finally:
        lib.mbpo_debug_set_rollout_lean(-1)
    if buf is not None:      # the true buffer is only read
        ref_data, ref_state = fc.device_buffer(name, dev)
        assert torch.equal(buf[0], ref_data) and torch.equal(buf[1], ref_state)
    return out


@pytest.mark.parametrize("name", list(fc.CASES))
def test_rollout_matches_reference(dev, name):
    ref, c = fc.oracle(name), fc.build(name)
    N, S, X, U = c["N"], c["S"], c["X"], c["U"]
    keep = ref["keep"]
    got = _launches(name, dev)
    disc, nxt = X + U + 1, X + U + 2
    q, qs = ref["queue"], ref["qstate"]
    chains = [[c["first"][e].numpy()] + [q.gather(qs, np.array([i]))[0, :X] for i in ref["draws"].of_env(e)] for e in range(N)]
    used = [0] * N
    for k, ((rows, obs, first, steps, done), rows_ref, st_ref) in enumerate(zip(got, ref["rows"], ref["states"])):
        r, rr = rows.reshape(S, N, -1)[:, keep], rows_ref.reshape(S, N, -1)[:, keep]
        print(f"{name} launch {k}: max |rows - ref| = {float((r - rr).abs().max()):.3e}, kept envs {int(keep.sum())} of {N}")
        torch.testing.assert_close(r, rr, atol=c["atol"], rtol=c["atol"])
        torch.testing.assert_close(obs[keep], st_ref.obs[keep], atol=c["atol"], rtol=c["atol"])
        assert torch.equal(r[..., disc], rr[..., disc]) and torch.equal(r[..., -1], rr[..., -1])          # discount, truncation
        assert torch.equal(steps[keep], st_ref.steps[keep]) and torch.equal(done[keep], st_ref.done[keep])
        assert torch.equal(first[keep], st_ref.first_obs[keep])                                              # written back, exact
        # every next_observation of a done row is the start state the reference's chain holds for that reset, bit for bit
        full = rows.reshape(S, N, -1)
        for e in np.nonzero(keep.numpy())[0]:
            for s in np.nonzero(full[:, e, disc].numpy() == 0)[0]:
                assert np.array_equal(full[s, e, nxt:nxt + X].numpy(), chains[e][used[e]]), (name, k, int(s), int(e))
                used[e] += 1
    for e in np.nonzero(keep.numpy())[0]:
        assert used[e] == len(chains[e]) - 1 >= 2      # every drawn start but the last was consumed by a reset; at least two resets


@pytest.mark.parametrize("name", fc.LEAN)
def test_lean_equals_generic_with_a_start_buffer(dev, name):
    """k_rollout_lean with one tile (mode 3) and two tiles in flight (mode 2; the Pendulum system has no member phase and stays on one)
    against the generic 64-wide kernel (mode 0): rows, obs, first_obs, steps and done bit for bit."""
    base = _launches(name, dev, mode=0)
    for mode in (3, 2):
        got = _launches(name, dev, mode=mode)
        for k, (a, b) in enumerate(zip(got, base)):
            for what, x, y in zip(("rows", "obs", "first_obs", "steps", "done"), a, b):
                assert torch.equal(x, y), f"{name}: mode {mode} launch {k} differs from the generic kernel in {what}"


@pytest.mark.parametrize("name", ["ens_ts1_noise", "pendulum", "wide128_x17", "openloop_pendulum"])
def test_a_start_buffer_without_resets_changes_nothing(dev, name):
    """episode_length beyond the unroll and no termination: every output and first_obs is bit-identical to the launch without a start
    buffer (modes 0, 3 and 2 where the lean kernel applies)."""
    c = fc.build(name)
    for mode in ((0, 3, 2) if name in fc.LEAN else (-1, 0)):
        with_buf = _launches(name, dev, mode=mode, L=1000)
        without = _launches(name, dev, mode=mode, start=False, L=1000)
        for a, b in zip(with_buf, without):
            for x, y in zip(a, b):
                assert torch.equal(x, y), f"{name}: mode {mode}"
            assert torch.equal(a[2], c["first"])


def test_without_a_start_buffer_first_obs_is_left_alone(dev):
    """No start buffer: the resets go back to the same first_obs, which the launch does not write (the behaviour before)."""
    name = "ens_ts1_noise"
    c = fc.build(name)
    for mode in (0, 3, 2):
        for rows, obs, first, steps, done in _launches(name, dev, mode=mode, start=False):
            assert torch.equal(first, c["first"])
            r = rows.reshape(c["S"], c["N"], -1)
            dn = r[..., c["X"] + c["U"] + 1] == 0
            assert bool(dn.any()) and torch.equal(r[..., c["X"] + c["U"] + 2:2 * c["X"] + c["U"] + 2][dn], c["first"].expand(c["S"], -1, -1)[dn])


def test_per_step_path_draws_what_the_fused_launch_draws(dev):
    """A user-defined torch System restating the Pendulum, stepped through mbpo_policy_act -> step -> mbpo_episode_step, against the
    fused Pendulum launch under the same key: the same first_obs chain and done flags, exactly."""
    from mbpo import ops
    from test_gpu_generic_system import _user_pendulum
    name = "pendulum"
    c = fc.build(name)
    user = _user_pendulum()()
    sp = user.init_params(0)
    fused = _launches(name, dev)
    buf = fc.device_buffer(name, dev)
    env = None
    for k in range(fc.LAUNCHES):
        kw = fc.device_kwargs(name, dev, k, env=env, start=buf)
        for drop in ("system_kind", "sys_params", "reward_kind", "reward_params", "model_noise", "member_idx"):
            kw.pop(drop)
        rows = ops.model_rollout(**kw, **user.rollout_spec(sp, dev))
        env = (kw["obs"], kw["first_obs"], kw["steps"], kw["done"])
        f_rows, f_obs, f_first, f_steps, f_done = fused[k]
        assert torch.equal(env[1].cpu(), f_first) and torch.equal(env[3].cpu(), f_done) and torch.equal(env[2].cpu(), f_steps)
        disc = c["X"] + c["U"] + 1
        assert torch.equal(rows.cpu()[:, disc], f_rows[:, disc])
        # a done row's next_observation is a start state: a bit copy in both paths
        dn = f_rows[:, disc] == 0
        assert torch.equal(rows.cpu()[dn][:, disc + 1:disc + 1 + c["X"]], f_rows[dn][:, disc + 1:disc + 1 + c["X"]])
        torch.testing.assert_close(rows.cpu(), f_rows, atol=2e-4, rtol=2e-4)
    assert user.calls == fc.LAUNCHES * c["S"]


def test_ops_argument_checks(dev):
    from mbpo import ops
    name = "pendulum"
    data, state = fc.device_buffer(name, dev)
    kw = fc.device_kwargs(name, dev, 0, start=None)
    with pytest.raises(ValueError, match="both"):
        ops.model_rollout(**kw, start_rows=data)
    with pytest.raises(ValueError, match="row_len"):
        ops.model_rollout(**kw, start_rows=data[:, :2].contiguous(), start_state=state)
    with pytest.raises(Exception, match="start_state"):
        ops.model_rollout(**kw, start_rows=data, start_state=state.to(torch.int64))


# ------------------------------------------------------------------------------------------------ trainers
X, U, E = 4, 1, 5
TRUE_ROWS = 500
SAC_KW = dict(num_envs=32, batch_size=64, grad_updates_per_step=2, num_env_steps_between_updates=3, episode_length=2,
              normalize_observations=True, max_replay_size=4000, min_replay_size=32, discounting=0.95, lr_policy=3e-4, lr_q=3e-4,
              lr_alpha=3e-4)
N_STEPS = 6
PPO_KW = dict(num_envs=32, unroll_length=8, batch_size=8, num_minibatches=4, num_updates_per_batch=1, episode_length=2,
              normalize_observations=True, discounting=0.97, lr=3e-4, entropy_cost=1e-2, policy_hidden_layer_sizes=(64, 64),
              critic_hidden_layer_sizes=(64, 64))


def _true_rows():
    g = torch.Generator().manual_seed(5)
    return torch.randn(TRUE_ROWS, 2 * X + U + 2, generator=g)


def _env(dev):
    from mbpo.replay import UniformSamplingQueue
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    from mbpo.systems.brax_wrapper import BraxWrapper
    from mbpo.types import Transition
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev)
    system = EnsembleSystem(dyn, QuadraticReward(X, U, target=[0.1, 0, 0, 0], q=[1, 2, 0.5, 0.1], r=[0.3]))
    sp = system.init_params(1)
    sp.dynamics_params.params.mul_(0.5)
    z = torch.zeros
    tb = UniformSamplingQueue(TRUE_ROWS, Transition(z(X), z(U), z(1), z(1), z(X)), 1, device=dev)
    return BraxWrapper(system, sp, tb.insert_rows(tb.init(0), _true_rows().to(dev)), tb)


def _match_true_rows(obs: torch.Tensor) -> np.ndarray:
    """Logical index of the true-buffer row whose observation is bit-equal to each row of obs (-1: none)."""
    table = {r[:X].numpy().tobytes(): i for i, r in enumerate(_true_rows())}
    return np.array([table.get(o.numpy().tobytes(), -1) for o in obs])


def _reset_indices(key, n, offset):
    k0 = philox.split(philox.split(key, n)[0])[0]
    return philox.philox_randint(k0, offset, philox.STREAM_REPLAY, np.arange(n, dtype=np.uint64), 0, TRUE_ROWS)


def _consumed(first_idx, chain):
    """The start rows the resets consumed: the initial first_obs, then every draw but each env's last."""
    return set(first_idx.tolist()) | {i for ch in chain for i in ch[:-1]}


def _sac_run(dev, use_graph, **extra):
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    env = _env(dev)
    N, S = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"]
    tr = SAC(environment=env, num_timesteps=32 + N * S * N_STEPS, use_graph=use_graph, **SAC_KW, **extra)
    assert tr.num_training_steps_per_epoch == N_STEPS and tr.num_prefill_actor_steps == 1
    ts, es, bs = tr.init_training_state(7), tr.reset_envs(env, 11, N), tr.replay_buffer.init(13)
    ts, es, bs, _ = tr.prefill_replay_buffer(ts, es, bs, 17)
    ts, es, bs, _ = tr.training_epoch(ts, es, bs, 19)
    torch.cuda.synchronize()
    assert (tr._graph is not None) == use_graph
    n_rows = bs.insert_position
    out = dict(params=tr.updater.params.cpu().clone(), data=bs.data.cpu().clone()[:n_rows], first=es.info["first_obs"].cpu().clone(),
               obs=es.obs.cpu().clone(), true_state=env.sample_buffer_state.state.cpu().tolist())
    tr.close()
    return out


def test_sac_resample_starts_graph_equals_eager_and_starts_are_true_rows(dev):
    from mbpo.optimizers.policy_optimizers.sac import sac as sac_mod
    from mbpo.utils import keys as K
    eager, graph = _sac_run(dev, False, resample_starts=True), _sac_run(dev, True, resample_starts=True)
    for k in ("params", "data", "first", "obs"):
        assert torch.equal(eager[k], graph[k]), f"graph replay vs eager: differs in {k}"
    N, S, L = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"], SAC_KW["episode_length"]
    data = graph["data"]
    assert data.shape[0] == N * S * (1 + N_STEPS)
    disc = X + U + 1
    starts = data[data[:, disc] == 0][:, disc + 1:disc + 1 + X]          # where the resets went: the next episodes' first observations
    got = _match_true_rows(starts)
    assert (got >= 0).all(), "a model episode starts at a state that is no true-buffer row"
    # the reference: the bookkeeping rule + the START stream, launch by launch (prefill under its own key, then the epoch's steps)
    site = sac_mod.SITE_ROLLOUT << 32
    keys = [(K.PRNGKey(K.split(17)[0]), site)] + [(K.PRNGKey(19), site + t) for t in range(N_STEPS)]
    chain = fref.chain_of_starts(N, [S] * (1 + N_STEPS), L, keys, 0, TRUE_ROWS)
    want = _consumed(_reset_indices(11, N, 1), chain)
    assert set(got.tolist()) == want and len(want) > 32
    print(f"SAC resample_starts: {len(want)} distinct start rows over {starts.shape[0]} resets")
    # the carried first_obs is each env's last draw
    assert np.array_equal(_match_true_rows(graph["first"]), np.array([ch[-1] for ch in chain]))
    assert graph["true_state"][:3] == [TRUE_ROWS, 0, 0]
    # without the option: at most one start per env, the reset's own obs
    plain = _sac_run(dev, True)
    pstarts = plain["data"][plain["data"][:, disc] == 0][:, disc + 1:disc + 1 + X]
    pgot = _match_true_rows(pstarts)
    assert (pgot >= 0).all() and len(set(pgot.tolist())) <= 32
    assert set(pgot.tolist()) == set(_reset_indices(11, N, 0).tolist())
    assert not torch.equal(plain["params"], graph["params"])


def test_ppo_resample_starts_one_unroll_holds_different_starts(dev):
    from mbpo.optimizers.policy_optimizers.ppo import ppo as ppo_mod
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    from mbpo.utils import keys as K
    N, T, L = PPO_KW["num_envs"], PPO_KW["unroll_length"], PPO_KW["episode_length"]
    disc = X + U + 1
    res = {}
    for use_graph in (False, True):
        env = _env(dev)
        tr = PPO(environment=env, num_timesteps=2 * N * T, use_graph=use_graph, resample_starts=True, **PPO_KW)
        assert tr.num_training_steps_per_epoch == 2 and tr.batch_size * tr.num_minibatches // tr.num_envs == 1      # one unroll per step
        ts = tr.init_training_state(5)
        es = env.reset(K.split(11, N), resample_first_obs=True)
        ts, es, _ = tr.training_epoch(ts, es, 19)
        torch.cuda.synchronize()
        assert (tr._graph is not None) == use_graph
        res[use_graph] = dict(data=tr._data.cpu().clone(), first=es.info["first_obs"].cpu().clone(), params=tr.updater.params.cpu().clone())
        tr.close()
    for k in ("data", "first", "params"):
        assert torch.equal(res[False][k], res[True][k]), f"graph replay vs eager: differs in {k}"
    data = res[True]["data"]                                         # the second step's unroll: [N, T, D]
    site = ppo_mod.SITE_UNROLL << 32
    chain = fref.chain_of_starts(N, [T, T], L, [(K.PRNGKey(19), site), (K.PRNGKey(19), site + 1)], 0, TRUE_ROWS)
    per_env = T // L
    for e in range(N):
        rows = data[e]
        starts = rows[rows[:, disc] == 0][:, disc + 1:disc + 1 + X]
        got = _match_true_rows(starts)
        # the second unroll's resets consume the draws of the first unroll's last reset onwards
        assert got.tolist() == chain[e][per_env - 1:2 * per_env - 1], e
    assert len({i for ch in chain for i in ch[per_env - 1:2 * per_env - 1]}) > 32
    assert np.array_equal(_match_true_rows(res[True]["first"]), np.array([ch[-1] for ch in chain]))


def test_run_training_refuses_an_empty_true_buffer(dev):
    from mbpo.optimizers import PPOOptimizer, SACOptimizer
    env = _env(dev)
    opt = SACOptimizer(system=env.system, true_buffer=env.sample_buffer, num_timesteps=32 + 32 * 3 * 2, num_evals=1, num_eval_envs=8,
                       resample_starts=True, **SAC_KW)
    assert opt.dummy_trainer.resample_starts
    with pytest.raises(ValueError, match="true buffer"):
        opt.train(opt.init(key=5))                                   # the dummy (empty) true buffer
    out = opt.train(opt.init(key=5, true_buffer_state=env.sample_buffer_state))
    assert bool(torch.isfinite(out.optimizer_state.policy_params[1]).all())
    popt = PPOOptimizer(system=env.system, true_buffer=env.sample_buffer, num_timesteps=2 * 32 * 8, num_evals=1, num_eval_envs=8,
                        resample_starts=True, **PPO_KW)
    with pytest.raises(ValueError, match="true buffer"):
        popt.train(popt.init(key=5))
    out = popt.train(popt.init(key=5, true_buffer_state=env.sample_buffer_state))
    assert bool(torch.isfinite(out.optimizer_state.policy_params[1]).all())
