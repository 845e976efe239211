"""GPU: whole SAC / PPO training steps on a TERMINATING EnsembleSystem against the CPU oracle loops given the wrapped oracle system
(tests/termination_ref.py), at tests/test_gpu_trainer_parity.py's smallest configuration and tolerances; and the hipGraph-replayed
epoch against the eagerly issued one, bit for bit.

The margin rule of tests/test_gpu_termination.py, evaluated on the ORACLE loop (the wrapper records every step call of the loop): an
env whose next state ever comes within 2e-3 (10 x the rows' tolerance) of a bound is excluded from the row comparison as a whole; at
most 10 % of the envs may be excluded, at least 10 % must terminate by sys_done and a truncation must occur — asserted on the oracle
loop before any device result is compared.  Replay positions, statistics and parameters are compared in full: they depend on every
row, and a next state 2e-3 from a bound is still 10 tolerances away from a flipped decision.
"""
import math

import numpy as np
import pytest
import torch

from oracle import ppo as oppo, sac as osac, systems as osys, trainer as otr

import termination_ref as tref

pytestmark = pytest.mark.gpu
INF = math.inf
X, U, E = 4, 1, 5
SAC_BOUNDS = {0: (-1.2, 1.2), 3: (-INF, 1.1)}
PPO_BOUNDS = {0: (-1.2, 1.2), 3: (-INF, 1.1)}

SAC_KW = dict(num_envs=64, batch_size=256, grad_updates_per_step=4, num_env_steps_between_updates=5, episode_length=5,
              normalize_observations=True, max_replay_size=1500, min_replay_size=64, discounting=0.95, lr_policy=3e-4,
              lr_q=3e-4, lr_alpha=3e-4, wd_q=1e-4)
PPO_KW = dict(num_envs=32, unroll_length=8, batch_size=16, num_minibatches=4, num_updates_per_batch=2, episode_length=20,
              normalize_observations=True, discounting=0.97, lr=3e-4, wd=1e-5, entropy_cost=1e-2, gae_lambda=0.95,
              clipping_epsilon=0.3, policy_hidden_layer_sizes=(64, 64), critic_hidden_layer_sizes=(64, 64))


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _box(bounds):
    low, high = [-INF] * X, [INF] * X
    for d, (lo, hi) in bounds.items():
        low[d], high[d] = lo, hi
    return low, high


def _true_buffer(dev, rows, seed=0):
    from mbpo.replay import UniformSamplingQueue
    from mbpo.types import Transition
    dummy = Transition(observation=torch.zeros(X), action=torch.zeros(U), reward=torch.zeros(1), discount=torch.zeros(1),
                       next_observation=torch.zeros(X))
    tb = UniformSamplingQueue(rows, dummy, 1, device=dev)
    data = torch.randn(rows, 2 * X + U + 2, generator=torch.Generator().manual_seed(seed))
    return tb, tb.insert_rows(tb.init(0), data.to(dev))


def make_system(dev, bounds):
    """(system with the termination, its params, the wrapped oracle system)"""
    from mbpo.systems import BoxTermination, EnsembleDynamics, EnsembleSystem, QuadraticReward
    low, high = _box(bounds)
    dyn = EnsembleDynamics(X, U, n_members=E, device=dev)
    rew = QuadraticReward(X, U, target=[0.1, 0, 0, 0], q=[1, 2, 0.5, 0.1], r=[0.3])
    system = EnsembleSystem(dyn, rew, termination=BoxTermination(low, high))
    sp = system.init_params(1)
    sp.dynamics_params.params.mul_(0.5)
    rp = sp.reward_params
    osystem = osys.EnsembleSystem(sp.dynamics_params.params.cpu().clone(), dyn.dims, E, X, U,
                                  reward_fn=lambda a, b: osys.quadratic_reward(a, b, torch.tensor(rp.target), torch.tensor(rp.q),
                                                                               torch.tensor(rp.r)))
    return system, sp, tref.TerminatingSystem(osystem, low, high)


def check_oracle_loop(wrapped, truncation):
    """The three conditions on everything the oracle loop stepped (tref.check_oracle_run); returns the kept-env mask [N]."""
    d = torch.stack(wrapped.distances)
    print(f"oracle loop: min distance to a bound {float(d.min()):.4e}, {int(wrapped.near_mask().sum())} envs excluded, "
          f"{int(wrapped.terminated_mask().sum())} of {d.shape[1]} terminate, {int(truncation.sum())} truncations")
    return tref.check_oracle_run(wrapped, truncation)


# ------------------------------------------------------------------------------------------------ SAC
def sac_setup(dev, use_graph, bounds=SAC_BOUNDS, n_steps=2):
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    from mbpo.systems.brax_wrapper import BraxWrapper
    system, sp, wrapped = make_system(dev, bounds)
    tb, tbs = _true_buffer(dev, 512)
    env = BraxWrapper(system, sp, tbs, tb)
    N, S = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"]
    tr = SAC(environment=env, num_timesteps=64 + N * S * n_steps, use_graph=use_graph, **SAC_KW)
    assert tr.num_training_steps_per_epoch == n_steps
    return tr, tr.init_training_state(7), tr.reset_envs(env, 11, N), tr.replay_buffer.init(13), wrapped


def sac_oracle(tr, es, wrapped):
    cfg = osac.SacConfig(X, U, tr.policy_dims, tr.q_dims, discounting=SAC_KW["discounting"], lr_policy=3e-4, lr_q=3e-4,
                         lr_alpha=3e-4, wd_q=1e-4)
    return otr.CpuSacLoop(cfg, wrapped, SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"], SAC_KW["episode_length"],
                          SAC_KW["batch_size"], SAC_KW["grad_updates_per_step"], SAC_KW["max_replay_size"], True,
                          init_params=tr.updater.params.cpu().clone(), init_obs=es.obs.cpu().clone())


def _sac_state(tr, es, bs):
    torch.cuda.synchronize()
    return dict(params=tr.updater.params.cpu().clone(), tq=tr.updater.target_q.cpu().clone(), m=tr.updater.adam_m.cpu().clone(),
                v=tr.updater.adam_v.cpu().clone(), obs=es.obs.cpu().clone(), steps=es.info["steps"].cpu().clone(),
                done=es.done.cpu().clone(), stats=tr._stats_vec.cpu().clone(), rows=tr._rollout_rows.cpu().clone(),
                data=bs.data.cpu().clone(), rng=tr._rng.cpu().clone())


def test_sac_training_step_on_a_terminating_system(dev):
    from mbpo.utils import keys as K
    D = 2 * X + U + 3
    # eager, step by step, against the oracle loop
    tr, ts, es, bs, wrapped = sac_setup(dev, use_graph=False)
    loop = sac_oracle(tr, es, wrapped)
    ts, es, bs, _ = tr.prefill_replay_buffer(ts, es, bs, 17)
    loop.rekey(K.split(17)[0])
    loop.prefill_step()
    prefill_rows = tr._rollout_rows.cpu().clone()
    prefill_ref = loop.last_rows.clone()
    tr.rekey(19)
    loop.rekey(19)
    ts, es, bs = tr.training_step(ts, es, bs)
    loop.training_step()
    torch.cuda.synchronize()
    # (the oracle's own run; nothing of the device's is involved)
    keep = check_oracle_loop(wrapped, torch.cat([prefill_ref[:, D - 1], loop.last_rows[:, D - 1]]))
    kr = keep.repeat(SAC_KW["num_env_steps_between_updates"])       # rows are step-major: env = row % N
    for got, want in ((prefill_rows, prefill_ref), (tr._rollout_rows.cpu(), loop.last_rows)):
        for col in (X + U + 1, D - 1):                                # discount, truncation: exact
            assert torch.equal(got[kr, col], want[kr, col])
        torch.testing.assert_close(got[kr], want[kr], atol=2e-4, rtol=2e-4)
    rows = loop.last_rows[kr]
    assert int(((rows[:, X + U + 1] == 0) & (rows[:, D - 1] == 0)).sum()) >= 1      # terminations that are not truncations
    assert torch.equal(es.info["steps"].cpu()[keep], loop.env.steps[keep]) and torch.equal(es.done.cpu()[keep], loop.env.done[keep])
    torch.testing.assert_close(es.obs.cpu()[keep], loop.env.obs[keep], atol=2e-4, rtol=2e-4)
    st = bs.state.cpu().tolist()
    assert st[0] == int(loop.qstate["insert_position"]) and st[1] == int(loop.qstate["sample_position"])
    ref_batch = torch.from_numpy(loop.queue.gather(loop.qstate, loop.last_idx))
    torch.testing.assert_close(tr._batch_rows.cpu(), ref_batch, atol=2e-4, rtol=2e-4)
    sv = tr._stats_vec.cpu().numpy()
    assert sv[0] == loop.stats[0]
    np.testing.assert_allclose(sv[1:], loop.stats[1:], rtol=2e-5, atol=2e-5)
    P, Q2 = tr.updater.P, 2 * tr.updater.Q
    assert _rel(tr.updater.params[:P], loop.state.params[:P]) < 5e-4
    assert _rel(tr.updater.params[P:P + Q2], loop.state.params[P:P + Q2]) < 5e-4
    assert _rel(tr.updater.target_q, loop.state.target_q) < 5e-4
    ts, es, bs = tr.training_step(ts, es, bs)                       # the epoch's second step
    eager = _sac_state(tr, es, bs)
    tr.close()
    # the same epoch through the hipGraph: first step eager and captured, second step a replay
    tr, ts, es, bs, _ = sac_setup(dev, use_graph=True)
    ts, es, bs, _ = tr.prefill_replay_buffer(ts, es, bs, 17)
    ts, es, bs, _ = tr.training_epoch(ts, es, bs, 19)
    assert tr._graph is not None
    graph = _sac_state(tr, es, bs)
    tr.close()
    for k, v in eager.items():
        assert torch.equal(v, graph[k]), f"graph replay differs from eager in {k}"


# ------------------------------------------------------------------------------------------------ PPO
def ppo_setup(dev, use_graph, bounds=PPO_BOUNDS, n_steps=2):
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    from mbpo.systems.brax_wrapper import BraxWrapper
    system, sp, wrapped = make_system(dev, bounds)
    tb, tbs = _true_buffer(dev, 256)
    env = BraxWrapper(system, sp, tbs, tb)
    tr = PPO(environment=env, num_timesteps=n_steps * 16 * 8 * 4, use_graph=use_graph, **PPO_KW)
    assert tr.num_training_steps_per_epoch == n_steps
    return tr, tr.init_training_state(5), env.reset([101 + i for i in range(PPO_KW["num_envs"])]), wrapped


def ppo_oracle(tr, es, wrapped):
    kw = PPO_KW
    cfg = oppo.PpoConfig(X, U, tr.policy_dims, tr.value_dims, entropy_cost=kw["entropy_cost"], discounting=kw["discounting"],
                         gae_lambda=kw["gae_lambda"], clipping_epsilon=kw["clipping_epsilon"], lr=kw["lr"], wd=kw["wd"])
    return otr.CpuPpoLoop(cfg, wrapped, kw["num_envs"], kw["unroll_length"], kw["episode_length"], kw["batch_size"],
                          kw["num_minibatches"], kw["num_updates_per_batch"], True, init_params=tr.updater.params.cpu().clone(),
                          init_obs=es.obs.cpu().clone())


def _ppo_state(tr, es):
    torch.cuda.synchronize()
    u = tr.updater
    return dict(params=u.params.cpu().clone(), m=u.adam_m.cpu().clone(), v=u.adam_v.cpu().clone(), count=u.step_count.cpu().clone(),
                obs=es.obs.cpu().clone(), steps=es.info["steps"].cpu().clone(), done=es.done.cpu().clone(),
                stats=tr._stats_vec.cpu().clone(), data=tr._data.cpu().clone(), perm=tr._perm.cpu().clone(), rng=tr._rng.cpu().clone())


def test_ppo_training_step_on_a_terminating_system(dev):
    """Two training steps (2 x 2 unrolls of 8 env steps; episode_length 20, so the truncations fall into the second) against
    CpuPpoLoop; the first at the one-step tolerances of tests/test_gpu_trainer_parity.py, the second at its later-step ones."""
    tr, ts, es, wrapped = ppo_setup(dev, use_graph=False)
    loop = ppo_oracle(tr, es, wrapped)
    tr.rekey(19)
    loop.rekey(19)
    snaps = []
    for step in range(2):
        ts, es, _ = tr.training_step(ts, es)
        terms = loop.training_step()
        torch.cuda.synchronize()
        snaps.append(dict(data=tr._data.cpu().clone(), ref=loop.last_data.clone(), perm=tr._perm.cpu().clone(),
                          ref_perm=torch.from_numpy(loop.last_perms[-1]).clone(), sv=tr._stats_vec.cpu().numpy().copy(),
                          ref_sv=np.array(loop.stats, dtype=np.float64), params=tr.updater.params.cpu().clone(),
                          ref_params=loop.state.params.clone(), m=tr.updater.metrics.cpu().tolist(), terms=dict(terms)))
    D = snaps[0]["ref"].shape[-1]
    keep = check_oracle_loop(wrapped, torch.cat([s["ref"].reshape(-1, D)[:, D - 1] for s in snaps]))
    N = PPO_KW["num_envs"]
    P = tr.updater.P
    for step, s in enumerate(snaps):
        got, want = s["data"].reshape(-1, PPO_KW["unroll_length"], D), s["ref"].reshape(-1, PPO_KW["unroll_length"], D)
        kt = keep.repeat(got.shape[0] // N)                           # trajectories are unroll-major: env = trajectory % N
        got, want = got[kt], want[kt]
        for col in (X + U + 1, D - 1):
            assert torch.equal(got[..., col], want[..., col])
        tol = 2e-4 if step == 0 else 3e-3
        torch.testing.assert_close(got, want, atol=tol, rtol=tol)
        assert torch.equal(s["perm"], s["ref_perm"])
        assert s["sv"][0] == s["ref_sv"][0]
        np.testing.assert_allclose(s["sv"][1:], s["ref_sv"][1:], rtol=2e-5 if step == 0 else 5e-4, atol=2e-5)
        lim = 1e-3 if step == 0 else 1e-2
        assert _rel(s["params"][:P], s["ref_params"][:P]) < lim
        assert _rel(s["params"][P:], s["ref_params"][P:]) < lim
        for value, key in zip(s["m"], ("total_loss", "policy_loss", "v_loss", "entropy_loss")):
            assert abs(value - s["terms"][key]) <= (2e-3 if step == 0 else 2e-2) * max(1.0, abs(s["terms"][key])), key
    allref = torch.cat([s["ref"].reshape(-1, D) for s in snaps])
    assert int(((allref[:, X + U + 1] == 0) & (allref[:, D - 1] == 0)).sum()) >= 1      # terminations that are not truncations
    eager = _ppo_state(tr, es)
    tr.close()
    tr, ts, es, _ = ppo_setup(dev, use_graph=True)
    ts, es, _ = tr.training_epoch(ts, es, 19)
    assert tr._graph is not None
    graph = _ppo_state(tr, es)
    tr.close()
    for k, v in eager.items():
        assert torch.equal(v, graph[k]), f"graph replay differs from eager in {k}"
