"""GPU: time-adaptive model rollouts (mbpo_rollout_desc.hold_*; include/mbpo_hip.h "time-adaptive rollouts") against the CPU restatement
(tests/time_adaptive_ref.py) at each case's tolerance (tests/time_adaptive_cases.py), the exact identity of a fixed hold with
action_repeat, mbpo_hold_steps, System.step as one decision, and SAC / PPO on a time-adaptive EnsembleSystem.

tests/test_cpu_time_adaptive.py asserts, on the reference alone, the conditions the parity cases rest on: every k is taken, rows
terminate in the middle of a hold, resets fall inside the launch.
"""
import pytest
import torch

import time_adaptive_cases as tc
import time_adaptive_ref as taref

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", list(tc.CASES))
def test_rollout_matches_the_restatement(dev, name):
    b, ref, k = tc.build(name), tc.oracle(name), tc.kept(name)
    X, A, tol = b["X"], b["A"], tc.tol(name)
    rows, obs, first, steps, done = tc.run_device(name, dev)
    keep, st = k["env"], ref["state"]
    got, want = tc.env_rows(rows, name)[keep], tc.env_rows(ref["rows"], name)[keep]
    D = got.shape[-1]
    print(f"{name}: max |rows - ref| / (1 + |ref|) {float(((got - want).abs() / (1 + want.abs())).max()):.3g} at tol {tol:.3g}, "
          f"kept {int(keep.sum())} of {tc.N}")
    # integer-valued bookkeeping is exact: discount, truncation, steps, done
    assert torch.equal(got[..., X + A + 1], want[..., X + A + 1]) and torch.equal(got[..., D - 1], want[..., D - 1])
    assert torch.equal(steps[keep], st.steps[keep]) and torch.equal(done[keep], st.done[keep])
    torch.testing.assert_close(got, want, atol=tol, rtol=tol)
    torch.testing.assert_close(obs[keep], st.obs[keep], atol=tol, rtol=tol)
    if b["start"]:      # the start states are bit copies of true-buffer rows
        assert torch.equal(first[keep], st.first_obs[keep]) and not torch.equal(first, b["first"])
    else:
        assert torch.equal(first, b["first"])
    assert int((want[..., X + A + 1] == 0).sum()) > 0      # resets inside the launch


@pytest.mark.parametrize("name", list(tc.CASES))
def test_hold_steps_is_the_rollouts_k(dev, name):
    """mbpo_hold_steps on the device run's own actions: the restatement's k on the decisions away from an integer, and the `steps`
    increment of a one-decision launch over the same actions on the rows it neither terminated nor reset."""
    from mbpo import ops
    b, h = tc.build(name), tc.hold(name)
    X, A, K = b["X"], b["A"], b["K"]
    rows = tc.run_device(name, dev)[0]
    acts = tc.env_rows(rows, name)[:, :, X:X + A].permute(1, 0, 2).contiguous()          # [S, N, A]
    k_dev = ops.hold_steps(acts.reshape(-1, A).to(dev), h.t_lo, h.t_hi, h.dt, K).cpu().reshape(tc.S, tc.N).long()
    assert int(k_dev.min()) == 1 and int(k_dev.max()) == K
    far = taref.integer_distance(acts, b["UE"], h) >= tc.INT_MARGIN
    assert float(far.float().mean()) > 0.9
    assert torch.equal(k_dev[far], taref.hold_steps(acts[..., b["UE"]], h)[far])
    # the first decision again, open loop: steps_out - steps_in (zeroed where the env came in done) is the inner steps it took
    kw = tc.device_kwargs(name, dev)
    for key in ("member_idx", "model_noise"):
        if kw.get(key) is not None:
            kw[key] = kw[key][:1].contiguous()
    d = lambda t: t.to(dev).clone()
    steps, done = d(b["steps0"]), d(b["done0"])
    one = ops.model_rollout(x_dim=X, u_dim=A, actions=acts[:1].to(dev).contiguous(), obs=d(b["obs0"]), first_obs=d(b["first"]), steps=steps,
                            done=done, n_steps=1, episode_length=tc.L, **kw)
    torch.cuda.synchronize()
    taken = steps.cpu() - torch.where(b["done0"] != 0, torch.zeros(tc.N), b["steps0"])
    running = done.cpu() == 0                                   # neither terminated nor reset
    assert int(running.sum()) > tc.N // 4
    assert torch.equal(taken[running].long(), k_dev[0][running])
    assert bool((taken >= 1).all()) and bool((taken.long() <= k_dev[0]).all())
    assert torch.equal(one.cpu()[:, X:X + A], acts[0])


# ------------------------------------------------------------------------------------------------ a fixed hold is action_repeat
def _fixed_hold_pair(dev, K, hidden, mode, N=40, S=3, X=3, UE=2, E=3, seed=0):
    """(rows at action_repeat = K over actions [u], rows of the hold t_lo = t_hi = K dt over [u | tau], final states of both)."""
    from mbpo import _hip, ops
    g = torch.Generator().manual_seed(seed)
    ddims = [X + UE, *hidden, 2 * X]
    dpar = tc.member_params(ddims, E, g).to(dev)
    rparams = torch.cat([torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(UE, generator=g)]).to(dev)
    obs0, first0 = torch.randn(N, X, generator=g), torch.randn(N, X, generator=g)
    acts = torch.rand(S, N, UE, generator=g) * 2 - 1
    tau = torch.rand(S, N, 1, generator=g) * 2 - 1
    dt, L = 0.0625, K + 2      # (initial steps are env % 3: every K sees episodes run out)
    kw = dict(system_kind=_hip.SYS_ENSEMBLE, dyn_params=dpar, dyn_spec=ops.MlpSpec(ddims, "swish", E), reward_kind=_hip.REWARD_QUADRATIC,
              reward_params=rparams, n_steps=S, episode_length=L, seed=77, offset=(3 << 32) + 5)
    if mode == "ts1":      # Philox-drawn members and noise: element ((s K + j) N + env) in both runs
        kw.update(ens_mode=_hip.ENS_TS1, ens_sample_noise=True)
    out = []
    for u_dim, actions, extra in ((UE, acts, dict(action_repeat=K)),
                                  (UE + 1, torch.cat([acts, tau], dim=2), dict(hold_max_steps=K, hold_min_time=K * dt, hold_max_time=K * dt,
                                                                               hold_dt=dt, hold_gamma=1.0, hold_switch_cost=0.0))):
        obs, first = obs0.to(dev), first0.to(dev)
        steps, done = (torch.arange(N) % 3).float().to(dev), torch.zeros(N, device=dev)
        rows = ops.model_rollout(x_dim=X, u_dim=u_dim, actions=actions.to(dev).contiguous(), obs=obs, first_obs=first, steps=steps, done=done,
                                 **kw, **extra)
        torch.cuda.synchronize()
        out.append((rows.cpu(), obs.cpu(), steps.cpu(), done.cpu()))
    return out[0], out[1], X, UE


@pytest.mark.parametrize("mode", ["mean", "ts1"])
@pytest.mark.parametrize("hidden", [(64, 64, 64), (128, 128)])
@pytest.mark.parametrize("K", [1, 3])
def test_fixed_hold_is_action_repeat_bit_for_bit(dev, K, hidden, mode):
    (plain, pobs, psteps, pdone), (held, hobs, hsteps, hdone), X, UE = _fixed_hold_pair(dev, K, hidden, mode)
    A = UE + 1
    assert torch.equal(held[:, :X + UE], plain[:, :X + UE])          # obs, controls
    assert torch.equal(held[:, X + A:], plain[:, X + UE:])            # reward, discount, next_observation, truncation
    assert torch.equal(hobs, pobs) and torch.equal(hsteps, psteps) and torch.equal(hdone, pdone)
    assert plain[:, X + UE + 1].min() == 0                            # episodes run out inside the launch


# ------------------------------------------------------------------------------------------------ System.step is one decision
def test_system_step_is_one_decision(dev):
    from mbpo import ops
    from mbpo.systems import BoxTermination, PendulumSystem, TimeAdaptive
    from mbpo.utils import keys as K
    ta = TimeAdaptive(0.05, 0.2499, 0.05, switch_cost=0.2, continuous_discounting=0.5)
    system = PendulumSystem(termination=BoxTermination([-tc.INF, -tc.INF, -3.0], [tc.INF, tc.INF, 3.0]), time_adaptive=ta)
    assert system.action_dim == 2 and ta.max_steps == 4
    g = torch.Generator().manual_seed(3)
    N = 37
    import fresh_start_cases as fc
    x = fc._pendulum_obs(N, g, 2.5).to(dev)
    a = (torch.rand(N, 2, generator=g) * 2 - 1).to(dev)
    sp = system.init_params(0)
    st = system.step(x, a, sp)
    spec = system.rollout_spec(sp, dev)
    obs = x.clone()
    rows = ops.model_rollout(x_dim=3, u_dim=2, actions=a.reshape(1, N, 2), obs=obs, first_obs=x.clone(), steps=torch.zeros(N, device=dev),
                             done=torch.zeros(N, device=dev), n_steps=1, episode_length=2 ** 30, seed=K.split(sp.key)[1], **spec)
    assert torch.equal(st.x_next, rows[:, 7:10]) and torch.equal(st.reward, rows[:, 5]) and torch.equal(st.done, 1 - rows[:, 6])
    k = system.hold_steps(a)
    assert k.dtype == torch.int32 and int(k.min()) >= 1 and int(k.max()) == 4 and len(set(k.tolist())) == 4
    assert float(st.done.sum()) > 0 and float(st.done.sum()) < N
    # one decision of k = 1 rows is one model step of the plain system, less the switch cost
    one = (k == 1) & (st.done == 0)
    assert int(one.sum()) > 0
    plain = PendulumSystem().step(x[one], a[one, :1], PendulumSystem().init_params(0))
    assert torch.equal(plain.x_next, st.x_next[one])
    torch.testing.assert_close(plain.reward - 0.2, st.reward[one], atol=1e-6, rtol=1e-6)
    assert int(system.hold_steps(a[0])) == int(k[0])


# ------------------------------------------------------------------------------------------------ trainers
X, U, E = 3, 1, 5
A = U + 1
TA_KW = dict(min_time_between_switches=0.05, max_time_between_switches=0.2, env_dt=0.05, switch_cost=0.05, continuous_discounting=0.5)
SAC_KW = dict(num_envs=16, batch_size=32, grad_updates_per_step=2, num_env_steps_between_updates=2, episode_length=6,
              normalize_observations=True, max_replay_size=512, min_replay_size=64, discounting=0.95, lr_policy=3e-4, lr_q=3e-4,
              lr_alpha=3e-4)
PPO_KW = dict(num_envs=16, unroll_length=4, batch_size=8, num_minibatches=2, num_updates_per_batch=2, episode_length=8,
              normalize_observations=True, discounting=0.97, lr=3e-4, entropy_cost=1e-2, policy_hidden_layer_sizes=(64, 64),
              critic_hidden_layer_sizes=(64, 64))


def _env(dev, rows=256):
    """A time-adaptive Pendulum-shaped system (x = 3, u_env = 1) behind a BraxWrapper whose TRUE buffer holds u_env-wide actions."""
    from mbpo.replay import UniformSamplingQueue
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, PendulumReward, TimeAdaptive
    from mbpo.systems.brax_wrapper import BraxWrapper
    from mbpo.types import Transition
    ta = TimeAdaptive(**TA_KW)
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=E, device=dev), PendulumReward(), time_adaptive=ta)
    sp = system.init_params(1)
    dummy = Transition(observation=torch.zeros(X), action=torch.zeros(U), reward=torch.zeros(1), discount=torch.zeros(1),
                       next_observation=torch.zeros(X))
    tb = UniformSamplingQueue(rows, dummy, 1, device=dev)
    data = torch.randn(rows, 2 * X + U + 2, generator=torch.Generator().manual_seed(0))
    return BraxWrapper(system, sp, tb.insert_rows(tb.init(0), data.to(dev)), tb), ta


def test_sac_on_a_time_adaptive_system_graph_equals_eager(dev):
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    N, S = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"]

    def run(use_graph):
        env, ta = _env(dev)
        tr = SAC(environment=env, num_timesteps=64 + N * S, use_graph=use_graph, **SAC_KW, **ta.trainer_kwargs())
        assert tr.num_training_steps_per_epoch == 1
        assert (tr.x_dim, tr.u_dim) == (X, A) and tr.policy_dims_logical[-1] == 2 * A and tr.q_dims_logical[0] == X + A
        assert tr.row_len == 2 * X + A + 3
        ts, es, bs = tr.init_training_state(7), tr.reset_envs(env, 11, N), tr.replay_buffer.init(13)
        ts, es, bs, _ = tr.prefill_replay_buffer(ts, es, bs, 17)
        graphs, metrics = [], []
        for epoch in range(3):      # one training step each: eager (and captured), replayed, replayed
            if use_graph:
                ts, es, bs, m = tr.training_epoch(ts, es, bs, 19 + epoch)
                graphs.append(tr._graph)
                metrics += list(m.values())
            else:
                tr.updater.metrics_accum.zero_()
                tr.rekey(19 + epoch)
                ts, es, bs = tr.training_step(ts, es, bs)
                metrics += tr.updater.metrics_accum.cpu().tolist()
        if use_graph:
            assert graphs[0] is not None and graphs[1] is graphs[0] and graphs[2] is graphs[0]
        assert all(v == v and abs(v) != float("inf") for v in metrics), metrics
        torch.cuda.synchronize()
        out = dict(params=tr.updater.params.cpu().clone(), tq=tr.updater.target_q.cpu().clone(), obs=es.obs.cpu().clone(),
                   steps=es.info["steps"].cpu().clone(), stats=tr._stats_vec.cpu().clone(), rows=tr._rollout_rows.cpu().clone(),
                   data=bs.data.cpu().clone(), rng=tr._rng.cpu().clone())
        tr.close()
        return out

    eager, graph = run(False), run(True)
    for k, v in eager.items():
        assert torch.isfinite(v.float()).all(), k
        assert torch.equal(v, graph[k]), f"graph replay differs from eager in {k}"
    rows = eager["rows"]
    assert float(rows[:, X + U].abs().max()) > 0 and float(rows[:, X:X + A].abs().max()) <= 1.0      # tau is sampled, tanh-squashed


def test_ppo_on_a_time_adaptive_system_graph_equals_eager(dev):
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    per_step = PPO_KW["batch_size"] * PPO_KW["unroll_length"] * PPO_KW["num_minibatches"]

    def run(use_graph):
        env, ta = _env(dev)
        tr = PPO(environment=env, num_timesteps=per_step, use_graph=use_graph, **PPO_KW, **ta.trainer_kwargs())
        assert tr.num_training_steps_per_epoch == 1
        assert (tr.x_dim, tr.u_dim) == (X, A) and tr.policy_dims_logical[-1] == 2 * A and tr.row_len == 2 * X + 2 * A + 4
        ts, es = tr.init_training_state(5), env.reset([101 + i for i in range(PPO_KW["num_envs"])])
        graphs, metrics = [], []
        for epoch in range(3):
            if use_graph:
                ts, es, m = tr.training_epoch(ts, es, 19 + epoch)
                graphs.append(tr._graph)
                metrics += list(m.values())
            else:
                tr.updater.metrics_accum.zero_()
                tr.rekey(19 + epoch)
                ts, es, _ = tr.training_step(ts, es)
                metrics += tr.updater.metrics_accum.cpu().tolist()
        if use_graph:
            assert graphs[0] is not None and graphs[1] is graphs[0] and graphs[2] is graphs[0]
        assert all(v == v and abs(v) != float("inf") for v in metrics), metrics
        torch.cuda.synchronize()
        u = tr.updater
        out = dict(params=u.params.cpu().clone(), m=u.adam_m.cpu().clone(), obs=es.obs.cpu().clone(), stats=tr._stats_vec.cpu().clone(),
                   data=tr._data.cpu().clone(), rng=tr._rng.cpu().clone())
        tr.close()
        return out

    eager, graph = run(False), run(True)
    for k, v in eager.items():
        assert torch.isfinite(v.float()).all(), k
        assert torch.equal(v, graph[k]), f"graph replay differs from eager in {k}"
