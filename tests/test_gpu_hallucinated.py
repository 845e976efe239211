"""GPU: hallucinated control in the fused model rollouts (mbpo_rollout_desc.halluc_beta; include/mbpo_hip.h "hallucinated control")
against the CPU restatement (tests/halluc_ref.py) at the project's rollout tolerance (tests/test_gpu_rollout.py: atol = rtol = 2e-4 for
S <= 5), the exact identities with the plain 'mean' rollout, and the three consumers on an optimistic EnsembleSystem.

tests/test_cpu_hallucinated.py asserts, on the reference alone, that the optimistic term of every parity case is more than ten times
the tolerance: a kernel that drops it cannot pass.
"""
import importlib.util
import math
from pathlib import Path

import pytest
import torch

import halluc_cases as hc
import halluc_ref as href
from oracle import nets as onets
from oracle import rollout as oro
from oracle import systems as osys

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", list(hc.CASES))
def test_rollout_matches_the_restatement(dev, name):
    b, ref = hc.build(name), hc.oracle(name)
    X, A = b["X"], b["A"]
    rows, obs, first, steps, done = hc.run_device(name, dev)
    keep, st = ref["keep"], ref["state"]
    got, want = hc.env_rows(rows, name)[keep], hc.env_rows(ref["rows"], name)[keep]
    D = got.shape[-1]
    print(f"{name}: max |rows - ref| {float((got - want).abs().max()):.3g}, mean |beta sd eta| {ref['term_mean']:.3g}, "
          f"kept {int(keep.sum())} of {hc.N}")
    # integer-valued bookkeeping is exact: discount, truncation, steps, done
    assert torch.equal(got[..., X + A + 1], want[..., X + A + 1]) and torch.equal(got[..., D - 1], want[..., D - 1])
    assert torch.equal(steps[keep], st.steps[keep]) and torch.equal(done[keep], st.done[keep])
    torch.testing.assert_close(got, want, atol=hc.ATOL, rtol=hc.ATOL)
    torch.testing.assert_close(obs[keep], st.obs[keep], atol=hc.ATOL, rtol=hc.ATOL)
    if b["start"]:      # the start states are bit copies of true-buffer rows
        assert torch.equal(first[keep], st.first_obs[keep]) and not torch.equal(first, b["first"])
    else:
        assert torch.equal(first, b["first"])
    assert int((want[..., X + A + 1] == 0).sum()) > 0      # resets inside the launch


def test_plain_mean_rollout_after_a_hallucinated_one(dev):
    """Hallucinated and plain runs in one process: the plain 'mean' rollout of the same shape still matches its own oracle."""
    from mbpo import _hip, ops
    name = "c1_64_x3_u2"
    b = hc.build(name)
    hc.run_device(name, dev)
    X, U, E, S = b["X"], b["A"], b["E"], b["S"]      # the plain run at the same action width: its dynamics read all 5 columns
    g = torch.Generator().manual_seed(5)
    ddims = [X + U, 64, 64, 64, 2 * X]
    dpar = hc.member_params(ddims, E, g)
    tgt, q, r = torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(U, generator=g) * 0.1
    osystem = osys.EnsembleSystem(dpar, ddims, E, X, U, reward_fn=lambda x, u: osys.quadratic_reward(x, u, tgt, q, r))
    st_ref, rows_ref = oro.rollout(osystem, b["ppar"], b["pdims"], oro.EnvState(b["obs0"], b["first"], b["steps0"], b["done0"]), S, hc.L,
                                   policy_noise=b["pnoise"])
    obs = b["obs0"].to(dev)
    rows = ops.model_rollout(policy_params=b["ppar"].to(dev), policy_spec=ops.MlpSpec(b["pdims"], "swish", 1), x_dim=X, u_dim=U, obs=obs,
                             first_obs=b["first"].to(dev), steps=b["steps0"].to(dev), done=b["done0"].to(dev), n_steps=S,
                             episode_length=hc.L, system_kind=_hip.SYS_ENSEMBLE, dyn_params=dpar.to(dev),
                             dyn_spec=ops.MlpSpec(ddims, "swish", E), reward_kind=_hip.REWARD_QUADRATIC,
                             reward_params=torch.cat([tgt, q, r]).to(dev), policy_noise=b["pnoise"].to(dev))
    torch.testing.assert_close(rows.cpu(), rows_ref, atol=hc.ATOL, rtol=hc.ATOL)
    torch.testing.assert_close(obs.cpu(), st_ref.obs, atol=hc.ATOL, rtol=hc.ATOL)


# ------------------------------------------------------------------------------------------------ open-loop actions: exact identities
def _openloop(dev, S, E, beta, hidden=(64, 64, 64), X=3, UE=2, N=40, seed=0):
    """(plain 'mean' rows, hallucinated rows) of the same members and controls; the hallucinated run's eta is random."""
    from mbpo import _hip, ops
    g = torch.Generator().manual_seed(seed)
    A = UE + X
    ddims = [X + UE, *hidden, 2 * X]
    dpar = hc.member_params(ddims, E, g).to(dev)
    rparams = torch.cat([torch.randn(X, generator=g), torch.rand(X, generator=g), torch.rand(UE, generator=g)]).to(dev)
    obs0 = torch.randn(N, X, generator=g)
    acts = torch.rand(S, N, UE, generator=g) * 2 - 1
    eta = torch.rand(S, N, X, generator=g) * 2 - 1
    out = []
    for u_dim, actions, extra in ((UE, acts, {}), (A, torch.cat([acts, eta], dim=2), dict(halluc_beta=torch.full((X,), float(beta), device=dev)))):
        z = torch.zeros(N, device=dev)
        rows = ops.model_rollout(x_dim=X, u_dim=u_dim, actions=actions.to(dev).contiguous(), obs=obs0.to(dev), first_obs=obs0.to(dev), steps=z,
                                 done=z.clone(), n_steps=S, episode_length=3, system_kind=_hip.SYS_ENSEMBLE, dyn_params=dpar,
                                 dyn_spec=ops.MlpSpec(ddims, "swish", E), reward_kind=_hip.REWARD_QUADRATIC, reward_params=rparams, **extra)
        out.append(rows.cpu())
    return out[0], out[1], X, UE, A


@pytest.mark.parametrize("hidden", [(64, 64, 64), (128, 128)])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("E,beta", [(5, 0.0), (1, 1.0)])
def test_openloop_beta_zero_or_one_member_is_the_mean_rollout_exactly(dev, S, E, beta, hidden):
    """With beta = 0, or with a single member (sd = 0) and any eta, reward, discount, next observation and truncation equal the plain
    'mean' rollout's bit for bit (the System.step / iCEM path: open-loop `actions`, S = 1 and S = 4)."""
    plain, hal, X, UE, A = _openloop(dev, S, E, beta, hidden)
    assert torch.equal(hal[:, :X], plain[:, :X]) and torch.equal(hal[:, X:X + UE], plain[:, X:X + UE])
    assert torch.equal(hal[:, X + A:], plain[:, X + UE:])      # reward, discount, next_observation, truncation
    assert plain[:, X + UE + 1].min() == 0 or S == 1             # (S = 4: episodes of 3 steps reset inside the launch)


def test_openloop_eta_moves_the_state(dev):
    plain, hal, X, UE, A = _openloop(dev, 1, 5, 1.0)
    assert float((hal[:, X + A + 2:X + A + 2 + X] - plain[:, X + UE + 2:X + UE + 2 + X]).abs().mean()) > 10 * hc.ATOL
    assert torch.equal(hal[:, X + A], plain[:, X + UE])         # the reward never sees eta


# ------------------------------------------------------------------------------------------------ consumers
X, U, E = 3, 1, 5
A = U + X
SAC_KW = dict(num_envs=64, batch_size=256, grad_updates_per_step=4, num_env_steps_between_updates=5, episode_length=5,
              normalize_observations=True, max_replay_size=1500, min_replay_size=64, discounting=0.95, lr_policy=3e-4,
              lr_q=3e-4, lr_alpha=3e-4, wd_q=1e-4)
PPO_KW = dict(num_envs=32, unroll_length=8, batch_size=16, num_minibatches=4, num_updates_per_batch=2, episode_length=20,
              normalize_observations=True, discounting=0.97, lr=3e-4, wd=1e-5, entropy_cost=1e-2, gae_lambda=0.95,
              clipping_epsilon=0.3, policy_hidden_layer_sizes=(64, 64), critic_hidden_layer_sizes=(64, 64))


def _env(dev, rows=512):
    """An optimistic Pendulum-shaped system (x = 3, u_env = 1) behind a BraxWrapper whose TRUE buffer holds u_env-wide actions."""
    from mbpo.replay import UniformSamplingQueue
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, PendulumReward
    from mbpo.systems.brax_wrapper import BraxWrapper
    from mbpo.types import Transition
    system = EnsembleSystem(EnsembleDynamics(X, U, n_members=E, device=dev), PendulumReward(), mode="optimistic", beta=[0.5, 1.0, 2.0])
    sp = system.init_params(1)
    dummy = Transition(observation=torch.zeros(X), action=torch.zeros(U), reward=torch.zeros(1), discount=torch.zeros(1),
                       next_observation=torch.zeros(X))
    tb = UniformSamplingQueue(rows, dummy, 1, device=dev)
    data = torch.randn(rows, 2 * X + U + 2, generator=torch.Generator().manual_seed(0))
    return BraxWrapper(system, sp, tb.insert_rows(tb.init(0), data.to(dev)), tb)


def test_sac_on_an_optimistic_system_graph_equals_eager(dev):
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    N, S = SAC_KW["num_envs"], SAC_KW["num_env_steps_between_updates"]

    def run(use_graph):
        env = _env(dev)
        tr = SAC(environment=env, num_timesteps=64 + N * S * 2, use_graph=use_graph, **SAC_KW)
        assert tr.num_training_steps_per_epoch == 2
        assert (tr.x_dim, tr.u_dim) == (X, A) and tr.policy_dims_logical[-1] == 2 * A and tr.q_dims_logical[0] == X + A
        assert tr.row_len == 2 * X + A + 3 and tr._rollout_rows.shape == (S * N, 2 * X + A + 3)
        ts, es, bs = tr.init_training_state(7), tr.reset_envs(env, 11, N), tr.replay_buffer.init(13)
        ts, es, bs, _ = tr.prefill_replay_buffer(ts, es, bs, 17)
        for epoch in range(2):
            if use_graph:
                ts, es, bs, _ = tr.training_epoch(ts, es, bs, 19 + epoch)
            else:
                tr.rekey(19 + epoch)
                for _ in range(2):
                    ts, es, bs = tr.training_step(ts, es, bs)
        if use_graph:
            assert tr._graph is not None
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
    assert float(rows[:, X + U:X + A].abs().max()) > 0 and float(rows[:, X:X + A].abs().max()) <= 1.0      # eta is sampled, tanh-squashed


def test_ppo_on_an_optimistic_system_graph_equals_eager(dev):
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO

    def run(use_graph):
        env = _env(dev, rows=256)
        tr = PPO(environment=env, num_timesteps=2 * 16 * 8 * 4, use_graph=use_graph, **PPO_KW)
        assert tr.num_training_steps_per_epoch == 2
        assert (tr.x_dim, tr.u_dim) == (X, A) and tr.policy_dims_logical[-1] == 2 * A and tr.row_len == 2 * X + 2 * A + 4
        ts, es = tr.init_training_state(5), env.reset([101 + i for i in range(PPO_KW["num_envs"])])
        if use_graph:
            ts, es, _ = tr.training_epoch(ts, es, 19)
            assert tr._graph is not None
        else:
            tr.rekey(19)
            for _ in range(2):
                ts, es, _ = tr.training_step(ts, es)
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


def test_icem_acts_on_an_optimistic_system(dev):
    from mbpo.optimizers.trajectory_optimizers.icem_optimizer import iCEMOptimizer, iCemParams
    system = _env(dev).system
    small = iCemParams(num_particles=2, num_samples=64, num_elites=8, num_steps=2)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, X, generator=g).to(dev)
    single = iCEMOptimizer(horizon=5, opt_params=small, system=system, key=1)
    a, _ = single.act(x[0], single.init(2))
    assert a.shape == (1, A) and bool(torch.isfinite(a).all())      # (the single-state interface returns [1, action_dim])
    assert system.env_action(a).shape == (1, U)
    batched = iCEMOptimizer(horizon=5, opt_params=small, system=system, key=1, batch_size=4)
    ab, _ = batched.act(x, batched.init(2))
    assert ab.shape == (4, A) and bool(torch.isfinite(ab).all())
    assert float(ab[:, U:].abs().max()) > 0      # the planner optimises eta too


def test_system_step_takes_the_whole_action(dev):
    """System.step (S = 1, open-loop) on the optimistic system against the restatement, single and batched."""
    system = _env(dev).system
    sp = system.init_params(1)
    g = torch.Generator().manual_seed(4)
    x, a = torch.randn(20, X, generator=g), torch.rand(20, A, generator=g) * 2 - 1
    ref = href.HallucinatedEnsembleSystem(sp.dynamics_params.params.cpu(), system.dynamics.dims, E, X, U, system.beta,
                                          reward_fn=lambda xx, uu: osys.pendulum_reward(xx, uu, osys.PendulumParams()))
    xn, r = ref.step(x, a)
    out = system.step(x.to(dev), a.to(dev), sp)
    torch.testing.assert_close(out.x_next.cpu(), xn, atol=2e-5, rtol=2e-5)
    torch.testing.assert_close(out.reward.cpu(), r, atol=2e-5, rtol=2e-5)
    one = system.step(x[0].to(dev), a[0].to(dev), sp)
    assert one.x_next.shape == (X,) and torch.equal(one.x_next.cpu(), out.x_next[0].cpu())


def test_example_runs_optimistic(dev):
    """examples/mbpo_pendulum.py --optimistic: the MBPO loop on an optimistic model, acting on the true Pendulum through env_action."""
    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("mbpo_pendulum_example", root / "examples" / "mbpo_pendulum.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.run(iters=1, n_true=512, model_steps=50, sac_steps=2000, verbose=False, optimistic=1.0)
    assert len(hist) == 1 and math.isfinite(hist[0]["model_nll"]) and math.isfinite(hist[0]["true_return"])
    with pytest.raises(ValueError, match="optimistic"):
        mod.run(iters=1, n_true=512, model_steps=5, sac_steps=2000, verbose=False, optimistic=1.0, real_ratio=0.05)
