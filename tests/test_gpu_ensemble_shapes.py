"""GPU: ensembles of any hidden sizes.  The layered model-learning path of mbpo_ens_nll_grads against fp64 autograd (the criterion of
test_gpu_ensemble_train.py::test_ens_nll_grads_parity), fitting a zero-padded 4 x 200 model (the padding stays exactly zero and the
logical network follows an fp64 AdamW loop), and the rollout consumers running it at the padded width against the oracles on the
LOGICAL network: SAC (graph replay == eager, a fit between replays), PPO, iCEM (single and batched) and a BPTT train step."""
import math

import numpy as np
import pytest
import torch

from oracle import ensemble as oens
from oracle import icem as oicem
from oracle import nets as onets
from oracle import sac as osac
from oracle import systems as osys

import learned_reward_ref as lref
from test_cpu_ensemble_shapes import deep_64_case

pytestmark = pytest.mark.gpu

TARGET, Q, R = [0.1, 0.0, 0.0, 0.0], [1.0, 2.0, 0.5, 0.1], [0.3]
_DEEP = deep_64_case()


# ------------------------------------------------------------------------------------------------ 1. the layered NLL path
@pytest.mark.parametrize("X,U,E,B,hidden,delta,reward,seed", [
    (4, 1, 7, 256, (200,) * 4, True, False, 0),           # MBPO's model
    (4, 1, 3, 64, (200, 100, 50), True, False, 1),        # non-uniform
    (4, 1, 2, 48, (512, 512), True, False, 2),            # above every kernel width
    (_DEEP[0], _DEEP[1], 2, 40, (64,) * _DEEP[2], True, False, 3),    # 64 wide, but past the fused kernel's LDS plan
    (11, 3, 3, 64, (200, 200), True, False, 4),
    (4, 1, 3, 37, (200, 200), True, False, 5),            # ragged batch
    (4, 1, 3, 64, (200, 200), False, False, 6),           # absolute prediction
    (4, 1, 3, 64, (200, 200), True, True, 7),             # reward head fitted at reward_off
    (4, 1, 2, 1500, (128, 96), True, False, 8),           # more than 1024 rows: split-k weight gradients
])
def test_layered_nll_grads_parity(dev, X, U, E, B, hidden, delta, reward, seed):
    from mbpo import ops
    g = torch.Generator().manual_seed(seed)
    dims = [X + U, *hidden, 2 * X + (2 if reward else 0)]
    P = onets.n_params(dims)
    params = torch.cat([onets.init_mlp_flat(dims, g) + 0.02 * torch.randn(P, generator=g) for _ in range(E)])
    R_, D = 500, 2 * X + U + 2
    rows = torch.randn(R_, D, generator=g)
    rows[:, X + U + 2:] = rows[:, :X] + 0.1 * torch.randn(R_, X, generator=g)
    idx = torch.randint(0, R_, (E, B), generator=g)
    roff = X + U if reward else None
    op = ops.EnsembleNllGrad(x_dim=X, u_dim=U, spec=ops.MlpSpec(dims, "swish", E), batch=B, device=dev, predict_delta=delta)
    args = (params.to(dev), rows.to(dev), idx.to(torch.int32).to(dev))
    got = op(*args, reward_off=roff).clone()
    met = op.metrics.clone()
    again = op(*args, reward_off=roff)
    torch.cuda.synchronize()
    assert torch.equal(got, again) and torch.equal(met, op.metrics), "two calls differ"
    if reward:
        ref_g, ref_l = lref.nll_grads(params, dims, E, rows, idx, X, U, delta, 1e-3, reward_off=roff)
        g64, _ = lref.nll_grads(params.double(), dims, E, rows.double(), idx, X, U, delta, 1e-3, reward_off=roff)
    else:
        ref_g, ref_l = oens.nll_grads(params, dims, E, rows, idx, X, U, delta, 1e-3)
        g64, _ = oens.nll_grads(params.double(), dims, E, rows.double(), idx, X, U, delta, 1e-3)
    np.testing.assert_allclose(met.cpu().numpy(), ref_l.numpy(), rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(got.cpu(), ref_g, atol=2e-6, rtol=5e-4)
    rel = float((got.cpu().double() - g64).norm() / g64.norm())
    assert rel < 5e-5, rel


# ------------------------------------------------------------------------------------------------ 2. fitting a padded model
def _rows(n, X, U, seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(n, 2 * X + U + 2, generator=g)
    rows[:, X + U + 2:] = rows[:, :X] + 0.3 * torch.tanh(rows[:, X:X + U]).sum(1, keepdim=True) + 0.05 * torch.randn(n, X, generator=g)
    return rows


def test_padded_fit_keeps_the_padding_and_follows_the_logical_adamw(dev):
    from mbpo import ops
    from mbpo.systems import EnsembleDynamics
    from mbpo.utils import keys as K
    X, U, E, B, lr = 4, 1, 7, 256, 1e-3
    dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=(200,) * 4, device=dev)
    assert dyn.kernel_width == 256
    p = dyn.init_params(3)
    logical0 = dyn.logical_params(p).cpu().clone()
    mask = dyn.from_logical_params(torch.ones_like(logical0)).params != 0
    rows = _rows(2000, X, U, 0).to(dev)
    # 5 steps against fp64 AdamW on the logical network, on the sampler's own indices
    p, _ = dyn.fit(p, rows, num_steps=5, batch_size=B, learning_rate=lr, key=9)
    torch.cuda.synchronize()
    state = torch.tensor([2000, 0, 0, 2000], device=dev, dtype=torch.int32)
    col0, scratch = rows[:, :1].contiguous(), torch.zeros(E * B, 1, device=dev)
    idx = torch.zeros(E * B, device=dev, dtype=torch.int32)
    w = logical0.double()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    rows64 = rows.cpu().double()
    for it in range(5):
        ops.replay_sample(col0, state, E * B, seed=K.PRNGKey(9), offset=it, out=scratch, idx_out=idx)
        g, _ = oens.nll_grads(w, dyn.dims_logical, E, rows64, idx.cpu().long().view(E, B), X, U, True, 1e-3)
        w, m, v = osac.adamw_step(w, g, m, v, it + 1, lr, 0.0)
    torch.testing.assert_close(dyn.logical_params(p).cpu().double(), w, atol=2e-5, rtol=1e-4)
    assert bool((p.params[~mask] == 0).all())
    # 200 more steps (weight decay on): every padded entry is still exactly zero
    dyn2 = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=(200, 100), device=dev)
    p2 = dyn2.init_params(4)
    mask2 = dyn2.from_logical_params(torch.ones(dyn2.logical_params(p2).numel())).params != 0
    p2, losses = dyn2.fit(p2, rows, num_steps=200, batch_size=B, learning_rate=3e-3, weight_decay=1e-4, key=2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all()) and float(losses[-10:].mean()) < float(losses[:10].mean())
    assert int((p2.params[~mask2] != 0).sum()) == 0
    p, _ = dyn.fit(p, rows, num_steps=200, batch_size=B, learning_rate=3e-3, weight_decay=1e-4, key=5)
    torch.cuda.synchronize()
    assert int((p.params[~mask] != 0).sum()) == 0


def test_mbpo_model_learns_pendulum_dynamics(dev):
    """test_ensemble_fit_learns_pendulum_dynamics's thresholds with MBPO's 7 x 4 x 200 model."""
    from mbpo.systems import EnsembleDynamics, PendulumSystem
    system = PendulumSystem()
    g = torch.Generator().manual_seed(0)
    n = 6000
    th = (torch.rand(n, generator=g) * 2 - 1) * math.pi
    x = torch.stack([torch.cos(th), torch.sin(th), (torch.rand(n, generator=g) * 2 - 1) * 6], 1).to(dev)
    u = (torch.rand(n, 1, generator=g) * 2 - 1).to(dev)
    nxt = system.step(x, u, system.reset().system_params)
    rows = torch.cat([x, u, nxt.reward[:, None], torch.ones(n, 1, device=dev), nxt.x_next], 1)
    train, test = rows[:5000], rows[5000:]
    dyn = EnsembleDynamics(3, 1, n_members=7, hidden_layer_sizes=(200,) * 4)
    params = dyn.init_params(1)
    params, losses = dyn.fit(params, train, num_steps=1500, batch_size=256, learning_rate=3e-3, key=7)
    l0, l1 = float(losses[:20].mean()), float(losses[-20:].mean())
    assert l1 < l0 - 3.0, (l0, l1)
    dist, _ = dyn.next_state(test[:, :3], test[:, 3:4], params)
    err = float((dist.mean() - test[:, 6:9]).abs().mean())
    base = float((test[:, :3] - test[:, 6:9]).abs().mean())
    assert err < 0.25 * base, (err, base)


def test_wide_model_runs_layer_by_layer(dev):
    """Above 256 the parameters are logical: member_outputs against the oracle; the rollout consumers refuse by name."""
    from mbpo import _hip
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    X, U, E = 4, 1, 2
    dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=(512, 300), device=dev)
    p = dyn.init_params(2)
    assert dyn.kernel_width is None and p.params.numel() == E * onets.n_params(dyn.dims_logical)
    x = torch.randn(33, X, device=dev)
    u = torch.randn(33, U, device=dev)
    y = dyn.member_outputs(x, u, p)
    ref = onets.ensemble_forward(p.params.cpu(), dyn.dims_logical, E, torch.cat([x, u], 1).cpu())
    torch.testing.assert_close(y.cpu(), ref, atol=1e-4, rtol=1e-4)
    p, losses = dyn.fit(p, _rows(500, X, U, 1).to(dev), num_steps=3, batch_size=64)
    assert bool(torch.isfinite(losses).all())
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    from mbpo.systems.brax_wrapper import BraxWrapper
    import test_gpu_trainer_parity as tp
    system = EnsembleSystem(dyn, QuadraticReward(X, U, target=TARGET, q=Q, r=R))
    tb, tbs = tp._true_buffer(dev, X, U, 64)
    env = BraxWrapper(system, system.init_params(1), tbs, tb)
    with pytest.raises(_hip.MbpoHipError, match="hidden width 512"):
        SAC(environment=env, num_timesteps=64 + 64 * 5 * 4, **tp.SAC_KW)


# ------------------------------------------------------------------------------------------------ 3. rollouts at the padded width
def _mbpo_system(dev, mode="mean", E=7):
    from mbpo.systems import EnsembleDynamics, EnsembleSystem, QuadraticReward
    X, U = 4, 1
    dyn = EnsembleDynamics(X, U, n_members=E, hidden_layer_sizes=(200,) * 4, device=dev)
    system = EnsembleSystem(dyn, QuadraticReward(X, U, target=TARGET, q=Q, r=R), mode=mode)
    sp = system.init_params(1)
    sp.dynamics_params.params.mul_(0.5)
    osystem = osys.EnsembleSystem(dyn.logical_params(sp.dynamics_params).cpu().clone(), dyn.dims_logical, E, X, U, mode=mode,
                                  reward_fn=lambda a, b: osys.quadratic_reward(a, b, torch.tensor(TARGET), torch.tensor(Q),
                                                                               torch.tensor(R)))
    return system, sp, osystem, X, U


def _member_residual(osystem, rows, X, U):
    """min over members of |next_obs - (obs + mu_m(obs, a))| per row: 'ts1' rows must come from one member of the logical model."""
    obs, act, nxt = rows[:, :X].double(), rows[:, X:X + U].double(), rows[:, X + U + 2:2 * X + U + 2].double()
    y = onets.ensemble_forward(osystem.params.double(), osystem.dims, osystem.E, torch.cat([obs, act], 1))
    return (nxt[None] - (obs[None] + y[:, :, :X])).abs().amax(2).amin(0)


@pytest.mark.parametrize("mode", ["mean", "ts1"])
def test_sac_on_mbpo_model_graph_equals_eager_and_oracle(dev, mode):
    """SAC (policy (64, 64) padded to 256 beside the 256-padded model) through the captured hipGraph == the same epochs issued eagerly,
    bit for bit, with a fit of the model between the epochs (the replay reads the fitted parameters); the rows against the oracle on
    the logical model: in 'mean' CpuSacLoop's rows, in 'ts1' every row is one logical member's prediction."""
    from mbpo.optimizers.policy_optimizers.sac.sac import SAC
    from mbpo.systems.brax_wrapper import BraxWrapper
    from mbpo.utils import keys as K
    from oracle import trainer as otr
    import test_gpu_trainer_parity as tp
    kw = dict(tp.SAC_KW, policy_hidden_layer_sizes=(64, 64), critic_hidden_layer_sizes=(64, 64))
    fit_rows = _rows(800, 4, 1, 3).to(dev)
    out = []
    for use_graph in (False, True):
        system, sp, osystem, X, U = _mbpo_system(dev, mode)
        tb, tbs = tp._true_buffer(dev, X, U, 512)
        env = BraxWrapper(system, sp, tbs, tb)
        N, S = kw["num_envs"], kw["num_env_steps_between_updates"]
        tr = SAC(environment=env, num_timesteps=64 + N * S * 4, use_graph=use_graph, **kw)
        assert tr.kernel_width == 256 and tr.policy_dims == [X, 256, 256, 2 * U]
        ts, es, bs = tr.init_training_state(7), tr.reset_envs(env, 11, N), tr.replay_buffer.init(13)
        loop = None
        if use_graph and mode == "mean":
            cfg = osac.SacConfig(X, U, tr.policy_dims, tr.q_dims, discounting=kw["discounting"], lr_policy=3e-4, lr_q=3e-4,
                                 lr_alpha=3e-4, wd_q=1e-4)
            loop = otr.CpuSacLoop(cfg, osystem, N, S, kw["episode_length"], kw["batch_size"], kw["grad_updates_per_step"],
                                  kw["max_replay_size"], True, init_params=tr.updater.params.cpu().clone(), init_obs=es.obs.cpu().clone())
        ts, es, bs, _ = tr.prefill_replay_buffer(ts, es, bs, 17)
        ts, es, bs, _ = tr.training_epoch(ts, es, bs, 19)
        torch.cuda.synchronize()
        rows1 = tr._rollout_rows.cpu().clone()
        params1 = tr.updater.params.cpu().clone()
        osys_before = osystem.params.clone()
        system.dynamics.fit(sp.dynamics_params, fit_rows, num_steps=3, batch_size=64, learning_rate=1e-2, key=4)
        ts, es, bs, metrics = tr.training_epoch(ts, es, bs, 23)
        torch.cuda.synchronize()
        assert (tr._graph is not None) == use_graph
        out.append(dict(rows1=rows1, params1=params1, rows=tr._rollout_rows.cpu().clone(), params=tr.updater.params.cpu().clone(),
                        obs=es.obs.cpu().clone(), data=bs.data.cpu().clone(), metrics=metrics,
                        logical=system.dynamics.logical_params(sp.dynamics_params).cpu().clone()))
        if loop is not None:
            loop.rekey(K.split(17)[0])
            loop.prefill_step()
            loop.rekey(19)
            for _ in range(4):
                loop.training_step()
            torch.testing.assert_close(rows1, loop.last_rows, atol=5e-3, rtol=5e-3)
            P = tr.updater.P
            assert tp._rel(params1[:P], loop.state.params[:P]) < 5e-3
        # the rows of the last epoch come from the fitted logical model (a truncated row's next_obs is the reset observation)
        osystem.params = out[-1]["logical"]
        assert not torch.equal(osys_before, osystem.params)
        rows = out[-1]["rows"]
        rows = rows[rows[:, -1] == 0]
        assert rows.shape[0] >= out[-1]["rows"].shape[0] // 2
        res = _member_residual(osystem, rows, X, U)
        if mode == "mean":
            xn, r = osystem.step(rows[:, :X], rows[:, X:X + U])
            torch.testing.assert_close(rows[:, X + U + 2:2 * X + U + 2], xn, atol=2e-4, rtol=2e-4)
            torch.testing.assert_close(rows[:, X + U], r, atol=2e-4, rtol=2e-4)
        else:
            assert float(res.max()) < 2e-4, float(res.max())
    a, b = out
    for k in ("rows1", "params1", "rows", "params", "obs", "data"):
        assert torch.equal(a[k], b[k]), f"graph replay differs from eager in {k}"
    assert a["metrics"] == b["metrics"]


def test_ppo_on_mbpo_model_matches_cpu_oracle(dev):
    from mbpo.optimizers.policy_optimizers.ppo.ppo import PPO
    from mbpo.systems.brax_wrapper import BraxWrapper
    from oracle import ppo as oppo, trainer as otr
    import test_gpu_trainer_parity as tp
    system, sp, osystem, X, U = _mbpo_system(dev)
    tb, tbs = tp._true_buffer(dev, X, U, 256)
    env = BraxWrapper(system, sp, tbs, tb)
    kw = tp.PPO_KW
    tr = PPO(environment=env, num_timesteps=3 * 16 * 8 * 4, **kw)
    assert tr.kernel_width == 256
    ts = tr.init_training_state(5)
    es = env.reset([101 + i for i in range(kw["num_envs"])])
    cfg = oppo.PpoConfig(X, U, tr.policy_dims, tr.value_dims, entropy_cost=kw["entropy_cost"], discounting=kw["discounting"],
                         gae_lambda=kw["gae_lambda"], clipping_epsilon=kw["clipping_epsilon"], lr=kw["lr"], wd=kw["wd"])
    loop = otr.CpuPpoLoop(cfg, osystem, kw["num_envs"], kw["unroll_length"], kw["episode_length"], kw["batch_size"],
                          kw["num_minibatches"], kw["num_updates_per_batch"], True, init_params=tr.updater.params.cpu().clone(),
                          init_obs=es.obs.cpu().clone())
    tr.rekey(23)
    loop.rekey(23)
    ts, es, _ = tr.training_step(ts, es)
    loop.training_step()
    torch.cuda.synchronize()
    torch.testing.assert_close(tr._data.cpu(), loop.last_data, atol=2e-4, rtol=2e-4)
    assert tp._rel(tr.updater.params, loop.state.params) < 1e-3
    tr.close()


def test_icem_on_mbpo_model_matches_oracle_loop(dev):
    """iCemTO.optimize through the open-loop rollout at the padded width vs the numpy loop on the logical model; the batched
    optimize equals single calls bit for bit."""
    from mbpo.optimizers import iCemParams, iCemTO
    from mbpo.utils import keys as K
    from test_gpu_icem_batched import _compare_with_single_calls
    params = iCemParams(num_particles=2, num_samples=120, num_elites=12, num_steps=3, exponent=1.0, alpha=0.1, init_std=0.6)
    H = 6
    system, sp, osystem, X, U = _mbpo_system(dev)
    opt = iCemTO(horizon=H, action_dim=U, opt_params=params, key=5)
    opt.set_system(system)
    st = opt.init(7)
    st = st.replace(system_params=sp, best_sequence=(torch.rand(H, U, device=dev) - 0.5))
    x0 = torch.tensor([0.3, -0.2, 0.1, 0.4], device=dev)
    new = opt.optimize(x0, st)
    torch.cuda.synchronize()

    def step(x, u):
        xn, r = osystem.step(torch.from_numpy(x).float(), torch.from_numpy(u).float())
        return xn.double().numpy(), r.double().numpy()

    bs = st.best_sequence.cpu().double().numpy()
    mean = np.zeros((H, U)); mean[:-1] = bs[1:]; mean[-1] = bs[-1]
    std = np.full((H, U), params.init_std)
    best_v, best_s = -np.inf, mean.copy()
    nprev = max(int(params.elite_set_fraction * params.num_elites), 1)
    prev = np.zeros((nprev, H, U))
    carry, _ = K.split(st.key, 2)
    for it in range(params.num_steps):
        sampling_key, _pk = K.split(carry, 2)
        carry = K.split(sampling_key, 2)[0]
        cand = oicem.sample_candidates(mean, std, prev, -1.0, 1.0, params.num_samples, H, U, params.exponent, sampling_key, it)
        vals = oicem.objective(step, x0.cpu().double().numpy(), cand, params.num_particles)
        mean, std, best_v, best_s, prev = oicem.update(vals, cand, mean, std, best_v, best_s, params.num_elites, nprev, params.alpha)
    assert abs(float(new.best_reward) - best_v) <= 2e-3 * max(1.0, abs(best_v))
    np.testing.assert_allclose(new.best_sequence.cpu().numpy(), best_s, atol=5e-3)
    g = torch.Generator().manual_seed(3)
    xb = (torch.randn(3, X, generator=g) * 0.5).to(dev)
    warm = ((torch.rand(3, H, U, generator=g) - 0.5) * 1.5).to(dev)
    bnew = _compare_with_single_calls(opt, xb, warm)
    assert torch.isfinite(bnew.best_reward).all()


def test_bptt_step_through_mbpo_model_matches_cpu_oracle(dev):
    """A BPTTOptimizer with 64-wide actor and critic on a 200-wide ensemble: the wide path (the fused BPTT kernel needs a 64-wide
    model), one train step against oracle.bptt.CpuBpttLoop on the logical model."""
    from mbpo.optimizers import BPTTOptimizer
    from mbpo.replay import UniformSamplingQueue
    from mbpo.types import Transition
    from oracle import bptt as obptt
    n, H, kc = 24, 6, 2
    system, sp, osystem, X, U = _mbpo_system(dev, E=3)
    g = torch.Generator().manual_seed(3)
    q = UniformSamplingQueue(16, Transition(observation=torch.zeros(X), action=torch.zeros(U), reward=torch.zeros(1),
                                            discount=torch.zeros(1), next_observation=torch.zeros(X)), 1, device=dev)
    sbs = q.insert_rows(q.init(0), torch.randn(16, 2 * X + U + 2, generator=g).to(dev))
    opt = BPTTOptimizer(action_dim=U, obs_dim=X, horizon=H, num_samples_per_gradient_update=n, train_steps=1, init_stddev=1.5,
                        critic_updates_per_policy_update=kc, sampling_buffer_size=4096, actor_features=(64, 64),
                        critic_features=(64, 64))
    opt.set_system(system)
    st0 = opt.init(key=11, true_buffer_state=sbs)
    assert not opt.wide and opt.actor_dims == [X, 64, 64, 2 * U]
    out1 = opt.train(bptt_state=st0)
    assert not opt._last_train_captured
    dp = st0.system_params.dynamics_params
    tsys = obptt.TorchEnsembleSystem(system.dynamics.logical_params(dp).cpu().clone(), system.dynamics.dims_logical, 3, X, U,
                                     torch.tensor(TARGET), torch.tensor(Q), torch.tensor(R))
    cfg = obptt.BpttConfig(x_dim=X, u_dim=U, actor_dims=opt.actor_dims, critic_dims=opt.critic_dims, horizon=H, init_stddev=1.5)
    loop = obptt.CpuBpttLoop(cfg, tsys, st0.actor_params.cpu(), st0.critic_params.cpu(), sbs.data.cpu(), n, kc, opt._last_seeds,
                             buffer_size=4096)
    r = loop.step()
    s1, o1 = out1.bptt_summary, out1.optimizer_state
    assert abs(float(s1.actor_loss[0]) - r["actor_loss"]) <= 2e-5 * max(1.0, abs(r["actor_loss"]))
    assert abs(float(s1.critic_loss[0]) - r["critic_loss"]) <= 1e-4 * max(1.0, abs(r["critic_loss"]))
    assert abs(float(s1.actor_grad_norm[0]) - r["actor_grad_norm"]) <= 2e-3 * r["actor_grad_norm"]
    rel = lambda a, b: float((a.cpu() - b).norm() / b.norm())
    assert rel(o1.actor_params, loop.ap) < 2e-4 and rel(o1.critic_params, loop.cp) < 2e-4
